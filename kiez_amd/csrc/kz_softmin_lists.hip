// SINKHORN AND THE INVERTED SOFTMAX ON THE CANDIDATE LISTS: the soft-min potentials with the transport plan
// restricted to the pairs of the neighbour lists dist / ind [n_q, k] (float64 / int64).  Entry (i, c) is a PAIR of source row i and
// target row ind[i, c] when 0 <= ind[i, c] < n_index -- kz_match.hip's rule; any other id (-1, the INT_MAX padding of
// kz_knn_reduced, an id >= n_index) is no pair.  kz_softmin_rows recomputes n_q n_index distances per step; here a step reads the
// n_q k listed ones.  Three pieces:
//   (a) kz_lists_transpose: the column-major view of the pairs (colptr, col_row, col_val), entries of a column in ascending flat
//       position i k + c -- a STABLE radix sort of (target id, flat position) (kz_sort.hip), one gather behind it, colptr by binary
//       search in the sorted ids.  No atomic places an entry: the arrays are the same in every run.
//   (b) kz_softmin_list_rows / kz_softmin_list_cols: softmin_eps(x) = m - eps log sum exp(-(x - m) / eps), m = min x taken out before
//       the sum, over a row's pairs / a column's entries, in float64.
//   (c) kz_sinkhorn_lists: the loop of Sinkhorn._potentials over (b), every launch queued at once, the stopping rule decided on the
//       device.
//
// THE TREE RULE.  A row: k <= 64 -- a group of G = the next power of two >= k lanes holds the row (64 / G rows per wave), lane c the
// entry c, the values stay in registers between the minimum and the sum, both taken by xor butterflies inside the group (both
// partners add the same two numbers: every lane ends with the same bits); k > 64 -- one wave per row, lane l the entries l, l + 64,
// ... in ascending order, then the butterfly over the 64 lanes.  Places that hold no pair are +inf and add exact zeros: the tree is a
// function of k alone.  A column: its entries are cut into chunks of KZ_SOFTMIN_LIST_CHUNK from the column's OWN first entry; a
// chunk is reduced by one wave to (m, s) (KzSoftminPart) -- lane l the entries l, l + 64, ... of the chunk, then the butterfly -- and
// a column of more than one chunk folds its parts, lane l the chunks l, l + 64, ... in ascending order, then the butterfly.  The
// tree is a function of the column's entry count and KZ_SOFTMIN_LIST_CHUNK alone: not of where the column lies in col_val, not of
// what else is in the call.  No float atomics anywhere; the same bits from run to run.
//
// SPECIAL VALUES, as kz_softmin_rows: a NaN value (a NaN distance, a NaN offset) counts as +inf; a set with no entry below +inf
// gives +inf + shift, one with a -inf gives -inf.  New here: a row or column with NO PAIR AT ALL gives NaN -- "no value": a target
// that nobody lists has no potential.
#include "kz_common.h"
#include "kz_reduce.h"   // KzSoftminPart, kz_softmin_rescaled
#include "kz_rows.h"     // kz_csr_row_of (also the column of a place of the view), kz_sl_require, kz_csr_require, kz_csr_validate

constexpr int KZ_SL_CHUNK = 512;   // entries of a column per first-level wave: 8 loads per lane, all in flight
static_assert(KZ_SL_CHUNK == KZ_SOFTMIN_LIST_CHUNK, "include/kiez_amd.h documents the chunk size");
static_assert(KZ_SL_CHUNK % 64 == 0, "a chunk is whole rounds of a wave");

namespace {

// A kernel of iteration `it` of kz_sinkhorn_lists returns at once when the loop stopped at an earlier iteration (*stop: 0 = not
// stopped, else the iteration whose column step met the tolerance -- its own row step is still taken).  stop == NULL: never.
__device__ __forceinline__ bool kz_sl_stopped(const int* __restrict__ stop, int it) {
    if (!stop) return false;
    const int s = *stop;
    return s != 0 && s < it;
}

__device__ __forceinline__ double kz_sl_min(double a, double b) { return b < a ? b : a; }

// x -> the term of the sum, for a finite minimum m (x = +inf: exp(-inf) = exactly 0)
__device__ __forceinline__ double kz_sl_term(double x, double m, double eps) { return exp(-((x - m) / eps)); }

// (m, s) of a set, or its "no entry" mark, -> the result
__device__ __forceinline__ double kz_sl_finish(double m, double s, double eps, double shift) {
    if (m == INFINITY) return m + shift;
    if (m == -INFINITY) return m;
    return (m - eps * log(s)) + shift;
}

// ---- (a) transposition ---------------------------------------------------------------------------------------------------------
// key[p] = the target id of entry p = i k + c (a pair) or n_index (no pair: sorts behind every column), as the bit pattern the
// float sort orders like the integer (ids < 2^31: kz_sort_key_bits flips the sign bit only); val[p] = p
__global__ __launch_bounds__(256) void kz_sl_keys_kernel(const int64_t* __restrict__ ind, int total, int64_t n_index, int* __restrict__ key,
                                                         int* __restrict__ val) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int64_t t = ind[p];
        key[p] = (int)(t >= 0 && t < n_index ? t : n_index);
        val[p] = (int)p;
    }
}

// behind the sort: place p < nnz of the column-major view is the entry at flat position pos[p]
__global__ __launch_bounds__(256) void kz_sl_gather_kernel(const int* __restrict__ key, const int* __restrict__ pos, int total, int k, int64_t n_index,
                                                           const double* __restrict__ dist, int* __restrict__ col_row, double* __restrict__ col_val) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        if (key[p] >= n_index) continue;   // (the non-pairs: the tail of the sorted order)
        const int q = pos[p];
        col_row[p] = q / k;
        col_val[p] = dist[q];
    }
}

// colptr[j] = the first place of the sorted keys with key >= j, j = 0 .. n_index (colptr[n_index] = nnz)
__global__ __launch_bounds__(256) void kz_sl_colptr_kernel(const int* __restrict__ key, int total, int64_t n_index, int64_t* __restrict__ colptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.x * blockDim.x + threadIdx.x; j <= n_index; j += stride) {
        int lo = 0, hi = total;   // (the answer lies in [lo, hi])
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (key[mid] < j)
                lo = mid + 1;
            else
                hi = mid;
        }
        colptr[j] = lo;
    }
}

// ---- (b) rows ------------------------------------------------------------------------------------------------------------------
// x of entry (i, c): dist - off[target], NaN -> +inf; pair = false: +inf and not counted
__device__ __forceinline__ double kz_sl_row_entry(const double* __restrict__ dist, const int64_t* __restrict__ ind, int64_t e, int64_t n_index,
                                                  const double* __restrict__ off, bool& pair) {
    const int64_t t = ind[e];
    pair = t >= 0 && t < n_index;
    if (!pair) return INFINITY;
    double x = dist[e];
    if (off) x = x - off[t];
    return x == x ? x : INFINITY;
}

// k <= 64: G lanes per row (G = the next power of two >= k), 256 / G rows per workgroup.  Rows of one wave end differently (a row
// without a pair, an infinite minimum): selects, no branch around a shuffle.
__global__ __launch_bounds__(256) void kz_sl_rows_group_kernel(const double* __restrict__ dist, const int64_t* __restrict__ ind, int n_q, int k, int G,
                                                               int64_t n_index, double eps, const double* __restrict__ off, double shift,
                                                               double* __restrict__ out, const int* __restrict__ stop, int it) {
    if (kz_sl_stopped(stop, it)) return;
    const int c = threadIdx.x & (G - 1);
    const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = i < n_q && c < k;
    bool pair = false;
    const double x = live ? kz_sl_row_entry(dist, ind, i * k + c, n_index, off, pair) : INFINITY;
    double m = x;
    int any = pair ? 1 : 0;
    for (int sh = G >> 1; sh >= 1; sh >>= 1) {
        m = kz_sl_min(m, __shfl_xor(m, sh, 64));
        any |= __shfl_xor(any, sh, 64);
    }
    const bool finite = m > -INFINITY && m < INFINITY;
    double s = finite ? kz_sl_term(x, m, eps) : 0.0;
    for (int sh = G >> 1; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (i < n_q && c == 0) out[i] = any ? kz_sl_finish(m, s, eps, shift) : (double)NAN;
}

// k > 64: one wave per row, four rows per workgroup; the row is read twice (the second time out of L2)
__global__ __launch_bounds__(256) void kz_sl_rows_wave_kernel(const double* __restrict__ dist, const int64_t* __restrict__ ind, int n_q, int k,
                                                              int64_t n_index, double eps, const double* __restrict__ off, double shift,
                                                              double* __restrict__ out, const int* __restrict__ stop, int it) {
    if (kz_sl_stopped(stop, it)) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_q) return;   // (wave-uniform)
    const int64_t e0 = i * k;
    double m = INFINITY;
    int any = 0;
    for (int c = lane; c < k; c += 64) {
        bool pair;
        m = kz_sl_min(m, kz_sl_row_entry(dist, ind, e0 + c, n_index, off, pair));
        any |= pair ? 1 : 0;
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        m = kz_sl_min(m, __shfl_xor(m, sh, 64));
        any |= __shfl_xor(any, sh, 64);
    }
    if (!any || m == INFINITY || m == -INFINITY) {   // (wave-uniform)
        if (lane == 0) out[i] = any ? kz_sl_finish(m, 0.0, eps, shift) : (double)NAN;
        return;
    }
    double s = 0.0;
    for (int c = lane; c < k; c += 64) {
        bool pair;
        s += kz_sl_term(kz_sl_row_entry(dist, ind, e0 + c, n_index, off, pair), m, eps);
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) out[i] = kz_sl_finish(m, s, eps, shift);
}

// ---- (b) columns ---------------------------------------------------------------------------------------------------------------
// One wave: (m, s) of the entries [p0, p1) of a column, p1 - p0 <= KZ_SL_CHUNK.  Lane l holds the entries p0 + l, p0 + l + 64, ... in
// registers; places behind p1 are +inf and add exact zeros, so the tree is that of a full chunk.  Every lane returns the same part.
// I: the type of the ids beside the values -- int32 source rows in the view kz_lists_transpose writes, int64 target ids where the
// "columns" are the ROWS of a CSR (kz_softmin_csr_rows).  CHECK (the CSR rows): an id outside [0, n_off) is no pair -- +inf, an exact
// zero in the same place of the same tree, and off is not read --, and a chunk without any pair is (+inf, -1): the mark the fold
// turns into NaN (kz_softmin_rescaled gives 0 for any +inf part).  Without CHECK every entry is a pair, as the view holds pairs only.
template <typename I, bool CHECK>
__device__ __forceinline__ KzSoftminPart kz_sl_chunk(const I* __restrict__ col_row, const double* __restrict__ col_val, int64_t p0, int64_t p1,
                                                     const double* __restrict__ off, int64_t n_off, double eps, int lane) {
    constexpr int U = KZ_SL_CHUNK / 64;
    double x[U];
    double m = INFINITY;
    bool any = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + 64 * u + lane;
        double xu = INFINITY;
        if (p < p1) {
            const int64_t r = CHECK || off ? (int64_t)col_row[p] : 0;
            if (!CHECK || (r >= 0 && r < n_off)) {
                any = true;
                xu = col_val[p];
                if (off) xu = xu - off[r];
                xu = xu == xu ? xu : INFINITY;
            }
        }
        x[u] = xu;
        m = kz_sl_min(m, xu);
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) m = kz_sl_min(m, __shfl_xor(m, sh, 64));
    if (CHECK && m == INFINITY) return KzSoftminPart{m, __ballot(any) != 0ull ? 0.0 : -1.0};   // (wave-uniform, as the next)
    if (m == INFINITY || m == -INFINITY) return KzSoftminPart{m, m < 0.0 ? 1.0 : 0.0};
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) s += kz_sl_term(x[u], m, eps);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    return KzSoftminPart{m, s};
}

// the gather behind the sort of a CSR's entries: the source row of flat position q is the row of indptr that holds it (empty rows
// hold nothing: the search steps over them)
__global__ __launch_bounds__(256) void kz_sl_gather_csr_kernel(const int* __restrict__ key, const int* __restrict__ pos, int total,
                                                               const int64_t* __restrict__ indptr, int64_t n_q, int64_t n_index,
                                                               const double* __restrict__ dist, int* __restrict__ col_row, double* __restrict__ col_val) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        if (key[p] >= n_index) continue;
        const int q = pos[p];
        col_row[p] = (int)kz_csr_row_of(indptr, n_q, q);
        col_val[p] = dist[q];
    }
}

// where the part of chunk c of a column that starts at place `start` lies: chunk starts of one column are KZ_SL_CHUNK apart, and a
// LONG column (more than one chunk) spans more than a block of KZ_SL_CHUNK places, so a block [b C, (b + 1) C) of places holds at
// most two chunk starts of long columns -- one of a later chunk (c >= 1: slot 0; its column holds place b C) and one of a first
// chunk (c == 0: slot 1; its column holds place (b + 1) C - 1).  No table, no count: the slot follows from colptr alone.
__device__ __forceinline__ int64_t kz_sl_part_slot(int64_t start, int64_t c) { return 2 * ((start + c * KZ_SL_CHUNK) / KZ_SL_CHUNK) + (c == 0 ? 1 : 0); }

// Level 1, the LONG columns only: wave w = (block b of KZ_SL_CHUNK places, slot) finds the chunk start of its slot by binary search
// in colptr, if there is one, and writes the chunk's part.  The grid covers the capacity of the view; blocks behind nnz return.
template <typename I, bool CHECK>
__global__ __launch_bounds__(256) void kz_sl_cols_chunk_kernel(const int64_t* __restrict__ colptr, const I* __restrict__ col_row,
                                                               const double* __restrict__ col_val, int64_t n_index, int64_t capacity, double eps,
                                                               const double* __restrict__ off, int64_t n_off, KzSoftminPart* __restrict__ part,
                                                               const int* __restrict__ stop, int it) {
    if (kz_sl_stopped(stop, it)) return;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t b = w >> 1;
    const int slot = (int)(w & 1);
    if (b * KZ_SL_CHUNK >= capacity) return;   // (everything below is wave-uniform)
    const int64_t nnz = colptr[n_index];
    if (nnz > capacity) return;   // (a colptr that does not belong to this view: nothing is read)
    const int64_t lo = b * KZ_SL_CHUNK, hi = lo + KZ_SL_CHUNK;
    if (lo >= nnz || (slot == 1 && hi > nnz)) return;   // (a long column that starts in the block ends behind it)
    const int64_t j = kz_csr_row_of(colptr, n_index, slot == 0 ? lo : hi - 1);   // (the column that holds the place: colptr is the view's indptr)
    const int64_t start = colptr[j], end = colptr[j + 1];
    if (end - start <= KZ_SL_CHUNK) return;   // (a short column: level 2 reduces it by itself)
    int64_t p0;
    if (slot == 0) {
        if (start >= lo) return;   // (its first chunk: slot 1's)
        p0 = start + ((lo - start + KZ_SL_CHUNK - 1) / KZ_SL_CHUNK) * KZ_SL_CHUNK;
        if (p0 >= end) return;
    } else {
        if (start < lo) return;
        p0 = start;
    }
    const int64_t p1 = p0 + KZ_SL_CHUNK < end ? p0 + KZ_SL_CHUNK : end;
    const KzSoftminPart pt = kz_sl_chunk<I, CHECK>(col_row, col_val, p0, p1, off, n_off, eps, lane);
    if (lane == 0) part[2 * b + slot] = pt;
}

// Level 2: one wave per column, four columns per workgroup.  No entry: NaN.  One chunk: reduced here.  More: the parts of level 1
// folded as kz_softmin_fold_kernel folds those of kz_softmin_rows.
template <typename I, bool CHECK>
__global__ __launch_bounds__(256) void kz_sl_cols_kernel(const int64_t* __restrict__ colptr, const I* __restrict__ col_row,
                                                         const double* __restrict__ col_val, int64_t n_index, int64_t capacity, double eps,
                                                         const double* __restrict__ off, int64_t n_off, double shift,
                                                         const KzSoftminPart* __restrict__ part, double* __restrict__ out,
                                                         const int* __restrict__ stop, int it) {
    if (kz_sl_stopped(stop, it)) return;
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_index) return;   // (wave-uniform, as everything that branches below)
    const int64_t start = colptr[j], end = colptr[j + 1], n = end - start;
    if (n <= 0 || start < 0 || end > capacity) {   // (no entry; or a colptr that does not belong to this view: nothing is read)
        if (lane == 0) out[j] = (double)NAN;
        return;
    }
    if (n <= KZ_SL_CHUNK) {
        const KzSoftminPart pt = kz_sl_chunk<I, CHECK>(col_row, col_val, start, end, off, n_off, eps, lane);
        if (lane == 0) out[j] = CHECK && pt.m == INFINITY && pt.s < 0.0 ? (double)NAN : kz_sl_finish(pt.m, pt.s, eps, shift);
        return;
    }
    const int64_t n_chunks = (n + KZ_SL_CHUNK - 1) / KZ_SL_CHUNK;
    double m = INFINITY;
    for (int64_t c = lane; c < n_chunks; c += 64) m = kz_sl_min(m, part[kz_sl_part_slot(start, c)].m);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) m = kz_sl_min(m, __shfl_xor(m, sh, 64));
    if (CHECK && m == INFINITY) {   // (every part is +inf: a pair in any of them?)
        bool any = false;
        for (int64_t c = lane; c < n_chunks; c += 64) any = any || part[kz_sl_part_slot(start, c)].s >= 0.0;
        if (__ballot(any) == 0ull) {
            if (lane == 0) out[j] = (double)NAN;
            return;
        }
    }
    if (m == INFINITY || m == -INFINITY) {
        if (lane == 0) out[j] = kz_sl_finish(m, 0.0, eps, shift);
        return;
    }
    double s = 0.0;
    for (int64_t c = lane; c < n_chunks; c += 64) s += kz_softmin_rescaled(part[kz_sl_part_slot(start, c)], m, eps);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) out[j] = kz_sl_finish(m, s, eps, shift);
}

// ---- (c) the loop's read-out ---------------------------------------------------------------------------------------------------
// slot[it] = max |a - b| as the bit pattern of the (non-negative) double, NaN differences ignored as kz_max_abs_diff ignores them: a
// maximum of non-negative doubles is the maximum of their bit patterns, taken by an INTEGER atomic -- the result does not depend on
// the order anything runs in.  slot is zeroed before the loop (0.0: none left).
__global__ __launch_bounds__(256) void kz_sl_change_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                                           unsigned long long* __restrict__ slot, const int* __restrict__ stop, int it) {
    if (kz_sl_stopped(stop, it)) return;
    __shared__ double s_m[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double d = fabs(a[i] - b[i]);
        m = d > m ? d : m;   // (a NaN difference compares false: ignored)
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const double t = __shfl_xor(m, sh, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = s_m[w] > m ? s_m[w] : m;
        atomicMax(slot + it, (unsigned long long)__double_as_longlong(m));
    }
}

// one thread behind the change kernel: the column step of iteration `it` moved g by at most tol -> the loop stops at `it`
__global__ void kz_sl_decide_kernel(const unsigned long long* __restrict__ slot, double tol, int* __restrict__ stop, int it) {
    if (*stop != 0) return;
    if (__longlong_as_double((long long)slot[it]) <= tol) *stop = it;
}

int kz_sl_require_eps(const char* who, double eps, double shift) {
    KZ_REQUIRE(eps > 0.0 && eps < INFINITY, "%s: the temperature eps must be finite and > 0, got %g", who, eps);
    KZ_REQUIRE(shift > -INFINITY && shift < INFINITY, "%s: shift must be finite, got %g", who, shift);
    return KZ_OK;
}

// ---- launchers: everything on the context's stream, nothing waits ----------------------------------------------------------------
void kz_sl_rows_launch(kz_ctx* ctx, const double* dist, const int64_t* ind, int n_q, int k, int64_t n_index, double eps, const double* off, double shift,
                       double* out, const int* stop, int it) {
    if (k <= 64) {
        int G = 1;
        while (G < k) G <<= 1;
        const int rows = 256 / G;
        hipLaunchKernelGGL(kz_sl_rows_group_kernel, dim3((unsigned)((n_q + rows - 1) / rows)), dim3(256), 0, ctx->stream, dist, ind, n_q, k, G, n_index,
                           eps, off, shift, out, stop, it);
    } else {
        hipLaunchKernelGGL(kz_sl_rows_wave_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, ctx->stream, dist, ind, n_q, k, n_index, eps, off,
                           shift, out, stop, it);
    }
}

// capacity: the places the view may hold (>= nnz); part: 2 ceil(capacity / KZ_SL_CHUNK) parts
int64_t kz_sl_part_count(int64_t capacity) { return 2 * ((capacity + KZ_SL_CHUNK - 1) / KZ_SL_CHUNK); }

// <int, false>: the columns of a transposed view (n_off unused).  <int64_t, true>: the ROWS of a CSR -- colptr = indptr, n_index = its
// row count, col_row = ind, n_off = the number of target rows.
template <typename I, bool CHECK>
void kz_sl_cols_launch(kz_ctx* ctx, const int64_t* colptr, const I* col_row, const double* col_val, int64_t n_index, int64_t capacity, double eps,
                       const double* off, int64_t n_off, double shift, KzSoftminPart* part, double* out, const int* stop, int it) {
    const int64_t n_blocks = (capacity + KZ_SL_CHUNK - 1) / KZ_SL_CHUNK;
    if (n_blocks > 0)   // (two waves per block of places, four waves per workgroup)
        hipLaunchKernelGGL((kz_sl_cols_chunk_kernel<I, CHECK>), dim3((unsigned)((2 * n_blocks + 3) / 4)), dim3(256), 0, ctx->stream, colptr, col_row,
                           col_val, n_index, capacity, eps, off, n_off, part, stop, it);
    hipLaunchKernelGGL((kz_sl_cols_kernel<I, CHECK>), dim3((unsigned)((n_index + 3) / 4)), dim3(256), 0, ctx->stream, colptr, col_row, col_val, n_index,
                       capacity, eps, off, n_off, shift, part, out, stop, it);
}

// the whole transposition, queued: keys, the stable sort, the gather, colptr.  d_indptr NULL: the [n_q, k] lists; else a CSR of
// nnz > 0 entries (k unused), its flat position p the secondary key as i k + c is here.
int kz_sl_transpose(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, int64_t* d_colptr, int* d_col_row,
                    double* d_col_val, const int64_t* d_indptr = nullptr, int64_t nnz = 0) {
    const int total = (int)(d_indptr ? nnz : n_q * k);
    // (released when the function returns, stream-ordered behind the kernels that read them)
    KzPoolBuf<int> key_in, val_in, key_out, val_out;
    int rc = key_in.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = val_in.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = key_out.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = val_out.alloc(ctx, (size_t)total * 4);
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_sl_keys_kernel, dim3(kz_blocks(total, 4096)), dim3(256), 0, ctx->stream, d_ind, total, n_index, key_in.get(), val_in.get());
    KZ_HIP(hipGetLastError());
    // (the sort moves the keys as bit patterns: non-negative ints come back as they went in, ordered as integers)
    rc = kz_sort_pairs_f32_i32(ctx, reinterpret_cast<const float*>(key_in.get()), reinterpret_cast<float*>(key_out.get()), val_in.get(),
                               val_out.get(), total, 0);
    if (rc != KZ_OK) return rc;
    if (d_indptr)
        hipLaunchKernelGGL(kz_sl_gather_csr_kernel, dim3(kz_blocks(total, 4096)), dim3(256), 0, ctx->stream, (const int*)key_out.get(),
                           (const int*)val_out.get(), total, d_indptr, n_q, n_index, d_dist, d_col_row, d_col_val);
    else
        hipLaunchKernelGGL(kz_sl_gather_kernel, dim3(kz_blocks(total, 4096)), dim3(256), 0, ctx->stream, (const int*)key_out.get(), (const int*)val_out.get(),
                           total, k, n_index, d_dist, d_col_row, d_col_val);
    hipLaunchKernelGGL(kz_sl_colptr_kernel, dim3(kz_blocks(n_index + 1, 4096)), dim3(256), 0, ctx->stream, (const int*)key_out.get(), total, n_index,
                       d_colptr);
    KZ_HIP(hipGetLastError());
    return KZ_OK;
}

// The tail kz_lists_transpose and kz_csr_transpose share.  No entry: every column is empty.  Else `transpose()` checks the arrays
// and queues the view, and its entry count is read back where the caller asks for it.
template <typename Transpose>
int kz_sl_transpose_finish(kz_ctx* ctx, bool no_entry, int64_t n_index, int64_t* d_colptr, int64_t* h_nnz, Transpose&& transpose) {
    if (no_entry) {
        KZ_HIP(hipMemsetAsync(d_colptr, 0, (size_t)(n_index + 1) * 8, ctx->stream));
        if (h_nnz) KZ_HIP(hipStreamSynchronize(ctx->stream));
        return KZ_OK;
    }
    const int rc = transpose();
    if (rc != KZ_OK) return rc;
    if (h_nnz) {
        KZ_HIP(hipMemcpyAsync(h_nnz, d_colptr + n_index, 8, hipMemcpyDeviceToHost, ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
    }
    return KZ_OK;
}

// the option checks kz_sinkhorn_lists and kz_sinkhorn_csr share
int kz_sl_require_loop(const char* who, double eps, int n_iter, double tol) {
    KZ_REQUIRE(eps > 0.0 && eps < INFINITY, "%s: the temperature eps must be finite and > 0, got %g", who, eps);
    KZ_REQUIRE(n_iter >= 1, "%s: n_iter must be >= 1, got %d", who, n_iter);
    KZ_REQUIRE(tol == tol, "%s: tol is NaN (negative: no tolerance)", who);
    return KZ_OK;
}

// THE LOOP of kz_sinkhorn_lists and kz_sinkhorn_csr (Sinkhorn._potentials: from f = 0 -- no offset in the first column step --, the
// column step with the constant, the row step), the read-out and the copy of g.  The two layouts differ in three things:
//   capacity / room   the places the column-major view may hold (n_q k, or nnz) and the entries its arrays get (a CSR's may be none);
//   transpose         (colptr, col_row, col_val) -> queues the view;
//   row_step          (g, part, stop, it) -> queues the row step into d_f -- kz_sl_rows_launch for the lists, the chunk tree
//                     kz_sl_cols_launch<int64_t, true> over indptr for a CSR, which shares the parts with the column step (they follow
//                     each other on the stream).
template <typename Transpose, typename RowStep>
int kz_sl_sinkhorn_run(kz_ctx* ctx, int64_t n_q, int64_t n_index, int64_t capacity, int64_t room, double eps, int n_iter, double tol,
                       Transpose&& transpose, RowStep&& row_step, double* d_f, double* d_g, int* h_n_iter, double* h_change, int* h_measured) {
    const bool with_tol = tol >= 0.0;
    // (released when the function returns, behind its last synchronise: the view lives for the call, g is double-buffered)
    KzPoolBuf<int64_t> colptr;
    KzPoolBuf<int> col_row, stop;
    KzPoolBuf<double> col_val, g2;
    KzPoolBuf<KzSoftminPart> part;
    KzPoolBuf<unsigned long long> slot;
    int rc = colptr.alloc(ctx, (size_t)(n_index + 1) * 8);
    if (rc == KZ_OK) rc = col_row.alloc(ctx, (size_t)room * 4);
    if (rc == KZ_OK) rc = col_val.alloc(ctx, (size_t)room * 8);
    if (rc == KZ_OK) rc = g2.alloc(ctx, (size_t)n_index * 2 * 8);
    if (rc == KZ_OK) rc = part.alloc(ctx, (size_t)(kz_sl_part_count(capacity) + 1) * sizeof(KzSoftminPart));
    if (rc == KZ_OK) rc = slot.alloc(ctx, (size_t)(n_iter + 1) * 8);
    if (rc == KZ_OK) rc = stop.alloc(ctx, 16);
    if (rc != KZ_OK) return rc;
    rc = transpose(colptr.get(), col_row.get(), col_val.get());
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemsetAsync(slot.get(), 0, (size_t)(n_iter + 1) * 8, ctx->stream));
    KZ_HIP(hipMemsetAsync(stop.get(), 0, 16, ctx->stream));
    const double shift = eps * log((double)n_q / (double)n_index);
    double* g_buf[2] = {g2.get(), g2.get() + n_index};
    for (int it = 1; it <= n_iter; ++it) {
        double* g_new = g_buf[it & 1];
        kz_sl_cols_launch<int, false>(ctx, colptr.get(), col_row.get(), col_val.get(), n_index, capacity, eps, it == 1 ? nullptr : d_f, 0, shift,
                                      part.get(), g_new, stop.get(), it);
        if (it >= 2) {
            hipLaunchKernelGGL(kz_sl_change_kernel, dim3(kz_blocks(n_index, 4096)), dim3(256), 0, ctx->stream, (const double*)g_new,
                               (const double*)g_buf[(it - 1) & 1], n_index, slot.get(), (const int*)stop.get(), it);
            if (with_tol) hipLaunchKernelGGL(kz_sl_decide_kernel, dim3(1), dim3(1), 0, ctx->stream, (const unsigned long long*)slot.get(), tol, stop.get(), it);
        }
        row_step((const double*)g_new, part.get(), (const int*)stop.get(), it);
    }
    KZ_HIP(hipGetLastError());
    // the one read behind the loop: where it stopped and every iteration's change; then g of that iteration
    int h_stop[4] = {0, 0, 0, 0};
    std::unique_ptr<unsigned long long[]> h_slot(new unsigned long long[n_iter + 1]);
    KZ_HIP(hipMemcpyAsync(h_stop, stop.get(), 16, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipMemcpyAsync(h_slot.get(), slot.get(), (size_t)(n_iter + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    const int done = h_stop[0] != 0 ? h_stop[0] : n_iter;
    KZ_HIP(hipMemcpyAsync(d_g, g_buf[done & 1], (size_t)n_index * 8, hipMemcpyDeviceToDevice, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (h_n_iter) *h_n_iter = done;
    if (done >= 2) {
        if (h_change) memcpy(h_change, &h_slot[done], 8);
        if (h_measured) *h_measured = 1;
    }
    return KZ_OK;
}

}  // namespace

extern "C" int kz_lists_transpose(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, int64_t* d_colptr,
                                  int32_t* d_col_row, double* d_col_val, int64_t* h_nnz) {
    const int rcq = kz_sl_require("kz_lists_transpose", ctx, n_q, k, n_index);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(d_colptr != nullptr, "kz_lists_transpose: null colptr");
    if (h_nnz) *h_nnz = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_sl_transpose_finish(ctx, n_q == 0, n_index, d_colptr, h_nnz, [&]() -> int {
        KZ_REQUIRE(d_dist && d_ind && d_col_row && d_col_val, "kz_lists_transpose: null argument");
        return kz_sl_transpose(ctx, d_dist, d_ind, n_q, k, n_index, d_colptr, d_col_row, d_col_val);
    });
}

extern "C" int kz_softmin_list_rows(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, double eps,
                                    const double* d_off, double shift, double* d_out) {
    int rc = kz_sl_require("kz_softmin_list_rows", ctx, n_q, k, n_index);
    if (rc == KZ_OK) rc = kz_sl_require_eps("kz_softmin_list_rows", eps, shift);
    if (rc != KZ_OK) return rc;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_dist && d_ind && d_out, "kz_softmin_list_rows: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    kz_sl_rows_launch(ctx, d_dist, d_ind, (int)n_q, k, n_index, eps, d_off, shift, d_out, nullptr, 0);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

extern "C" int kz_softmin_list_cols(kz_ctx* ctx, const int64_t* d_colptr, const int32_t* d_col_row, const double* d_col_val, int64_t n_index,
                                    int64_t nnz, double eps, const double* d_off, double shift, double* d_out) {
    KZ_REQUIRE(ctx != nullptr, "kz_softmin_list_cols: null context");
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_softmin_list_cols: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    KZ_REQUIRE(nnz >= 0 && nnz < 0x7fffffffLL, "kz_softmin_list_cols: nnz = %lld entries, the limit is 2^31 - 2", (long long)nnz);
    const int rce = kz_sl_require_eps("kz_softmin_list_cols", eps, shift);
    if (rce != KZ_OK) return rce;
    KZ_REQUIRE(d_colptr && d_out && (nnz == 0 || (d_col_row && d_col_val)), "kz_softmin_list_cols: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    KzPoolBuf<KzSoftminPart> part;   // (released when the function returns, behind its synchronise)
    const int rc = part.alloc(ctx, (size_t)(kz_sl_part_count(nnz) + 1) * sizeof(KzSoftminPart));
    if (rc != KZ_OK) return rc;
    kz_sl_cols_launch<int, false>(ctx, d_colptr, d_col_row, d_col_val, n_index, nnz, eps, d_off, 0, shift, part.get(), d_out, nullptr, 0);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

extern "C" int kz_sinkhorn_lists(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, double eps, int n_iter,
                                 double tol, double* d_f, double* d_g, int* h_n_iter, double* h_change, int* h_measured) {
    const int rcq = kz_sl_require("kz_sinkhorn_lists", ctx, n_q, k, n_index);
    if (rcq != KZ_OK) return rcq;
    const int rcl = kz_sl_require_loop("kz_sinkhorn_lists", eps, n_iter, tol);
    if (rcl != KZ_OK) return rcl;
    if (h_n_iter) *h_n_iter = 0;
    if (h_change) *h_change = 0.0;
    if (h_measured) *h_measured = 0;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_dist && d_ind && d_f && d_g, "kz_sinkhorn_lists: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_sl_sinkhorn_run(
        ctx, n_q, n_index, n_q * k, n_q * k, eps, n_iter, tol,
        [&](int64_t* colptr, int* col_row, double* col_val) { return kz_sl_transpose(ctx, d_dist, d_ind, n_q, k, n_index, colptr, col_row, col_val); },
        [&](const double* g, KzSoftminPart*, const int* stop, int it) {
            kz_sl_rows_launch(ctx, d_dist, d_ind, (int)n_q, k, n_index, eps, g, 0.0, d_f, stop, it);
        },
        d_f, d_g, h_n_iter, h_change, h_measured);
}

// ---- the CSR layout (include/kiez_amd.h: "the same three steps on RAGGED (CSR) pair lists") ------------------------------------

extern "C" int kz_csr_transpose(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                                int64_t n_index, int64_t* d_colptr, int32_t* d_col_row, double* d_col_val, int64_t* h_nnz) {
    const int rcq = kz_csr_require("kz_csr_transpose", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(d_colptr != nullptr, "kz_csr_transpose: null colptr");
    if (h_nnz) *h_nnz = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    if (n_q > 0) {
        const int rcv = kz_csr_validate("kz_csr_transpose", ctx, d_indptr, n_q, nnz);
        if (rcv != KZ_OK) return rcv;
    }
    return kz_sl_transpose_finish(ctx, n_q == 0 || nnz == 0, n_index, d_colptr, h_nnz, [&]() -> int {
        KZ_REQUIRE(d_dist && d_ind && d_col_row && d_col_val, "kz_csr_transpose: null argument");
        return kz_sl_transpose(ctx, d_dist, d_ind, n_q, 0, n_index, d_colptr, d_col_row, d_col_val, d_indptr, nnz);
    });
}

extern "C" int kz_softmin_csr_rows(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                                   int64_t n_index, double eps, const double* d_off, double shift, double* d_out) {
    int rc = kz_csr_require("kz_softmin_csr_rows", ctx, n_q, nnz, n_index);
    if (rc == KZ_OK) rc = kz_sl_require_eps("kz_softmin_csr_rows", eps, shift);
    if (rc != KZ_OK) return rc;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_out && (nnz == 0 || (d_dist && d_ind)), "kz_softmin_csr_rows: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    rc = kz_csr_validate("kz_softmin_csr_rows", ctx, d_indptr, n_q, nnz);
    if (rc != KZ_OK) return rc;
    KzPoolBuf<KzSoftminPart> part;   // (released when the function returns, behind its synchronise)
    rc = part.alloc(ctx, (size_t)(kz_sl_part_count(nnz) + 1) * sizeof(KzSoftminPart));
    if (rc != KZ_OK) return rc;
    kz_sl_cols_launch<int64_t, true>(ctx, d_indptr, d_ind, d_dist, n_q, nnz, eps, d_off, n_index, shift, part.get(), d_out, nullptr, 0);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

extern "C" int kz_sinkhorn_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                               int64_t n_index, double eps, int n_iter, double tol, double* d_f, double* d_g, int* h_n_iter, double* h_change,
                               int* h_measured) {
    const int rcq = kz_csr_require("kz_sinkhorn_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    const int rcl = kz_sl_require_loop("kz_sinkhorn_csr", eps, n_iter, tol);
    if (rcl != KZ_OK) return rcl;
    if (h_n_iter) *h_n_iter = 0;
    if (h_change) *h_change = 0.0;
    if (h_measured) *h_measured = 0;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_f && d_g && (nnz == 0 || (d_dist && d_ind)), "kz_sinkhorn_csr: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_sinkhorn_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    return kz_sl_sinkhorn_run(
        ctx, n_q, n_index, nnz, nnz + 1, eps, n_iter, tol,
        [&](int64_t* colptr, int* col_row, double* col_val) -> int {
            if (nnz > 0) return kz_sl_transpose(ctx, d_dist, d_ind, n_q, 0, n_index, colptr, col_row, col_val, d_indptr, nnz);
            KZ_HIP(hipMemsetAsync(colptr, 0, (size_t)(n_index + 1) * 8, ctx->stream));   // (no entry: every column is empty)
            return KZ_OK;
        },
        [&](const double* g, KzSoftminPart* part, const int* stop, int it) {
            kz_sl_cols_launch<int64_t, true>(ctx, d_indptr, d_ind, d_dist, n_q, nnz, eps, g, n_index, 0.0, part, d_f, stop, it);
        },
        d_f, d_g, h_n_iter, h_change, h_measured);
}
