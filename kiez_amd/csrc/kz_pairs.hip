// NEIGHBOUR PAIRS OF BOTH DIRECTIONS AS A CSR: the producer in front of kz_match_csr, kz_assign_csr and
// kz_sinkhorn_csr.  Two steps live here:
//   kz_lists_combine     the SET step: forward lists fwd [n_q, k_f] (target ids per source row) and reverse lists rev [n_index, k_r]
//                        (source ids per target row) -> the pairs (source row, target row) of F, R, F u R or F n R as a CSR over the
//                        source rows, every pair once, a row ascending by target id;
//   kz_pairs_raw_values  the exact ranking value of every entry of a CSR (what kz_pair_values gives the entries of [n_q, k] lists):
//                        the first half of kz_pairs_values, whose conversions and row sort live in kz_knn.hip's translation unit
//                        (kz_pairs.h), beside the kernels they share with kz_radius_neighbors.
//
// THE SET STEP IS A SORT, NOT A ROW WALK.  Every entry of the lists the mode reads is one (source row, target row, side) triple at
// flat position p -- forward entries first, p = i k_f + c, then the reverse entries, p = n_q k_f + j k_r + c.  Two passes of the
// library's STABLE radix sort (kz_sort.hip) order the positions by (source row, target row): first by target row, then by source row.
// An entry that is no pair -- a target id outside [0, n_index) in a forward list, a source id outside [0, n_q) in a reverse list:
// kz_match_lists' rule, so -1, kz_knn_reduced's INT_MAX padding and ids >= n are covered -- gets the key behind every row in both
// passes and ends in the tail.  In the sorted order the entries of one pair are a RUN: its first entry, the HEAD, walks the run (at
// most k_f + k_r entries: a row lists a target at most k_f times, a target lists a source at most k_r times), sees which sides hold
// the pair and keeps it or not by the mode.  The output place of a kept head is the exclusive prefix sum of the keep flags
// (tile counts, one workgroup over the tile totals, the tile again), indptr[i] is that prefix at the first entry of row i (a binary
// search in the sorted row keys), and the fill writes the target id of every kept head of a row that ends within `capacity`.
// Why not a lane or a wave per row: a hub source is listed by every target, so rows of the reverse side have any length while most
// are short; one thread per ENTRY has no row length in it -- no long-row hand-over, no LDS, no loop but the run walk and the
// binary searches.  Integer keys, counts and scans only; no atomics on any output; nothing depends on the order workgroups run in:
// two calls give identical bytes.
#include "kz_common.h"
#include "kz_bool.h"
#include "kz_pool_buf.h"
#include "kz_precomputed.h"
#include "kz_rows.h"

namespace {

// ---- (a) the set step -----------------------------------------------------------------------------------------------------------
struct KzCombineLists {
    const int64_t* __restrict__ fwd;   // [n_q, k_f] or unused (n_f == 0)
    const int64_t* __restrict__ rev;   // [n_index, k_r] or unused (total == n_f)
    int n_f;                           // forward entries in front of the reverse entries: n_q k_f, or 0 when the mode reads none
    int total;                         // all entries (< 2^31 - 1)
    int k_f, k_r;
    int64_t n_q, n_index;
};

// (source row, target row) of the entry at flat position p; false: no pair
__device__ __forceinline__ bool kz_pc_entry(const KzCombineLists& in, int p, int64_t& row, int64_t& tgt) {
    if (p < in.n_f) {
        row = p / in.k_f;
        tgt = in.fwd[p];
    } else {
        const int r = p - in.n_f;
        tgt = r / in.k_r;
        row = in.rev[r];
    }
    return row >= 0 && row < in.n_q && tgt >= 0 && tgt < in.n_index;
}

// pass 1: key = the target row (n_index: no pair), value = the flat position
__global__ __launch_bounds__(256) void kz_pc_target_keys_kernel(KzCombineLists in, int* __restrict__ key, int* __restrict__ pos) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < in.total; p += stride) {
        int64_t row, tgt;
        key[p] = (int)(kz_pc_entry(in, (int)p, row, tgt) ? tgt : in.n_index);
        pos[p] = (int)p;
    }
}

// pass 2: key = the source row (n_q: no pair) of the position pass 1 put at place p
__global__ __launch_bounds__(256) void kz_pc_row_keys_kernel(KzCombineLists in, const int* __restrict__ pos, int* __restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < in.total; p += stride) {
        int64_t row, tgt;
        key[p] = (int)(kz_pc_entry(in, pos[p], row, tgt) ? row : in.n_q);
    }
}

// behind pass 2: the target row of every place in front of the tail (the tail's places are never read: their row key is n_q)
__global__ __launch_bounds__(256) void kz_pc_targets_kernel(KzCombineLists in, const int* __restrict__ row_key, const int* __restrict__ pos,
                                                            int* __restrict__ tgt_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < in.total; p += stride) {
        if (row_key[p] >= in.n_q) continue;
        int64_t row, tgt;
        (void)kz_pc_entry(in, pos[p], row, tgt);
        tgt_out[p] = (int)tgt;
    }
}

// keep[p] = 1 for the head of a run that the mode keeps, else 0.  The walk ends at the first place of another pair, at the tail or
// at `total`: at most k_f + k_r steps.
__global__ __launch_bounds__(256) void kz_pc_keep_kernel(KzCombineLists in, int mode, const int* __restrict__ row_key, const int* __restrict__ tgt,
                                                         const int* __restrict__ pos, int* __restrict__ keep) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < in.total; p += stride) {
        const int r = row_key[p];
        int k = 0;
        if (r < in.n_q) {
            const int t = tgt[p];
            const bool head = p == 0 || row_key[p - 1] != r || tgt[p - 1] != t;
            if (head) {
                bool in_f = false, in_r = false;
                for (int64_t q = p; q < in.total && row_key[q] == r && tgt[q] == t; ++q) {
                    if (pos[q] < in.n_f)
                        in_f = true;
                    else
                        in_r = true;
                }
                k = mode == KZ_PAIRS_MUTUAL ? (in_f && in_r) : mode == KZ_PAIRS_FORWARD ? in_f : mode == KZ_PAIRS_REVERSE ? in_r : 1;
            }
        }
        keep[p] = k;
    }
}

// The exclusive prefix of v over the workgroup's 256 threads and their total, to every thread (a shuffle scan per wave, the four
// wave totals through LDS; s_w is free again when the call returns).  (kz_radius_tile_scan's scheme: that header is part of
// kz_knn.hip's translation unit -- it defines kernels -- and cannot be included here.)
__device__ __forceinline__ int kz_pc_tile_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return before + incl - v;
}

// scan, level 1: tile_sum[t] = the kept heads among places 256 t .. 256 t + 255
__global__ __launch_bounds__(256) void kz_pc_tile_sums_kernel(const int* __restrict__ keep, int total, int* __restrict__ tile_sum) {
    __shared__ int s_w[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int sum;
    (void)kz_pc_tile_scan(p < total ? keep[p] : 0, s_w, sum);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;
}

// scan, level 2 (ONE workgroup): tile_sum[t] <- the kept heads in front of tile t, 256 tiles a round with a running base;
// place[total] = the number of pairs
__global__ __launch_bounds__(256) void kz_pc_tile_bases_kernel(int* __restrict__ tile_sum, int n_tiles, int total, int* __restrict__ place) {
    __shared__ int s_w[4];
    int base = 0;   // (uniform)
    for (int t0 = 0; t0 < n_tiles; t0 += 256) {   // (uniform)
        const int t = t0 + (int)threadIdx.x;
        int sum;
        const int before = kz_pc_tile_scan(t < n_tiles ? tile_sum[t] : 0, s_w, sum);
        if (t < n_tiles) tile_sum[t] = base + before;
        base += sum;
    }
    if (threadIdx.x == 0) place[total] = base;
}

// scan, level 3: place[p] = the kept heads in front of place p
__global__ __launch_bounds__(256) void kz_pc_places_kernel(const int* __restrict__ keep, int total, const int* __restrict__ tile_base,
                                                           int* __restrict__ place) {
    __shared__ int s_w[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int sum;
    const int before = kz_pc_tile_scan(p < total ? keep[p] : 0, s_w, sum);
    if (p < total) place[p] = tile_base[blockIdx.x] + before;
}

// indptr[i] = place[the first place whose row key is >= i], i = 0 .. n_q (the tail's key is n_q: indptr[n_q] = the number of pairs)
__global__ __launch_bounds__(256) void kz_pc_indptr_kernel(const int* __restrict__ row_key, int total, int64_t n_q, const int* __restrict__ place,
                                                           int64_t* __restrict__ indptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_q; i += stride) {
        int lo = 0, hi = total;   // (the answer lies in [lo, hi])
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (row_key[mid] < i)
                lo = mid + 1;
            else
                hi = mid;
        }
        indptr[i] = place[lo];
    }
}

// the fill: the target id of every kept head whose row ends within `capacity`, at its place (< indptr[row + 1] <= capacity)
__global__ __launch_bounds__(256) void kz_pc_fill_kernel(const int* __restrict__ row_key, const int* __restrict__ tgt, const int* __restrict__ keep,
                                                         const int* __restrict__ place, int total, const int64_t* __restrict__ indptr,
                                                         int64_t capacity, int64_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        if (!keep[p]) continue;
        if (indptr[row_key[p] + 1] > capacity) continue;
        out[place[p]] = tgt[p];
    }
}

// ---- (b) the exact ranking value of every entry of a CSR ------------------------------------------------------------------------
// kz_pair_values_kernel's arithmetic with the query row of an entry taken from indptr.  An entry whose id is no index row: +inf.
// One WAVE per entry (euclidean, sqeuclidean, cosine: the canonical dot product of kz_exact_value, every element type)
template <typename T>
__global__ __launch_bounds__(256) void kz_pairs_wave_kernel(const T* __restrict__ qraw, const double* __restrict__ qsqn, const T* __restrict__ yraw,
                                                            const double* __restrict__ ysqn, int64_t n_i, int d, int metric, double p,
                                                            const int64_t* __restrict__ indptr, const int64_t* __restrict__ ind, int64_t n_q,
                                                            int64_t nnz, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (wave-uniform)
    if (e >= nnz) return;
    const int64_t row = kz_csr_row_of(indptr, n_q, e);
    const int64_t yi = ind[e];
    double v = INFINITY;
    if (yi >= 0 && yi < n_i) v = kz_exact_value<T>(qraw + row * (int64_t)d, yraw + yi * (int64_t)d, qsqn[row], ysqn[yi], d, metric, lane, p);
    if (lane == 0) out[e] = v;
}

// One LANE per entry: the Minkowski family, terms in feature order (kz_family_value_seq: the order of the tiled distance kernel)
template <typename T>
__global__ __launch_bounds__(256) void kz_pairs_family_kernel(const T* __restrict__ qraw, const T* __restrict__ yraw, int64_t n_i, int d, int metric,
                                                              double p, const double* __restrict__ V, const double* __restrict__ qcorr,
                                                              const double* __restrict__ ycorr, const int64_t* __restrict__ indptr,
                                                              const int64_t* __restrict__ ind, int64_t n_q, int64_t nnz, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t row = kz_csr_row_of(indptr, n_q, e);
        const int64_t yi = ind[e];
        const bool ok = yi >= 0 && yi < n_i;
        const kz_family_pair_args ex = {V, qcorr ? qcorr + 2 * row : nullptr, ycorr && ok ? ycorr + 2 * yi : nullptr};
        out[e] = ok ? kz_family_value_seq<T>(qraw + row * (int64_t)d, yraw + yi * (int64_t)d, d, metric, p, ex) : INFINITY;
    }
}

// One lane per entry: the boolean metrics over the packed rows (kz_bool_pair_values_kernel's integers and finish)
__global__ __launch_bounds__(256) void kz_pairs_bool_kernel(const uint32_t* __restrict__ qbits, const int32_t* __restrict__ qcnt,
                                                            const uint32_t* __restrict__ ybits, const int32_t* __restrict__ ycnt, int64_t n_i, int W,
                                                            int d, int metric, int self_zero, const int64_t* __restrict__ indptr,
                                                            const int64_t* __restrict__ ind, int64_t n_q, int64_t nnz, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t row = kz_csr_row_of(indptr, n_q, e);
        const int64_t yi = ind[e];
        double v = INFINITY;
        if (yi >= 0 && yi < n_i) {
            const uint4* __restrict__ q = reinterpret_cast<const uint4*>(qbits + row * (int64_t)W);
            const uint4* __restrict__ y = reinterpret_cast<const uint4*>(ybits + yi * (int64_t)W);
            int ntt = 0;
            for (int w = 0; w < W / 4; ++w) {
                const uint4 a = q[w], b = y[w];
                ntt += __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w);
            }
            v = (self_zero && yi == row) ? 0.0 : kz_bool_finish(metric, d, qcnt[row], ycnt[yi], ntt);
        }
        out[e] = v;
    }
}

// One lane per entry: a precomputed matrix D [n_rows, n_cols] -- the entry itself, widened.  q_is_cols: the query is the columns view
// (its row `row` is column `row` of D, the index rows are D's rows).
template <typename T>
__global__ __launch_bounds__(256) void kz_pairs_precomputed_kernel(const T* __restrict__ D, int64_t n_cols, int q_is_cols, int64_t n_i,
                                                                   const int64_t* __restrict__ indptr, const int64_t* __restrict__ ind, int64_t n_q,
                                                                   int64_t nnz, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t row = kz_csr_row_of(indptr, n_q, e);
        const int64_t yi = ind[e];
        double v = INFINITY;
        if (yi >= 0 && yi < n_i) v = (double)(q_is_cols ? D[yi * n_cols + row] : D[row * n_cols + yi]);
        out[e] = v;
    }
}

}  // namespace

// d_out[e] = the value kz_knn ranks index row d_ind[e] by for the query row that holds entry e of the CSR, e < nnz (nnz >= 1) -- the
// bits of kz_pair_values; an id outside [0, index.n): +inf.  The caller (kz_pairs_values, kz_pairs.h) has checked the pair of
// matrices (kz_require_pair), n_q <= query.n and d_indptr (kz_csr_validate).  Enqueued on the context's stream.
int kz_pairs_raw_values(kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index, const int64_t* d_indptr, const int64_t* d_ind, int64_t n_q,
                        int64_t nnz, double* d_out) {
    const int metric = index->metric;
    const dim3 lanes(kz_blocks(nnz, 4096));
    if (metric == KZ_PRECOMPUTED) {
        const kz_precomputed* p = query->pre;
        if (p->dtype == KZ_F32)
            hipLaunchKernelGGL(kz_pairs_precomputed_kernel<float>, lanes, dim3(256), 0, ctx->stream, (const float*)p->values, p->n_cols,
                               query->pre_cols ? 1 : 0, index->n, d_indptr, d_ind, n_q, nnz, d_out);
        else
            hipLaunchKernelGGL(kz_pairs_precomputed_kernel<double>, lanes, dim3(256), 0, ctx->stream, (const double*)p->values, p->n_cols,
                               query->pre_cols ? 1 : 0, index->n, d_indptr, d_ind, n_q, nnz, d_out);
    } else if (kz_is_bool_metric(metric)) {
        hipLaunchKernelGGL(kz_pairs_bool_kernel, lanes, dim3(256), 0, ctx->stream, (const uint32_t*)query->bits, (const int32_t*)query->bits_cnt,
                           (const uint32_t*)index->bits, (const int32_t*)index->bits_cnt, index->n, index->bits_words, (int)query->d, metric,
                           kz_bool_self_zero(query, index) ? 1 : 0, d_indptr, d_ind, n_q, nnz, d_out);
    } else {
        const int rc = kz_dispatch_rows(query->dtype, "kz_pairs_values", [&](auto e) {
            using T = typename decltype(e)::type;
            if (metric >= KZ_MANHATTAN) {
                if constexpr (kz_half_rows<T>) {   // (kz_matrix_create refuses the pair: 2-byte rows exist for metrics 0 .. 2 only)
                    kz_set_error("kz_pairs_values: metric %d is not supported for %s rows", metric, kz_dtype_name(index->dtype));
                    return (int)KZ_ERR_UNSUPPORTED;
                } else {
                    hipLaunchKernelGGL(kz_pairs_family_kernel<T>, lanes, dim3(256), 0, ctx->stream, (const T*)query->raw, (const T*)index->raw, index->n,
                                       (int)query->d, metric, query->mink_p, index->seu_v, query->corr, index->corr, d_indptr, d_ind, n_q, nnz, d_out);
                    return (int)KZ_OK;
                }
            }
            hipLaunchKernelGGL(kz_pairs_wave_kernel<T>, dim3((unsigned)((nnz + 3) / 4)), dim3(256), 0, ctx->stream, (const T*)query->raw, query->sqn,
                               (const T*)index->raw, index->sqn, index->n, (int)query->d, metric, query->mink_p, d_indptr, d_ind, n_q, nnz, d_out);
            return (int)KZ_OK;
        });
        if (rc != KZ_OK) return rc;
    }
    KZ_HIP(hipGetLastError());
    return KZ_OK;
}

// THE FLAG SCAN (kz_rows.h): the three launches above on the context's stream, total >= 1.  Shared with kz_forest.hip's compaction.
void kz_scan_flags(kz_ctx* ctx, const int* d_keep, int total, int* d_tile, int* d_place) {
    const int n_tiles = (total + 255) / 256;
    const dim3 wg(256);
    hipLaunchKernelGGL(kz_pc_tile_sums_kernel, dim3(n_tiles), wg, 0, ctx->stream, d_keep, total, d_tile);
    hipLaunchKernelGGL(kz_pc_tile_bases_kernel, dim3(1), wg, 0, ctx->stream, d_tile, n_tiles, total, d_place);
    hipLaunchKernelGGL(kz_pc_places_kernel, dim3(n_tiles), wg, 0, ctx->stream, d_keep, total, (const int*)d_tile, d_place);
}

extern "C" int kz_lists_combine(kz_ctx* ctx, const int64_t* d_fwd_ind, int64_t n_q, int k_f, const int64_t* d_rev_ind, int64_t n_index, int k_r,
                                int mode, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, int64_t* h_total) {
    KZ_REQUIRE(ctx && d_indptr && h_total, "kz_lists_combine: null argument");
    KZ_REQUIRE(mode >= KZ_PAIRS_FORWARD && mode <= KZ_PAIRS_MUTUAL, "kz_lists_combine: unknown mode %d (KZ_PAIRS_FORWARD .. KZ_PAIRS_MUTUAL)", mode);
    KZ_REQUIRE(k_f >= 1 && k_f <= KZ_MAX_CANDIDATES && k_r >= 1 && k_r <= KZ_MAX_CANDIDATES,
               "kz_lists_combine: lists of 1 .. %d columns, got k_f = %d, k_r = %d", KZ_MAX_CANDIDATES, k_f, k_r);
    KZ_REQUIRE(n_q >= 0 && n_q < 0x7fffffffLL, "kz_lists_combine: n_q = %lld is outside [0, 2^31 - 1)", (long long)n_q);
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_lists_combine: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    KZ_REQUIRE(capacity >= 0, "kz_lists_combine: capacity %lld is negative", (long long)capacity);
    KZ_REQUIRE(capacity == 0 || d_ind, "kz_lists_combine: d_ind is required for capacity > 0");
    const bool use_f = mode != KZ_PAIRS_REVERSE, use_r = mode != KZ_PAIRS_FORWARD;
    KZ_REQUIRE(n_q == 0 || ((!use_f || d_fwd_ind) && (!use_r || d_rev_ind)), "kz_lists_combine: the mode reads a list array that is null");
    const int64_t n_f = use_f ? n_q * (int64_t)k_f : 0, total64 = n_f + (use_r ? n_index * (int64_t)k_r : 0);
    if (total64 >= 0x7fffffffLL) {   // (the result is a subset of the entries read: its total is below the limit when they are)
        kz_set_error("kz_lists_combine: %lld list entries, the limit is 2^31 - 2", (long long)total64);
        return KZ_ERR_UNSUPPORTED;
    }
    *h_total = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    if (n_q == 0) {
        KZ_HIP(hipMemsetAsync(d_indptr, 0, sizeof(int64_t), ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        return KZ_OK;
    }
    const int total = (int)total64, n_tiles = (total + 255) / 256;
    const KzCombineLists in{d_fwd_ind, d_rev_ind, (int)n_f, total, k_f, k_r, n_q, n_index};
    // (released when the function returns, stream-ordered behind the kernels that read them)
    KzPoolBuf<int> a, b, c, d, place, tile;
    int rc = a.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = b.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = c.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = d.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = place.alloc(ctx, ((size_t)total + 1) * 4);
    if (rc == KZ_OK) rc = tile.alloc(ctx, (size_t)n_tiles * 4);
    if (rc != KZ_OK) return rc;
    const dim3 grid(kz_blocks(total, 4096)), wg(256);
    // by target row: a = keys, b = positions -> c, d   (the sort moves the keys as bit patterns: non-negative ints come back as they
    // went in, ordered as integers)
    hipLaunchKernelGGL(kz_pc_target_keys_kernel, grid, wg, 0, ctx->stream, in, a.get(), b.get());
    KZ_HIP(hipGetLastError());
    rc = kz_sort_pairs_f32_i32(ctx, reinterpret_cast<const float*>(a.get()), reinterpret_cast<float*>(c.get()), b.get(), d.get(), total, 0);
    if (rc != KZ_OK) return rc;
    // then, stable, by source row: a = keys of the positions d -> c = row keys, b = positions
    hipLaunchKernelGGL(kz_pc_row_keys_kernel, grid, wg, 0, ctx->stream, in, (const int*)d.get(), a.get());
    KZ_HIP(hipGetLastError());
    rc = kz_sort_pairs_f32_i32(ctx, reinterpret_cast<const float*>(a.get()), reinterpret_cast<float*>(c.get()), d.get(), b.get(), total, 0);
    if (rc != KZ_OK) return rc;
    const int* row_key = c.get();
    const int* pos = b.get();
    int* tgt = a.get();
    int* keep = d.get();
    hipLaunchKernelGGL(kz_pc_targets_kernel, grid, wg, 0, ctx->stream, in, row_key, pos, tgt);
    hipLaunchKernelGGL(kz_pc_keep_kernel, grid, wg, 0, ctx->stream, in, mode, row_key, (const int*)tgt, pos, keep);
    kz_scan_flags(ctx, keep, total, tile.get(), place.get());
    hipLaunchKernelGGL(kz_pc_indptr_kernel, dim3(kz_blocks(n_q + 1, 4096)), wg, 0, ctx->stream, row_key, total, n_q, (const int*)place.get(), d_indptr);
    if (capacity > 0)
        hipLaunchKernelGGL(kz_pc_fill_kernel, grid, wg, 0, ctx->stream, row_key, (const int*)tgt, (const int*)keep, (const int*)place.get(), total,
                           (const int64_t*)d_indptr, capacity, d_ind);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipMemcpyAsync(h_total, d_indptr + n_q, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}
