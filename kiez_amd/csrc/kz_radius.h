// RADIUS NEIGHBOURS (kz_radius_neighbors, kz_radius_neighbors_reduced): every index row within a threshold of every query row, over
// the whole index, as a CSR (indptr, index rows, values) -- the third member of the family of kz_gold_ranks.h (a COUNT in place of
// the exact stage's selection) and kz_knn_reduced.h (a two-level selection): a THRESHOLD in place of the selection.
//
// Rule: pair (i, j) is in the result exactly when w_ij <= radius, w = what the list calls return for the pair -- the plain call:
// kz_output_distance<T> of the exact ranking value (kz_knn's distance); the reduced call: kz_rank_reduce<T, KIND, METRIC> of it
// (kz_knn_reduced's w, the bits the transform kernels write).  A NaN w fails every comparison and is never in the result, also for
// radius = +inf.  The output has a variable length, so a call runs three passes per batch of the exact stage's value matrix
// (kz_exact_walk):
//   1. kz_radius_count_kernel: one workgroup per (chunk of KZ_RADIUS_CHUNK index rows, row of the batch) counts w <= radius in its
//      chunk and writes ONE integer to cnt [nb][n_chunks] -- a plain store, no atomic;
//   2. kz_radius_scan_rows_kernel (one workgroup per row: the exclusive offsets of the row's chunks, the row's total) and
//      kz_radius_scan_batch_kernel (one workgroup: d_indptr of the batch's rows on top of a running base that stays on the device
//      from batch to batch, and the longest row so far);
//   3. kz_radius_fill_kernel: the predicate again, for the chunks with a non-zero count of the rows that end inside `capacity`:
//      (index row, w) at row start + chunk offset + ballot prefix -- index order within a row, no atomics.
// Behind the walk ONE read-back (the total and the longest row), then with `sorted` kz_radius_sort_kernel: one workgroup per row,
// (w, index row) ascending under kz_knnr_key's order -- rows of up to KZ_RADIUS_SORT_LDS entries in LDS, longer rows by a stable
// radix sort through HBM.
// Integer counts, ballots and scans only; no float atomics; no kernel waits for another workgroup; every loop is bounded by the
// row or chunk length.  A row's entries depend on the row's values alone and its place on the counts of the rows before it in the
// call: the result has the same bits however the exact stage cuts the call into batches, and the rows of a row range are the rows of
// the whole call.
#pragma once
#include "kz_order_key.h"   // kz_knnr_key

constexpr int KZ_RADIUS_CHUNK = KZ_RANK_CHUNK;   // values per workgroup of the count and fill kernels: kz_rank_count_kernel's walk
// Rows of up to this many entries are sorted in LDS: 12 bytes per entry (w, index row) = 48 KiB of the CU's 160 KiB, so three
// workgroups of rows share a CU, and a static allocation (below the 64 KiB a kernel gets without asking for more).  A bitonic
// network over the next power of two.  Longer rows -- a row can hold the whole index -- take the radix path.
constexpr int KZ_RADIUS_SORT_LDS = 4096;

// w of a value: the distance kz_knn returns (KZ_RANK_NONE) or its hubness-reduced distance.
template <typename T, int KIND, int METRIC>
__device__ __forceinline__ double kz_radius_w(double v, double p, double qa, double qb, double ta, double tb) {
    if (KIND == KZ_RANK_NONE) return kz_output_distance<T>(v, METRIC, p);
    return kz_rank_reduce<T, KIND, METRIC>(v, p, qa, qb, ta, tb);
}

// The exclusive prefix of v over the workgroup's 256 threads and their total, to every thread: a shuffle scan per wave, the four
// wave totals through LDS (two barriers: s_w is free again when the call returns).
template <typename I>
__device__ __forceinline__ I kz_radius_tile_scan(I v, I* s_w, int lane, int wave, I& total) {
    I incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const I t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    I before = 0;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return before + incl - v;
}

// Pass 1.  vals [nb][n_i]: the value matrix of rows b0 .. b0 + nb of the call (q_a / q_b are indexed by that row).  Workgroup (c, b)
// writes cnt[b n_chunks + c] = #{ j in chunk c : w_bj <= radius }.  The walk is kz_rank_count_kernel's (KzRankChunk): 16-byte value
// loads, eight in flight, the scalar ends; the index-side state at j by 8-byte loads (a value row starts at an even or odd element
// of the matrix: the parity of j is not that of the value's address); the query side uniform.  KZ_RANK_NONE reads no state.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_radius_count_kernel(const double* __restrict__ vals, int64_t n_i, int b0, int n_chunks, double radius,
                                                              double mp, const double* __restrict__ q_a, const double* __restrict__ q_b,
                                                              const double* __restrict__ t_a, const double* __restrict__ t_b,
                                                              int* __restrict__ cnt) {
    constexpr bool ONE = KIND != KZ_RANK_NONE, TWO = KIND == KZ_RANK_MP_NORMAL;   // state vectors per side
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = b0 + blockIdx.y;
    const double qa = ONE ? q_a[row] : 0.0, qb = TWO ? q_b[row] : 0.0;
    const KzRankChunk ch(blockIdx.y, blockIdx.x, KZ_RADIUS_CHUNK, n_i);
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + ch.a);
    int n = 0;   // (wave-uniform: ballots)
    constexpr int U = 8;   // value loads in flight per thread
    for (int p0 = 0; p0 < ch.n_pairs; p0 += 256 * U) {   // (uniform)
        double2 x[U];
        double ta[U][2], tb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const bool in = p < ch.n_pairs;
            const int64_t j = in ? ch.a - ch.e0 + 2 * (int64_t)p : ch.j0;   // (past the pairs: the chunk's first row, read and not used)
            x[u] = in ? pairs[p] : double2{0.0, 0.0};
            ta[u][0] = ONE ? t_a[j] : 0.0;
            ta[u][1] = ONE ? t_a[in ? j + 1 : j] : 0.0;
            tb[u][0] = TWO ? t_b[j] : 0.0;
            tb[u][1] = TWO ? t_b[in ? j + 1 : j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = p0 + 256 * u + tid < ch.n_pairs;
            const double w0 = kz_radius_w<T, KIND, METRIC>(x[u].x, mp, qa, qb, ta[u][0], tb[u][0]);
            const double w1 = kz_radius_w<T, KIND, METRIC>(x[u].y, mp, qa, qb, ta[u][1], tb[u][1]);
            n += __popcll(__ballot(in && w0 <= radius)) + __popcll(__ballot(in && w1 <= radius));   // (NaN <= radius: false)
        }
    }
    if (wave == 0) {   // the chunk's scalar ends: lane 0 the element before the pairs, lane 1 the one behind them
        bool c = false;
        const bool first = lane == 0 && ch.a > ch.e0 + ch.j0, last = lane == 1 && (ch.rem & 1);
        if (first || last) {
            const int64_t j = first ? ch.j0 : ch.j1 - 1;
            c = kz_radius_w<T, KIND, METRIC>(vals[ch.e0 + j], mp, qa, qb, ONE ? t_a[j] : 0.0, TWO ? t_b[j] : 0.0) <= radius;
        }
        n += __popcll(__ballot(c));
    }
    if (lane == 0) s_w[wave] = n;
    __syncthreads();
    if (tid == 0) cnt[(int64_t)blockIdx.y * n_chunks + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Pass 2a.  One workgroup per row b of the batch: off[b][c] = the number of the row's entries in the chunks before c; row_n[b] = the
// row's count (< 2^31: a row holds at most the index).
__global__ __launch_bounds__(256) void kz_radius_scan_rows_kernel(const int* __restrict__ cnt, int n_chunks, int* __restrict__ off,
                                                                  int* __restrict__ row_n) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t at = (int64_t)blockIdx.x * n_chunks;
    int base = 0;   // (uniform)
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {   // (uniform)
        const int c = c0 + tid;
        int total;
        const int before = kz_radius_tile_scan<int>(c < n_chunks ? cnt[at + c] : 0, s_w, lane, wave, total);
        if (c < n_chunks) off[at + c] = base + before;
        base += total;
    }
    if (tid == 0) row_n[blockIdx.x] = base;
}

// Pass 2b.  One workgroup: indptr[b0 + b + 1] = state[0] + the counts of rows b0 .. b0 + b, for the nb rows of the batch, on top of
// the running base state[0] = the pairs of the rows before the batch; state[1] = the longest row so far.  The first batch writes
// indptr[0] = 0.  state lives on the device from batch to batch: nothing is read back in between.
__global__ __launch_bounds__(256) void kz_radius_scan_batch_kernel(const int* __restrict__ row_n, int b0, int nb, int64_t* __restrict__ indptr,
                                                                   int64_t* __restrict__ state) {
    __shared__ long long s_w[4];
    __shared__ int s_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long base = state[0];   // (uniform)
    int longest = 0;
    for (int r0 = 0; r0 < nb; r0 += 256) {   // (uniform)
        const int r = r0 + tid;
        const int n = r < nb ? row_n[r] : 0;
        longest = n > longest ? n : longest;
        long long total;
        const long long before = kz_radius_tile_scan<long long>(n, s_w, lane, wave, total);
        if (r < nb) indptr[(int64_t)b0 + r + 1] = base + before + n;
        base += total;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int t = __shfl_xor(longest, o, 64);
        longest = t > longest ? t : longest;
    }
    if (lane == 0) s_max[wave] = longest;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < 4; ++w) longest = s_max[w] > longest ? s_max[w] : longest;
        if (b0 == 0) indptr[0] = 0;
        state[0] = base;
        state[1] = state[1] > longest ? state[1] : longest;
    }
}

// Pass 3.  Workgroup (c, b): nothing for a row that ends beyond `capacity` or a chunk without an entry; else the walk of the count
// again, in index order -- the element before the pairs, the pairs in steps of 512 consecutive values, the element behind them --
// and every entry written at indptr[row] + off[b][c] + (the chunk's entries before it): per step the four wave counts go through
// LDS (kz_knnr_exchange: one barrier), a lane's place inside its wave is a ballot prefix.  All of a thread's loads are issued
// before the first barrier of the round.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_radius_fill_kernel(const double* __restrict__ vals, int64_t n_i, int b0, int n_chunks, double radius,
                                                             double mp, const double* __restrict__ q_a, const double* __restrict__ q_b,
                                                             const double* __restrict__ t_a, const double* __restrict__ t_b,
                                                             const int* __restrict__ cnt, const int* __restrict__ off,
                                                             const int64_t* __restrict__ indptr, int64_t capacity,
                                                             int64_t* __restrict__ d_ind, double* __restrict__ d_dist) {
    constexpr bool ONE = KIND != KZ_RANK_NONE, TWO = KIND == KZ_RANK_MP_NORMAL;
    __shared__ int s_cnt[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = b0 + blockIdx.y;
    const int64_t at = (int64_t)blockIdx.y * n_chunks + blockIdx.x;
    if (cnt[at] == 0 || indptr[row + 1] > capacity) return;   // (uniform)
    int64_t pos = indptr[row] + off[at];                       // (uniform: the next free place)
    const int64_t row_end = indptr[row + 1];                   // (no store at or behind it, whatever the counts said)
    const double qa = ONE ? q_a[row] : 0.0, qb = TWO ? q_b[row] : 0.0;
    const KzRankChunk ch(blockIdx.y, blockIdx.x, KZ_RADIUS_CHUNK, n_i);
    auto w_at = [&](int64_t j) -> double {   // (uniform j: the scalar ends)
        return kz_radius_w<T, KIND, METRIC>(vals[ch.e0 + j], mp, qa, qb, ONE ? t_a[j] : 0.0, TWO ? t_b[j] : 0.0);
    };
    if (ch.a > ch.e0 + ch.j0) {   // the element before the pairs
        const double w = w_at(ch.j0);
        if (w <= radius) {
            if (tid == 0 && pos < row_end) {
                d_ind[pos] = ch.j0;
                d_dist[pos] = w;
            }
            ++pos;
        }
    }
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + ch.a);
    const unsigned long long below = (1ull << lane) - 1ull;
    int pass = 0;
    constexpr int U = 8;
    for (int p0 = 0; p0 < ch.n_pairs; p0 += 256 * U) {   // (uniform)
        double2 x[U];
        double ta[U][2], tb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const bool in = p < ch.n_pairs;
            const int64_t j = in ? ch.a - ch.e0 + 2 * (int64_t)p : ch.j0;
            x[u] = in ? pairs[p] : double2{0.0, 0.0};
            ta[u][0] = ONE ? t_a[j] : 0.0;
            ta[u][1] = ONE ? t_a[in ? j + 1 : j] : 0.0;
            tb[u][0] = TWO ? t_b[j] : 0.0;
            tb[u][1] = TWO ? t_b[in ? j + 1 : j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + 256 * u >= ch.n_pairs) break;   // (uniform)
            const int p = p0 + 256 * u + tid;
            const bool in = p < ch.n_pairs;
            const int64_t j = ch.a - ch.e0 + 2 * (int64_t)p;
            const double w0 = kz_radius_w<T, KIND, METRIC>(x[u].x, mp, qa, qb, ta[u][0], tb[u][0]);
            const double w1 = kz_radius_w<T, KIND, METRIC>(x[u].y, mp, qa, qb, ta[u][1], tb[u][1]);
            const bool c0 = in && w0 <= radius, c1 = in && w1 <= radius;
            const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
            const int* s = kz_knnr_exchange(s_cnt, pass, __popcll(m0) + __popcll(m1), lane, wave);
            int64_t place = pos + __popcll(m0 & below) + __popcll(m1 & below);
            for (int w = 0; w < wave; ++w) place += s[w];
            const int64_t place1 = place + (c0 ? 1 : 0);
            if (c0 && place < row_end) {
                d_ind[place] = j;
                d_dist[place] = w0;
            }
            if (c1 && place1 < row_end) {
                d_ind[place1] = j + 1;
                d_dist[place1] = w1;
            }
            pos += s[0] + s[1] + s[2] + s[3];
        }
    }
    if (ch.rem & 1) {   // the element behind the pairs
        const double w = w_at(ch.j1 - 1);
        if (w <= radius && tid == 0 && pos < row_end) {
            d_ind[pos] = ch.j1 - 1;
            d_dist[pos] = w;
        }
    }
}

// (w, index row) before (v, i) in the order of kz_knn_reduced: by kz_knnr_key, ties by smaller index row.
__device__ __forceinline__ bool kz_radius_before(double w, int r, double v, int i) {
    const unsigned long long kw = kz_knnr_key(w), kv = kz_knnr_key(v);
    return kw < kv || (kw == kv && r < i);
}

// The row sort.  One workgroup per row r of the call; rows that end beyond `capacity` were not written and are left alone.  A row
// comes ascending by index row (the fill's order) and leaves ascending by (kz_knnr_key(w), index row).
//  * up to KZ_RADIUS_SORT_LDS entries: (w, row) in LDS, padded with (+inf, INT_MAX) -- behind every entry: an index row is below
//    2^31 - 1 -- to the next power of two, a bitonic network (the pairs are distinct: any network gives the one order), written back.
//  * longer rows: a least-significant-digit radix sort of the keys, 8 bits a pass, between the row's place in d_dist / d_ind and the
//    same place in tmp_w / tmp_i (HBM).  Every pass is STABLE -- a tile of 256 consecutive entries goes out in order: a lane's place
//    among its wave's entries with the same digit is a ballot prefix, the waves of a tile and the tiles follow each other through
//    LDS counters -- so entries with one key stay in the order they came in, by index row.  Passes over a digit all keys share are
//    skipped; an odd number of passes ends with a copy back.  Barriers only; 3 per tile.
__global__ __launch_bounds__(256) void kz_radius_sort_kernel(const int64_t* __restrict__ indptr, int64_t capacity, double* d_dist, int64_t* d_ind,
                                                             double* tmp_w, int64_t* tmp_i) {
    __shared__ double s_v[KZ_RADIUS_SORT_LDS];
    __shared__ int s_r[KZ_RADIUS_SORT_LDS];
    __shared__ int s_base[256];       // radix path: the next free place of every digit
    __shared__ int s_wave[4][256];    // radix path: a tile's entries per (wave, digit); zero between tiles
    __shared__ int s_scan[4];
    __shared__ unsigned long long s_or[4], s_and[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t start = indptr[blockIdx.x], end = indptr[blockIdx.x + 1];
    if (end > capacity || end - start < 2) return;   // (uniform)
    const int n = (int)(end - start);
    if (n <= KZ_RADIUS_SORT_LDS) {
        int n_pad = 2;
        while (n_pad < n) n_pad <<= 1;
        for (int e = tid; e < n_pad; e += 256) {
            s_v[e] = e < n ? d_dist[start + e] : INFINITY;
            s_r[e] = e < n ? (int)d_ind[start + e] : 0x7fffffff;
        }
        __syncthreads();
        for (int k = 2; k <= n_pad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n_pad >> 1); t += 256) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const double vl = s_v[lo], vh = s_v[hi];
                    const int rl = s_r[lo], rh = s_r[hi];
                    const bool up = (lo & k) == 0;   // this run ascends
                    if (kz_radius_before(vh, rh, vl, rl) == up) {
                        s_v[lo] = vh;
                        s_v[hi] = vl;
                        s_r[lo] = rh;
                        s_r[hi] = rl;
                    }
                }
                __syncthreads();
            }
        for (int e = tid; e < n; e += 256) {
            d_dist[start + e] = s_v[e];
            d_ind[start + e] = s_r[e];
        }
        return;
    }
    // ---- the radix path ----
    unsigned long long all_or = 0ull, all_and = ~0ull;
    for (int e = tid; e < n; e += 256) {
        const unsigned long long key = kz_knnr_key(d_dist[start + e]);
        all_or |= key;
        all_and &= key;
    }
    for (int e = tid; e < 4 * 256; e += 256) (&s_wave[0][0])[e] = 0;
    kz_knnr_or_and(all_or, all_and, s_or, s_and, lane, wave);
    const unsigned long long differ = all_or ^ all_and;
    double* src_w = d_dist + start;
    int64_t* src_i = d_ind + start;
    double* dst_w = tmp_w + start;
    int64_t* dst_i = tmp_i + start;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int shift = 0; shift < 64; shift += 8) {
        if (((differ >> shift) & 0xffull) == 0ull) continue;   // (uniform: every key has the same digit here)
        s_base[tid] = 0;
        __syncthreads();
        for (int e = tid; e < n; e += 256) atomicAdd(&s_base[(int)((kz_knnr_key(src_w[e]) >> shift) & 0xffull)], 1);   // (LDS, integer)
        __syncthreads();
        {
            int total;
            const int mine = s_base[tid];
            const int before = kz_radius_tile_scan<int>(mine, s_scan, lane, wave, total);
            s_base[tid] = before;
        }
        __syncthreads();
        for (int e0 = 0; e0 < n; e0 += 256) {   // (uniform)
            const int e = e0 + tid;
            const bool in = e < n;
            const double w = in ? src_w[e] : 0.0;
            const int64_t r = in ? src_i[e] : 0;
            const int digit = (int)((kz_knnr_key(w) >> shift) & 0xffull);
            unsigned long long same = __ballot(in);   // the lanes of the wave with an entry of this lane's digit
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (digit >> bit) & 1;
                const unsigned long long m = __ballot(in && one);
                same &= one ? m : ~m;
            }
            const int rank = __popcll(same & below);
            const bool leader = in && rank == 0;
            if (leader) s_wave[wave][digit] = __popcll(same);
            __syncthreads();
            int before = 0, all = 0;
            if (in) {
                for (int v = 0; v < 4; ++v) {
                    const int c = s_wave[v][digit];
                    before += v < wave ? c : 0;
                    all += c;
                }
                const int place = s_base[digit] + before + rank;
                dst_w[place] = w;
                dst_i[place] = r;
            }
            __syncthreads();
            if (leader && before == 0) s_base[digit] += all;   // (the first wave that holds the digit: one thread per digit)
            __syncthreads();
            if (leader) s_wave[wave][digit] = 0;   // (its own wave's row: read again by others only behind the next tile's first barrier)
        }
        __syncthreads();   // (the pass's stores, before the next pass reads them)
        double* tw = src_w;
        src_w = dst_w;
        dst_w = tw;
        int64_t* ti = src_i;
        src_i = dst_i;
        dst_i = ti;
    }
    if (src_w != d_dist + start)   // (uniform: an odd number of passes)
        for (int e = tid; e < n; e += 256) {
            d_dist[start + e] = src_w[e];
            d_ind[start + e] = src_i[e];
        }
}

// The host side of both entry points (red == nullptr: the plain call, KZ_RANK_NONE).
static int kz_radius_impl(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, double radius,
                          int sorted, int64_t capacity, const KzRankReduction* red, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                          int64_t* h_total) {
    KZ_REQUIRE(radius == radius, "%s: radius is NaN", who);
    KZ_REQUIRE(capacity >= 0, "%s: capacity %lld is negative", who, (long long)capacity);
    KZ_REQUIRE(capacity == 0 || (d_ind && d_dist), "%s: d_ind / d_dist are required for capacity > 0", who);
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    KZ_HIP(hipSetDevice(ctx->device));
    *h_total = 0;
    if (q_count == 0) {
        KZ_HIP(hipMemsetAsync(d_indptr, 0, sizeof(int64_t), ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        return KZ_OK;
    }
    // (released when the function returns, stream-ordered)
    KzPoolBuf<int> fl;          // every row of the range, as the row list the exact stage takes
    KzPoolBuf<int> tab;         // cnt [batch][n_chunks], off [batch][n_chunks], row_n [batch]
    KzPoolBuf<int64_t> state;   // the running base, the longest row
    KzPoolBuf<double> tmp_w;    // the radix path of the sort
    KzPoolBuf<int64_t> tmp_i;
    int rc = fl.alloc(ctx, (size_t)q_count * sizeof(int));
    if (rc == KZ_OK) rc = state.alloc(ctx, 2 * sizeof(int64_t));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((q_count + 255) / 256)), dim3(256), 0, ctx->stream, fl.get(), (int)q_count);
    KZ_HIP(hipMemsetAsync(state.get(), 0, 2 * sizeof(int64_t), ctx->stream));
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_begin(ctx, index, (int)q_count, &batch, &vals);
    if (rc != KZ_OK) return rc;
    const int n_chunks = (int)((index->n + KZ_RADIUS_CHUNK - 1) / KZ_RADIUS_CHUNK);
    const size_t n_tab = (size_t)batch * n_chunks;
    rc = tab.alloc(ctx, (2 * n_tab + (size_t)batch) * sizeof(int));
    if (rc != KZ_OK) return rc;
    int* cnt = tab.get();
    int* off = cnt + n_tab;
    int* row_n = off + n_tab;
    const double* q_a = red ? red->q_a : nullptr;
    const double* q_b = red ? red->q_b : nullptr;
    const double* t_a = red ? red->t_a : nullptr;
    const double* t_b = red ? red->t_b : nullptr;
    // the kernels of one (dtype, kind, metric): `fill` false = the count
    auto launch = [&](bool fill, int b0, int nb) {
        auto go = [&](auto t, auto kd, auto metric) {
            using T = typename decltype(t)::type;
            constexpr int KIND = decltype(kd)::value, METRIC = decltype(metric)::value;
            if (!fill)
                hipLaunchKernelGGL((kz_radius_count_kernel<T, KIND, METRIC>), dim3(n_chunks, nb), dim3(256), 0, ctx->stream, (const double*)vals,
                                   index->n, b0, n_chunks, radius, index->mink_p, q_a, q_b, t_a, t_b, cnt);
            else
                hipLaunchKernelGGL((kz_radius_fill_kernel<T, KIND, METRIC>), dim3(n_chunks, nb), dim3(256), 0, ctx->stream, (const double*)vals,
                                   index->n, b0, n_chunks, radius, index->mink_p, q_a, q_b, t_a, t_b, (const int*)cnt, (const int*)off,
                                   (const int64_t*)d_indptr, capacity, d_ind, d_dist);
        };
        if (!red)
            kz_rank_dispatch_distance(index, [&](auto t, auto metric) { go(t, KzRankC<KZ_RANK_NONE>(), metric); });
        else
            kz_rank_dispatch(red->kind, index, go);
    };
    rc = kz_exact_walk(who, ctx, fl.get(), (int)q_count, batch, vals, q_begin, query, index, [&](int b0, int nb) {
        launch(false, b0, nb);
        hipLaunchKernelGGL(kz_radius_scan_rows_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const int*)cnt, n_chunks, off, row_n);
        hipLaunchKernelGGL(kz_radius_scan_batch_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)row_n, b0, nb, d_indptr, state.get());
        if (capacity > 0) launch(true, b0, nb);
    });
    if (rc != KZ_OK) return rc;
    int64_t h_state[2] = {0, 0};   // THE read-back: the total, the longest row
    KZ_HIP(hipMemcpyAsync(h_state, state.get(), sizeof(h_state), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    *h_total = h_state[0];
    if (!sorted || capacity == 0 || h_state[1] < 2) return KZ_OK;
    if (h_state[1] > KZ_RADIUS_SORT_LDS) {   // (a row the LDS path cannot hold: the radix path's second copy of what was written)
        const size_t n_out = (size_t)(h_state[0] < capacity ? h_state[0] : capacity);
        rc = tmp_w.alloc(ctx, n_out * sizeof(double));
        if (rc == KZ_OK) rc = tmp_i.alloc(ctx, n_out * sizeof(int64_t));
        if (rc != KZ_OK) return rc;
    }
    hipLaunchKernelGGL(kz_radius_sort_kernel, dim3((unsigned)q_count), dim3(256), 0, ctx->stream, (const int64_t*)d_indptr, capacity, d_dist, d_ind,
                       tmp_w.get(), tmp_i.get());
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

extern "C" int kz_radius_neighbors(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                   double radius, int sorted, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                                   int64_t* h_total) {
    // (the matrices are logically const for the caller: cosine attaches the lazily built normalised rows to the index, as kz_knn does)
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_radius_neighbors", ctx, query, q_begin, q_count, index, d_indptr, h_total);
    if (rcp != KZ_OK) return rcp;
    return kz_radius_impl("kz_radius_neighbors", ctx, query, q_begin, q_count, index, radius, sorted, capacity, nullptr, d_indptr, d_ind, d_dist,
                          h_total);
}

extern "C" int kz_radius_neighbors_reduced(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                           double radius, int sorted, int64_t capacity, int kind, const double* d_q_a, const double* d_q_b,
                                           const double* d_t_a, const double* d_t_b, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                                           int64_t* h_total) {
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_radius_neighbors_reduced", ctx, query, q_begin, q_count, index, d_indptr, h_total);
    if (rcp != KZ_OK) return rcp;
    const int rcr = kz_rank_require_reduction("kz_radius_neighbors_reduced", kind, d_q_a, d_q_b, d_t_a, d_t_b);
    if (rcr != KZ_OK) return rcr;
    const KzRankReduction red{kind, d_q_a, d_q_b, d_t_a, d_t_b};
    return kz_radius_impl("kz_radius_neighbors_reduced", ctx, query, q_begin, q_count, index, radius, sorted, capacity, &red, d_indptr, d_ind,
                          d_dist, h_total);
}
