// WHOLE-INDEX NEIGHBOUR LISTS UNDER A POINTWISE HUBNESS REDUCTION (kz_knn_reduced): per query row the k index rows with the smallest
// reduced distance w = f(d, state of the query row, state of the index row) over EVERY index row, ascending by (w, index row) -- the
// list that the ranks of kz_gold_ranks_reduced (kz_gold_ranks.h) are positions in: kz_gold_ranks_reduced with d_gold[r] = d_ind[r, c]
// gives c.  kz_csls / kz_local_scaling / kz_mp_normal rescale the K candidates of a list; a row outside that list can have a smaller
// reduced distance, so the k best of the rescaled candidates and the k best of all rows are two different lists.
//
// The host loop is kz_gold_ranks_impl's over all query rows: the float64 value matrix of the exact stage batch by batch
// (kz_exact_walk), w of every pair by that header's kz_rank_reduce -- the bits the transform kernels write -- and a SELECTION
// where it has a count, in two levels whatever the index size:
//   1. kz_knn_reduced_chunk_kernel: one workgroup per (chunk of KZ_KNNR_CHUNK index rows, row of the batch) computes the chunk's w in
//      registers and writes the min(k, chunk length) smallest (w, row) pairs;
//   2. kz_knn_reduced_merge_kernel: one workgroup per row of the batch picks the k smallest of the n_chunks x k survivors and writes
//      them sorted.
// Why not the selection kernels of the exact stage (kz_exact.h): they rank the search's own values, which are >= 0 and never NaN --
// their arg-min rounds start from "after (-1.0, -1)" and their radix threshold orders doubles by their bit patterns, which holds
// for non-negative values only.  CSLS values 2 d - a - b are routinely negative, a NaN or infinite state makes w NaN or +-inf.
// Here a w is compared through an ORDER-PRESERVING 64-BIT KEY (kz_knnr_key): a double with the sign bit set has all its bits
// flipped, any other gets the sign bit set -- unsigned keys then order like the doubles, -inf first -- after NaN has taken +inf's
// pattern and -0.0 that of +0.0: kz_rank_before's rule (NaN ranks as +inf, both tie by row; -0.0 == +0.0) as one integer compare.
// The w that is WRITTEN is the expression's own result: a NaN comes back as NaN.  Integer compares and counts only: nothing depends
// on the order the workgroups, or the waves of one, run in.
#pragma once
#include "kz_order_key.h"   // kz_knnr_key, KZ_KNNR_PAD

constexpr int KZ_KNNR_CHUNK = 4096;   // index rows per workgroup of the first level: 8 loads of 16 bytes, 16 keys per thread

// The workgroup's total of a wave-uniform count, to every thread: one exchange through LDS and ONE barrier -- the calls alternate
// between two sets of four counters (`pass`), so the writes of call n + 2 come after the barrier of call n + 1, which every thread
// passes after its reads of call n.  -> the four per-wave counts.
__device__ __forceinline__ const int* kz_knnr_exchange(int (*s_cnt)[4], int& pass, int cnt, int lane, int wave) {
    int* s = s_cnt[pass & 1];
    ++pass;
    if (lane == 0) s[wave] = cnt;
    __syncthreads();
    return s;
}

// The OR and the AND of the workgroup's keys, to every thread: the bits all keys share are those of all_and outside all_or ^ all_and
// (one barrier; it also publishes what the caller wrote to LDS before the call).
__device__ __forceinline__ void kz_knnr_or_and(unsigned long long& all_or, unsigned long long& all_and, unsigned long long* s_or,
                                               unsigned long long* s_and, int lane, int wave) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        all_or |= __shfl_xor(all_or, o, 64);
        all_and &= __shfl_xor(all_and, o, 64);
    }
    if (lane == 0) {
        s_or[wave] = all_or;
        s_and[wave] = all_and;
    }
    __syncthreads();
    all_or = s_or[0] | s_or[1] | s_or[2] | s_or[3];
    all_and = s_and[0] & s_and[1] & s_and[2] & s_and[3];
}

// THE THRESHOLD SEARCH of both levels, the approach of kz_exact_chunk_radix_kernel on the keys.  count(pred): the number of the
// workgroup's entries (key, row) that pred holds for, to every thread (kz_knnr_exchange: one barrier per call).  -> thr = the k-th
// smallest key, bit by bit below the keys' common prefix (the largest pattern with fewer than k keys below it): everything below
// thr survives, and of the entries equal to it the m that are still missing, by smallest row -- r_thr = the m-th smallest row among
// them by the same bit-by-bit count over ROW_BITS bits where there are more ties than places, else every row.
template <int ROW_BITS, typename Count>
__device__ __forceinline__ void kz_knnr_thresholds(unsigned long long all_or, unsigned long long all_and, int k, Count count,
                                                   unsigned long long& thr, int& r_thr) {
    const unsigned long long differ = all_or ^ all_and;
    const int top = differ ? 63 - __clzll(differ) : -1;
    thr = top < 0 ? all_and : (all_and & ~((2ull << top) - 1ull));
    for (int bit = top; bit >= 0; --bit) {   // (uniform)
        const unsigned long long cand = thr | (1ull << bit);
        if (count([&](unsigned long long key, int) { return key < cand; }) < k) thr = cand;
    }
    const unsigned long long t = thr;
    const int below = count([&](unsigned long long key, int) { return key < t; });
    const int ties = count([&](unsigned long long key, int) { return key == t; });
    const int m = k - below;   // places left for the entries equal to thr: 1 <= m <= ties
    r_thr = (int)((1u << ROW_BITS) - 1u);
    if (ties > m) {            // (uniform)
        r_thr = 0;
#pragma unroll 1   // (a rare path: ROW_BITS counting passes, not ROW_BITS copies of one)
        for (int bit = ROW_BITS - 1; bit >= 0; --bit) {
            const int cand = r_thr | (1 << bit);
            if (count([&](unsigned long long key, int r) { return key == t && r < cand; }) < m) r_thr = cand;
        }
    }
}

// Level 1.  vals [nb][n_i]: the value matrix of rows list[batch0 .. batch0 + nb).  Workgroup (c, b) owns the values [c KZ_KNNR_CHUNK,
// (c + 1) KZ_KNNR_CHUNK) of row b and writes the k_c = min(k, chunk length) smallest (w, index row) of them to places [0, k_c) of
// cand_w / cand_i [(b n_chunks + c) k ..], in no particular order; places [k_c, k) hold (+inf, INT_MAX).
// Loads as kz_rank_count_kernel has them (KzRankChunk): pairs (16-byte loads, all eight of a thread in flight) between the scalar
// ends; t_a / t_b by 8-byte gathers; the query side uniform.  The two scalar ends live in the pair slot that a chunk with a scalar
// end never fills (the last one, thread 255's eighth: an end leaves at most 4095 values to the pairs), so every thread holds eight
// slots = 16 keys and nothing else.  Selection: kz_knnr_thresholds on the chunk-local rows, 12 bits; a counting pass is 16 compares
// and ballots per thread and one barrier.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_knn_reduced_chunk_kernel(const double* __restrict__ vals, int64_t n_i, const int* __restrict__ list,
                                                                   int batch0, int k, int n_chunks, double mp,
                                                                   const double* __restrict__ q_a, const double* __restrict__ q_b,
                                                                   const double* __restrict__ t_a, const double* __restrict__ t_b,
                                                                   double* __restrict__ cand_w, int* __restrict__ cand_i) {
    constexpr bool TWO = KIND == KZ_RANK_MP_NORMAL;
    constexpr int U = KZ_KNNR_CHUNK / 512;   // pair slots per thread
    __shared__ int s_cnt[2][4];
    __shared__ unsigned long long s_or[4], s_and[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, b = blockIdx.y;
    const int row = list[batch0 + b];
    const double qa = q_a[row], qb = TWO ? q_b[row] : 0.0;
    const KzRankChunk ch(b, c, KZ_KNNR_CHUNK, n_i);
    const int64_t e0 = ch.e0, j0 = ch.j0, j1 = ch.j1;
    const int nvalid = (int)(j1 - j0);   // (>= 1: the chunk is not empty)
    const int n_pairs = ch.n_pairs, off = ch.off;
    const bool has_first = off == 1, has_last = (ch.rem & 1) != 0;
    const bool end_slot = tid == 255 && 256 * (U - 1) + 255 >= n_pairs;   // this thread's last slot holds the ends, not a pair
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + ch.a);
    auto local_row = [&](int u, int h) -> int {
        if (u == U - 1 && end_slot) return h ? nvalid - 1 : 0;
        return off + 2 * (256 * u + tid) + h;
    };
    auto reduce_at = [&](int64_t j) -> double {
        return kz_rank_reduce<T, KIND, METRIC>(vals[e0 + j], mp, qa, qb, t_a[j], TWO ? t_b[j] : 0.0);
    };

    unsigned long long key[2 * U];
    {
        double2 x[U];
        double ta[U][2], tb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = 256 * u + tid;
            const bool in = p < n_pairs;
            const int64_t ja = j0 + (in ? off + 2 * p : 0);   // (past the pairs: the chunk's first row, read and not used)
            const int64_t jb = in ? ja + 1 : (u == U - 1 && end_slot ? j1 - 1 : j0);
            x[u] = in ? pairs[p] : double2{0.0, 0.0};
            ta[u][0] = t_a[ja];
            ta[u][1] = t_a[jb];
            tb[u][0] = TWO ? t_b[ja] : 0.0;
            tb[u][1] = TWO ? t_b[jb] : 0.0;
        }
        const double x_first = vals[e0 + j0], x_last = vals[e0 + j1 - 1];   // (uniform; the ends where the chunk has them)
        if (end_slot) x[U - 1] = double2{x_first, x_last};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = 256 * u + tid < n_pairs;
            const bool ends = u == U - 1 && end_slot;
            const double w0 = kz_rank_reduce<T, KIND, METRIC>(x[u].x, mp, qa, qb, ta[u][0], tb[u][0]);
            const double w1 = kz_rank_reduce<T, KIND, METRIC>(x[u].y, mp, qa, qb, ta[u][1], tb[u][1]);
            key[2 * u] = in || (ends && has_first) ? kz_knnr_key(w0) : KZ_KNNR_PAD;
            key[2 * u + 1] = in || (ends && has_last) ? kz_knnr_key(w1) : KZ_KNNR_PAD;
        }
    }

    int pass = 0;
    // pred(u, h): one of this thread's 16 places -> the four per-wave counts of the places it holds for
    auto wave_counts = [&](auto pred) -> const int* {
        int cnt = 0;   // (wave-uniform: ballots)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cnt += __popcll(__ballot(pred(u, 0)));
            cnt += __popcll(__ballot(pred(u, 1)));
        }
        return kz_knnr_exchange(s_cnt, pass, cnt, lane, wave);
    };
    auto count = [&](auto pred) -> int {   // pred(key, chunk-local row)
        const int* s = wave_counts([&](int u, int h) { return pred(key[2 * u + h], local_row(u, h)); });
        return s[0] + s[1] + s[2] + s[3];
    };

    // the bits all keys of the chunk share (pads: no bit to the OR, every bit to the AND)
    unsigned long long all_or = 0ull, all_and = ~0ull;
#pragma unroll
    for (int e = 0; e < 2 * U; ++e) {
        all_or |= key[e] == KZ_KNNR_PAD ? 0ull : key[e];
        all_and &= key[e];
    }
    kz_knnr_or_and(all_or, all_and, s_or, s_and, lane, wave);
    const int k_c = k < nvalid ? k : nvalid;
    unsigned long long thr;
    int r_thr;
    static_assert(KZ_KNNR_CHUNK == 1 << 12, "the row threshold walks the 12 bits of a chunk-local row");
    kz_knnr_thresholds<12>(all_or, all_and, k_c, count, thr, r_thr);

    // the survivors, each wave behind the waves before it, a lane behind the lanes before it: exactly k_c places
    auto survives = [&](int u, int h) { return key[2 * u + h] < thr || (key[2 * u + h] == thr && local_row(u, h) <= r_thr); };
    const int* per_wave = wave_counts(survives);
    int pos = 0;
    for (int w = 0; w < wave; ++w) pos += per_wave[w];
    double* ow = cand_w + ((int64_t)b * n_chunks + c) * k;
    int* oi = cand_i + ((int64_t)b * n_chunks + c) * k;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool s = survives(u, h);
            const unsigned long long mask = __ballot(s);
            const int place = pos + __popcll(mask & ((1ull << lane) - 1ull));
            if (s && place < k_c) {
                const int64_t j = j0 + local_row(u, h);
                ow[place] = reduce_at(j);   // (w itself, not its key: a NaN stays a NaN)
                oi[place] = (int)j;
            }
            pos += __popcll(mask);
        }
    }
    for (int e = k_c + tid; e < k; e += 256) {   // (a last chunk shorter than k)
        ow[e] = INFINITY;
        oi[e] = 0x7fffffff;
    }
}

// Level 2.  Row b's n_e = n_chunks x k survivors (cand_w / cand_i [b n_e ..]; unused places (+inf, INT_MAX), behind every entry of
// an index row: at least k entries are real) -> the k smallest by (key, index row), sorted, to row list[batch0 + b] of d_w / d_ind.
// The same two thresholds (kz_knnr_thresholds on the index rows, 31 bits), with the entries streamed from L2 in every counting pass.
// The k entries that pass go to LDS (12 bytes each); an entry's place in the output is the number of those that come before it.
__global__ __launch_bounds__(256) void kz_knn_reduced_merge_kernel(const double* __restrict__ cand_w, const int* __restrict__ cand_i, int n_e,
                                                                   int k, const int* __restrict__ list, int batch0,
                                                                   double* __restrict__ d_w, int64_t* __restrict__ d_ind) {
    __shared__ int s_cnt[2][4];
    __shared__ unsigned long long s_or[4], s_and[4];
    __shared__ double s_w[KZ_KNN_REDUCED_MAX_K];
    __shared__ int s_r[KZ_KNN_REDUCED_MAX_K];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const double* __restrict__ cw = cand_w + (int64_t)b * n_e;
    const int* __restrict__ ci = cand_i + (int64_t)b * n_e;
    int pass = 0;
    // pred(key, index row) -> the number of the row's entries it holds for
    auto count = [&](auto pred) -> int {
        int cnt = 0;   // (wave-uniform: ballots)
        for (int i0 = 0; i0 < n_e; i0 += 256) {
            const int i = i0 + tid;
            const bool in = i < n_e;
            const unsigned long long key = in ? kz_knnr_key(cw[i]) : KZ_KNNR_PAD;
            const int r = in ? ci[i] : 0x7fffffff;
            cnt += __popcll(__ballot(in && pred(key, r)));
        }
        const int* s = kz_knnr_exchange(s_cnt, pass, cnt, lane, wave);
        return s[0] + s[1] + s[2] + s[3];
    };
    unsigned long long all_or = 0ull, all_and = ~0ull;
    for (int i = tid; i < n_e; i += 256) {
        const unsigned long long key = kz_knnr_key(cw[i]);
        all_or |= key;
        all_and &= key;
    }
    if (tid == 0) s_n = 0;
    kz_knnr_or_and(all_or, all_and, s_or, s_and, lane, wave);
    unsigned long long thr;
    int r_thr;   // (an index row: a real one, the unused places come last)
    kz_knnr_thresholds<31>(all_or, all_and, k, count, thr, r_thr);
    for (int i = tid; i < n_e; i += 256) {
        const double w = cw[i];
        const unsigned long long key = kz_knnr_key(w);
        const int r = ci[i];
        if (key < thr || (key == thr && r <= r_thr)) {
            const int place = atomicAdd(&s_n, 1);   // (any order: the places below are counted, not taken from this one)
            if (place < k) {
                s_w[place] = w;
                s_r[place] = r;
            }
        }
    }
    __syncthreads();
    const int64_t out = (int64_t)list[batch0 + b] * k;
    for (int s = tid; s < k; s += 256) {
        const double w = s_w[s];
        const unsigned long long key = kz_knnr_key(w);
        const int r = s_r[s];
        int place = 0;
        for (int t = 0; t < k; ++t) {
            const unsigned long long kt = kz_knnr_key(s_w[t]);
            place += kt < key || (kt == key && s_r[t] < r) ? 1 : 0;
        }
        d_w[out + place] = w;
        d_ind[out + place] = r;
    }
}

extern "C" int kz_knn_reduced(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c, int k,
                              int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a, const double* d_t_b, double* d_w,
                              int64_t* d_ind) {
    // (the matrices are logically const for the caller: cosine attaches the lazily built normalised rows to the index, as kz_knn does)
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_knn_reduced", ctx, query, q_begin, q_count, index, d_w, d_ind);
    if (rcp != KZ_OK) return rcp;
    KZ_REQUIRE(k >= 1 && k <= index->n, "kz_knn_reduced: Expected n_neighbors <= n_samples_fit and >= 1, but n_neighbors = %d, n_samples_fit = %lld",
               k, (long long)index->n);
    if (k > KZ_KNN_REDUCED_MAX_K) {
        kz_set_error("kz_knn_reduced: k = %d exceeds the maximum of %d neighbours per query (beyond it, kz_gold_ranks_reduced ranks any row)", k,
                     KZ_KNN_REDUCED_MAX_K);
        return KZ_ERR_UNSUPPORTED;
    }
    const int rcr = kz_rank_require_reduction("kz_knn_reduced", kind, d_q_a, d_q_b, d_t_a, d_t_b);
    if (rcr != KZ_OK) return rcr;
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "kz_knn_reduced: more than 2^31 - 1 rows");
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    // (released when the function returns, stream-ordered: cand_i, cand_w, fl)
    KzPoolBuf<int> fl;   // every row of the range, as the row list the exact stage takes
    KzPoolBuf<double> cand_w;
    KzPoolBuf<int> cand_i;
    int rc = fl.alloc(ctx, (size_t)q_count * sizeof(int));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((q_count + 255) / 256)), dim3(256), 0, ctx->stream, fl.get(), (int)q_count);
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_begin(ctx, index, (int)q_count, &batch, &vals);
    if (rc != KZ_OK) return rc;
    const int n_chunks = (int)((index->n + KZ_KNNR_CHUNK - 1) / KZ_KNNR_CHUNK);
    const size_t n_cand = (size_t)batch * n_chunks * k;
    rc = cand_w.alloc(ctx, n_cand * 8);
    if (rc == KZ_OK) rc = cand_i.alloc(ctx, n_cand * 4);
    if (rc != KZ_OK) return rc;
    const int* list = fl.get();
    double* cw = cand_w.get();
    int* ci = cand_i.get();
    // (the buffers go back to the pool behind the walk's synchronise; the caller reads d_w / d_ind next)
    return kz_exact_walk("kz_knn_reduced", ctx, list, (int)q_count, batch, vals, q_begin, query, index, [&](int b0, int nb) {
        // (kz_rank_dispatch: the instantiations of the count)
        kz_rank_dispatch(kind, index, [&](auto t, auto kd, auto metric) {
            hipLaunchKernelGGL((kz_knn_reduced_chunk_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(metric)::value>),
                               dim3(n_chunks, nb), dim3(256), 0, ctx->stream, (const double*)vals, index->n, list, b0, k, n_chunks, index->mink_p,
                               d_q_a, d_q_b, d_t_a, d_t_b, cw, ci);
        });
        hipLaunchKernelGGL(kz_knn_reduced_merge_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const double*)cw, (const int*)ci, n_chunks * k, k, list,
                           b0, d_w, d_ind);
    });
}
