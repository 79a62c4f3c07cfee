// GOLD RANKS (kz_gold_ranks): the exact rank of ONE known index row per query row against the whole index -- mean rank, mean
// reciprocal rank and hits@k beyond any candidate list (kiez_amd/evaluate.py: rank_metrics).
//
// The exact route of kz_knn_impl computes, per batch of listed query rows, the [batch][n_index] float64 matrix of the values the
// search ranks by and SELECTS k of them.  The rank of a known row g is the same matrix with a COUNT in place of the selection:
//     rank = #{ j : v_j < v_g  or  (v_j == v_g and j < g) }
// = the 0-based position of g in kz_knn(query, index, k = index.n, exclude_self = 0): the order of kz_exact_select_kernel, ties by
// smaller index row, NaN (correlation against a constant row, dice / sokalsneath between all-false rows) ranked as +inf by row.
// No list, no limit on k, no n x n output.  This header calls the distance function of the exact stage (kz_exact.h: static in
// kz_knn.hip's translation unit, hence an include like kz_range.h).
//   1. kz_rank_compact_kernel: the rows with a gold id inside [0, index.n), in row order, as a row list of the fail_list kind (int
//      rows relative to q_begin); d_rank = 0 for them, -1 for every other row.  One count comes back to the host.  Rows without gold
//      cost no distance work.
//   2. per batch of listed rows (kz_exact_begin, kz_exact_walk): kz_exact_distances -- the kernel the exact stage runs for this metric
//      and dtype;
//   3. kz_rank_count_kernel: one workgroup per (chunk of the index row range, listed row) counts its chunk and adds ONE integer to
//      the row's d_rank entry -- integer counting: the result does not depend on the order the workgroups run in.
// kz_gold_ranks_reduced is the same with step 3 counting the values' hubness-reduced distances (the kernel's KIND).
// The list those ranks are positions in -- a selection in place of the count: kz_knn_reduced.h.
// Reference: the n_s x n_t neighbour matrix of SklearnNN(n_candidates = n_target) followed by kiez.evaluate.hits
// (kiez/evaluate/eval_metrics.py:23-61) is the only way the reference reaches a rank.
#pragma once
#include "kz_reduce.h"   // the pointwise hubness reductions, shared with the transform kernels (kz_hubness.hip)

constexpr int KZ_RANK_CHUNK = 8192;   // values per workgroup of kz_rank_count_kernel: 16 loads of 16 bytes per thread

// list [n] + count at list[n]: the rows r of [0, n) with 0 <= gold[r] < n_i, ascending; rank[r] = 0 for them, else -1.
// One workgroup (the order of the list is the row order: batches are the same from call to call).
__global__ __launch_bounds__(256) void kz_rank_compact_kernel(const int64_t* __restrict__ gold, int n, int64_t n_i, int* __restrict__ list,
                                                              int64_t* __restrict__ rank) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;   // (uniform: every thread adds the same four counts)
    for (int r0 = 0; r0 < n; r0 += 256) {
        const int r = r0 + tid;
        bool ok = false;
        if (r < n) {
            const int64_t g = gold[r];
            ok = g >= 0 && g < n_i;   // (INT64_MIN: no gold row)
            rank[r] = ok ? 0 : -1;
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_w[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        if (ok) list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) list[n] = base;
}

// The walk of one chunk of a value row: workgroup (c, b) owns the values [j0, j1) = [c len, (c + 1) len) of row b of vals [nb][n_i].
// 16-byte loads: a row starts at an even or odd element of the (16-byte aligned) matrix, so the chunk is one scalar element up to
// the next even element, pairs, and one scalar element behind them.
struct KzRankChunk {
    int64_t e0;    // first element of the row in vals
    int64_t j0, j1;
    int64_t a;     // first even element at or behind the chunk's start
    int64_t rem;   // elements from a to the chunk's end (>= 0: the chunk is not empty); odd: a scalar element behind the pairs
    int n_pairs;
    int off;       // chunk-local row of the first paired element: 1 where a scalar element comes before the pairs, else 0
    __device__ __forceinline__ KzRankChunk(int b, int c, int len, int64_t n_i) {
        e0 = (int64_t)b * n_i;
        j0 = (int64_t)c * len;
        j1 = j0 + len < n_i ? j0 + len : n_i;
        a = (e0 + j0 + 1) & ~(int64_t)1;
        rem = e0 + j1 - a;
        n_pairs = (int)(rem >> 1);
        off = (int)(a - e0 - j0);
    }
};

__device__ __forceinline__ bool kz_rank_before(double v, int64_t j, double vg, int64_t g) {
    v = v != v ? INFINITY : v;
    return v < vg || (v == vg && j < g);
}

// ---- ranks under a pointwise hubness reduction (kz_gold_ranks_reduced) ---------------------------------------------------------
// CSLS, LocalScaling 'standard', NICDM, MutualProximity 'normal' and the dual potentials of Sinkhorn / the inverted softmax
// (KZ_RANK_DUAL: w = (d - f_i) - g_j) are functions w = f(d, state of the query row, state of the
// index row) of the pair's distance (kz_reduce.h), defined for EVERY index row and not for the K candidates alone: the count
// with the value converted to the distance the search returns (kz_output_distance<T>: what the transform kernels are fed) and
// reduced before it is compared.  The expressions are the transform kernels' own, so w of a candidate is the bits kz_csls /
// kz_local_scaling / kz_mp_normal write for it.  A NaN w (a NaN distance; radius or deviation 0 against distance 0) ranks as +inf
// by row.  MutualProximity 'normal' is exactly 1.0 for every pair far beyond both lists (kz_reduce_mp_normal): those pairs tie
// and go by row.
constexpr int KZ_RANK_NONE = 0;   // (internal, beside the public KZ_RANK_*: no reduction, the ranking value itself -- kz_gold_ranks)
struct KzRankReduction {
    int kind;            // KZ_RANK_CSLS .. KZ_RANK_MP_NORMAL, KZ_RANK_DUAL
    const double* q_a;   // [q_count], entry r for query row q_begin + r: mean (CSLS, NICDM), last (LS), nanmean (MP) of its forward list;
                         // DUAL: the potentials f (here) and g (t_a)
    const double* q_b;   // MP: nanstd; else null
    const double* t_a;   // [index.n]: the fit state of the index side, same statistic of the reverse lists
    const double* t_b;   // MP: nanstd; else null
};

// METRIC: the metric as a compile-time constant, so that kz_output_distance folds to the one conversion the launch needs (a count of
// euclidean values carries no pow(); kz_rank_out_metric below picks the constant).
template <typename T, int KIND, int METRIC>
__device__ __forceinline__ double kz_rank_reduce(double v, double p, double qa, double qb, double ta, double tb) {
    if (KIND == KZ_RANK_NONE) return v;
    const double d = kz_output_distance<T>(v, METRIC, p);
    if (KIND == KZ_RANK_CSLS) return kz_reduce_csls(d, qa, ta);
    if (KIND == KZ_RANK_LS) return kz_reduce_ls(d, qa, ta);
    if (KIND == KZ_RANK_NICDM) return kz_reduce_nicdm(d, qa, ta);
    if (KIND == KZ_RANK_DUAL) return kz_reduce_dual(d, qa, ta);
    return kz_reduce_mp_normal(d, qa, qb, ta, tb);
}

// vals [nb][n_i]: the value matrix of listed rows list[batch0 .. batch0 + nb).  Workgroup (c, b) counts, among the values of chunk c
// (KZ_RANK_CHUNK) of row b, those whose w kz_knn orders before that of the gold row g = gold[list[batch0 + b]] and adds the count to
// rank[list[batch0 + b]]: 16-byte value loads, eight in flight, the scalar ends, ballots, one atomic.
// The query-side scalars and the gold's own w are uniform over the workgroup (scalar loads, computed once).  The index-side vectors
// are read at j with 8-byte loads: a value row starts at an even or odd ELEMENT of the matrix, so the parity of j is not the
// parity of the value's address and t[j], t[j + 1] are not one aligned pair.  They are n_index x 8 (MP: 16) bytes read again by
// every row of the batch: L2 hits beside the 8 bytes per value that stream from HBM.  KZ_RANK_NONE reads no state at all.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_rank_count_kernel(const double* __restrict__ vals, int64_t n_i, const int* __restrict__ list,
                                                            int batch0, const int64_t* __restrict__ gold, double mp,
                                                            const double* __restrict__ q_a, const double* __restrict__ q_b,
                                                            const double* __restrict__ t_a, const double* __restrict__ t_b,
                                                            int64_t* __restrict__ rank) {
    constexpr bool ONE = KIND != KZ_RANK_NONE, TWO = KIND == KZ_RANK_MP_NORMAL;   // state vectors per side
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = list[batch0 + blockIdx.y];
    const int64_t g = gold[row];
    const double qa = ONE ? q_a[row] : 0.0, qb = TWO ? q_b[row] : 0.0;
    const KzRankChunk ch(blockIdx.y, blockIdx.x, KZ_RANK_CHUNK, n_i);
    auto reduce_at = [&](int64_t j) -> double {
        return kz_rank_reduce<T, KIND, METRIC>(vals[ch.e0 + j], mp, qa, qb, ONE ? t_a[j] : 0.0, TWO ? t_b[j] : 0.0);
    };
    double wg = reduce_at(g);
    wg = wg != wg ? INFINITY : wg;
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + ch.a);
    int cnt = 0;   // (wave-uniform: ballots)
    constexpr int U = 8;   // value loads in flight per thread
    for (int p0 = 0; p0 < ch.n_pairs; p0 += 256 * U) {   // (uniform)
        double2 x[U];
        double ta[U][2], tb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const bool in = p < ch.n_pairs;
            const int64_t j = in ? ch.a - ch.e0 + 2 * (int64_t)p : g;   // (past the chunk: the gold's own entries, never compared)
            x[u] = in ? pairs[p] : double2{0.0, 0.0};
            ta[u][0] = ONE ? t_a[j] : 0.0;
            ta[u][1] = ONE ? t_a[in ? j + 1 : g] : 0.0;
            tb[u][0] = TWO ? t_b[j] : 0.0;
            tb[u][1] = TWO ? t_b[in ? j + 1 : g] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const int64_t j = ch.a - ch.e0 + 2 * (int64_t)p;
            const double w0 = kz_rank_reduce<T, KIND, METRIC>(x[u].x, mp, qa, qb, ta[u][0], tb[u][0]);
            const double w1 = kz_rank_reduce<T, KIND, METRIC>(x[u].y, mp, qa, qb, ta[u][1], tb[u][1]);
            const bool c0 = p < ch.n_pairs && kz_rank_before(w0, j, wg, g);
            const bool c1 = p < ch.n_pairs && kz_rank_before(w1, j + 1, wg, g);
            cnt += __popcll(__ballot(c0)) + __popcll(__ballot(c1));
        }
    }
    if (wave == 0) {   // the chunk's scalar ends: lane 0 the element before the pairs, lane 1 the one behind them
        bool c = false;
        const bool first = lane == 0 && ch.a > ch.e0 + ch.j0, last = lane == 1 && (ch.rem & 1);
        if (first || last) {
            const int64_t j = first ? ch.j0 : ch.j1 - 1;
            c = kz_rank_before(reduce_at(j), j, wg, g);
        }
        cnt += __popcll(__ballot(c));
    }
    if (lane == 0) s_w[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(rank + row), (unsigned long long)total);
    }
}

// The constant a launch passes for METRIC: the three metrics kz_output_distance converts stand for themselves, KZ_CORRELATION for
// those whose +inf ranking value is a NaN distance, KZ_COSINE for every metric whose ranking value IS the distance returned
// (KZ_PRECOMPUTED among them: the matrix entry as it is).
static int kz_rank_out_metric(int metric) {
    if (metric == KZ_EUCLIDEAN || metric == KZ_SEUCLIDEAN || metric == KZ_MINKOWSKI) return metric;
    return metric == KZ_CORRELATION || metric == KZ_DICE || metric == KZ_SOKALSNEATH ? KZ_CORRELATION : KZ_COSINE;
}

// THE kind x metric x dtype dispatch of the kernels that reduce a value (the count above, the first level of kz_knn_reduced.h):
// launch(KzRankT<T>, KzRankC<KIND>, KzRankC<METRIC>) is called with the one combination the reduction and the index ask for.
// (The input dtype decides the rounding of the three converted metrics only: the others have one instantiation.)
// kz_rank_dispatch_distance is its metric x dtype half, by_kind(KzRankT<T>, KzRankC<METRIC>): what a kernel needs that converts a
// value to the distance and does something else with it (the soft-min, kz_softmin.h).
template <typename T>
struct KzRankT {
    using type = T;
};
template <int V>
using KzRankC = std::integral_constant<int, V>;
template <typename F>
static void kz_rank_dispatch_distance(const kz_matrix* index, F by_kind) {
    // (these kernels read the float64 value matrix: T is the output convention -- float for float32 rows, double for float64 and the
    //  2-byte types; an element type that is none of the four launches nothing, and kz_matrix_create never made such a matrix)
    auto by_dtype = [&](auto metric) {
        (void)kz_dispatch_values(index->dtype, "kz_gold_ranks", [&](auto e) {
            by_kind(KzRankT<typename decltype(e)::type>(), metric);
            return (int)KZ_OK;
        });
    };
    switch (kz_rank_out_metric(index->metric)) {
        case KZ_EUCLIDEAN: by_dtype(KzRankC<KZ_EUCLIDEAN>()); break;
        case KZ_SEUCLIDEAN: by_dtype(KzRankC<KZ_SEUCLIDEAN>()); break;
        case KZ_MINKOWSKI: by_dtype(KzRankC<KZ_MINKOWSKI>()); break;
        case KZ_CORRELATION: by_kind(KzRankT<double>(), KzRankC<KZ_CORRELATION>()); break;
        default: by_kind(KzRankT<double>(), KzRankC<KZ_COSINE>()); break;
    }
}
template <typename F>
static void kz_rank_dispatch(int kind, const kz_matrix* index, F launch) {
    kz_rank_dispatch_distance(index, [&](auto t, auto metric) {
        switch (kind) {
            case KZ_RANK_CSLS: launch(t, KzRankC<KZ_RANK_CSLS>(), metric); break;
            case KZ_RANK_LS: launch(t, KzRankC<KZ_RANK_LS>(), metric); break;
            case KZ_RANK_NICDM: launch(t, KzRankC<KZ_RANK_NICDM>(), metric); break;
            case KZ_RANK_DUAL: launch(t, KzRankC<KZ_RANK_DUAL>(), metric); break;
            default: launch(t, KzRankC<KZ_RANK_MP_NORMAL>(), metric); break;
        }
    });
}

static int kz_rank_require_reduction(const char* who, int kind, const double* q_a, const double* q_b, const double* t_a, const double* t_b) {
    KZ_REQUIRE((kind >= KZ_RANK_CSLS && kind <= KZ_RANK_MP_NORMAL) || kind == KZ_RANK_DUAL,
               "%s: unknown kind %d (KZ_RANK_CSLS .. KZ_RANK_MP_NORMAL, KZ_RANK_DUAL)", who, kind);
    KZ_REQUIRE(q_a && t_a, "%s: the query-side and index-side state vectors d_q_a / d_t_a are required", who);
    if (kind == KZ_RANK_MP_NORMAL)
        KZ_REQUIRE(q_b && t_b, "%s: KZ_RANK_MP_NORMAL needs the deviations d_q_b / d_t_b", who);
    else
        KZ_REQUIRE(!q_b && !t_b, "%s: d_q_b / d_t_b belong to KZ_RANK_MP_NORMAL only and must be NULL for kind %d", who, kind);
    return KZ_OK;
}

// The host side of both entry points: the compaction, then the walk of the exact stage (kz_exact_walk) over the listed rows with the
// count per batch -- of the values themselves (red == nullptr: the one instantiation <double, KZ_RANK_NONE, KZ_COSINE>) or of their
// reduced distances.
static int kz_gold_ranks_impl(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index,
                              const int64_t* d_gold, const KzRankReduction* red, int64_t* d_rank) {
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));

    KzPoolBuf<int> fl;   // [q_count] listed rows + the count
    int rc = fl.alloc(ctx, ((size_t)q_count + 1) * sizeof(int));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_rank_compact_kernel, dim3(1), dim3(256), 0, ctx->stream, d_gold, (int)q_count, index->n, fl.get(), d_rank);
    KZ_HIP(hipGetLastError());
    int n_list = 0;
    KZ_HIP(hipMemcpyAsync(&n_list, fl.get() + q_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (n_list == 0) return KZ_OK;

    // the value matrix of the exact stage (kz_exact.h), batch by batch; the count in place of its selection
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_begin(ctx, index, n_list, &batch, &vals);
    if (rc != KZ_OK) return rc;
    const int n_chunks = (int)((index->n + KZ_RANK_CHUNK - 1) / KZ_RANK_CHUNK);
    const int* list = fl.get();
    // (fl goes back to the pool behind the walk's synchronise; the caller reads d_rank next)
    return kz_exact_walk(who, ctx, list, n_list, batch, vals, q_begin, query, index, [&](int b0, int nb) {
        const dim3 grid(n_chunks, nb);
        if (!red)
            hipLaunchKernelGGL((kz_rank_count_kernel<double, KZ_RANK_NONE, KZ_COSINE>), grid, dim3(256), 0, ctx->stream, (const double*)vals, index->n,
                               list, b0, d_gold, 0.0, nullptr, nullptr, nullptr, nullptr, d_rank);
        else
            kz_rank_dispatch(red->kind, index, [&](auto t, auto kind, auto metric) {
                hipLaunchKernelGGL((kz_rank_count_kernel<typename decltype(t)::type, decltype(kind)::value, decltype(metric)::value>), grid, dim3(256),
                                   0, ctx->stream, (const double*)vals, index->n, list, b0, d_gold, index->mink_p, red->q_a, red->q_b, red->t_a,
                                   red->t_b, d_rank);
            });
    });
}

extern "C" int kz_gold_ranks(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                             const int64_t* d_gold, int64_t* d_rank) {
    // (the matrices are logically const for the caller: cosine attaches the lazily built normalised rows to the index, as kz_knn does)
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_gold_ranks", ctx, query, q_begin, q_count, index, d_gold, d_rank);
    if (rcp != KZ_OK) return rcp;
    return kz_gold_ranks_impl("kz_gold_ranks", ctx, query, q_begin, q_count, index, d_gold, nullptr, d_rank);
}

extern "C" int kz_gold_ranks_reduced(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                     const int64_t* d_gold, int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a,
                                     const double* d_t_b, int64_t* d_rank) {
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_gold_ranks_reduced", ctx, query, q_begin, q_count, index, d_gold, d_rank);
    if (rcp != KZ_OK) return rcp;
    const int rcr = kz_rank_require_reduction("kz_gold_ranks_reduced", kind, d_q_a, d_q_b, d_t_a, d_t_b);
    if (rcr != KZ_OK) return rcr;
    const KzRankReduction red{kind, d_q_a, d_q_b, d_t_a, d_t_b};
    return kz_gold_ranks_impl("kz_gold_ranks_reduced", ctx, query, q_begin, q_count, index, d_gold, &red, d_rank);
}
