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
//   2. per batch of listed rows (kz_exact_batch_rows): kz_exact_distances -- the kernel the exact stage runs for this metric and dtype;
//   3. kz_rank_count_kernel: one workgroup per (chunk of the index row range, listed row) counts its chunk and adds ONE integer to
//      the row's d_rank entry -- integer counting: the result does not depend on the order the workgroups run in.
// kz_gold_ranks_reduced is the same with step 3 counting the values' hubness-reduced distances (kz_rank_count_reduced_kernel below).
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

// vals [nb][n_i]: the value matrix of listed rows list[batch0 .. batch0 + nb).  Workgroup (c, b) counts, among the values
// [c KZ_RANK_CHUNK, (c + 1) KZ_RANK_CHUNK) of row b, those that kz_knn orders before the gold row g = gold[list[batch0 + b]] and adds the
// count to rank[list[batch0 + b]].  16-byte loads: a row starts at an even or odd element of the (16-byte aligned) matrix, so the
// chunk is one scalar element up to the next even element, pairs, and one scalar element behind them.
__device__ __forceinline__ bool kz_rank_before(double v, int64_t j, double vg, int64_t g) {
    v = v != v ? INFINITY : v;
    return v < vg || (v == vg && j < g);
}
__global__ __launch_bounds__(256) void kz_rank_count_kernel(const double* __restrict__ vals, int64_t n_i, const int* __restrict__ list,
                                                            int batch0, const int64_t* __restrict__ gold, int64_t* __restrict__ rank) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int row = list[batch0 + b];
    const int64_t g = gold[row];
    const int64_t e0 = (int64_t)b * n_i;   // first element of the row in vals
    double vg = vals[e0 + g];
    vg = vg != vg ? INFINITY : vg;
    const int64_t j0 = (int64_t)blockIdx.x * KZ_RANK_CHUNK;
    const int64_t j1 = j0 + KZ_RANK_CHUNK < n_i ? j0 + KZ_RANK_CHUNK : n_i;
    const int64_t a = (e0 + j0 + 1) & ~(int64_t)1;   // first even element at or behind the chunk's start
    const int64_t rem = e0 + j1 - a;                 // (>= 0: the chunk is not empty)
    const int n_pairs = (int)(rem >> 1);
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + a);
    int cnt = 0;   // (wave-uniform: ballots)
    constexpr int U = 8;   // loads in flight per thread
    for (int p0 = 0; p0 < n_pairs; p0 += 256 * U) {   // (uniform)
        double2 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            x[u] = p < n_pairs ? pairs[p] : double2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const int64_t j = a - e0 + 2 * (int64_t)p;
            const bool c0 = p < n_pairs && kz_rank_before(x[u].x, j, vg, g);
            const bool c1 = p < n_pairs && kz_rank_before(x[u].y, j + 1, vg, g);
            cnt += __popcll(__ballot(c0)) + __popcll(__ballot(c1));
        }
    }
    if (wave == 0) {   // the chunk's scalar ends: lane 0 the element before the pairs, lane 1 the one behind them
        bool c = false;
        if (lane == 0 && a > e0 + j0) c = kz_rank_before(vals[e0 + j0], j0, vg, g);
        if (lane == 1 && (rem & 1)) c = kz_rank_before(vals[e0 + j1 - 1], j1 - 1, vg, g);
        cnt += __popcll(__ballot(c));
    }
    if (lane == 0) s_w[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(rank + row), (unsigned long long)total);
    }
}

// ---- ranks under a pointwise hubness reduction (kz_gold_ranks_reduced) ---------------------------------------------------------
// CSLS, LocalScaling 'standard', NICDM and MutualProximity 'normal' are functions w = f(d, state of the query row, state of the
// index row) of the pair's distance (kz_reduce.h), defined for EVERY index row and not for the K candidates alone: the count above
// with the value converted to the distance the search returns (kz_output_distance<T>: what the transform kernels are fed) and
// reduced before it is compared.  The expressions are the transform kernels' own, so w of a candidate is the bits kz_csls /
// kz_local_scaling / kz_mp_normal write for it.  A NaN w (a NaN distance; radius or deviation 0 against distance 0) ranks as +inf
// by row.  MutualProximity 'normal' is exactly 1.0 for every pair far beyond both lists (kz_reduce_mp_normal): those pairs tie
// and go by row.
struct KzRankReduction {
    int kind;            // KZ_RANK_CSLS .. KZ_RANK_MP_NORMAL
    const double* q_a;   // [q_count], entry r for query row q_begin + r: mean (CSLS, NICDM), last (LS), nanmean (MP) of its forward list
    const double* q_b;   // MP: nanstd; else null
    const double* t_a;   // [index.n]: the fit state of the index side, same statistic of the reverse lists
    const double* t_b;   // MP: nanstd; else null
};

// METRIC: the metric as a compile-time constant, so that kz_output_distance folds to the one conversion the launch needs (a count of
// euclidean values carries no pow(); kz_rank_out_metric below picks the constant).
template <typename T, int KIND, int METRIC>
__device__ __forceinline__ double kz_rank_reduce(double v, double p, double qa, double qb, double ta, double tb) {
    const double d = kz_output_distance<T>(v, METRIC, p);
    if (KIND == KZ_RANK_CSLS) return kz_reduce_csls(d, qa, ta);
    if (KIND == KZ_RANK_LS) return kz_reduce_ls(d, qa, ta);
    if (KIND == KZ_RANK_NICDM) return kz_reduce_nicdm(d, qa, ta);
    return kz_reduce_mp_normal(d, qa, qb, ta, tb);
}

// The layout of kz_rank_count_kernel: workgroup (c, b), 16-byte value loads, eight in flight, the scalar ends, ballots, one atomic.
// The query-side scalars and the gold's own w are uniform over the workgroup (scalar loads, computed once).  The index-side vectors
// are read at j with 8-byte loads: a value row starts at an even or odd ELEMENT of the matrix, so the parity of j is not the
// parity of the value's address and t[j], t[j + 1] are not one aligned pair.  They are n_index x 8 (MP: 16) bytes read again by
// every row of the batch: L2 hits beside the 8 bytes per value that stream from HBM.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_rank_count_reduced_kernel(const double* __restrict__ vals, int64_t n_i, const int* __restrict__ list,
                                                                    int batch0, const int64_t* __restrict__ gold, double mp,
                                                                    const double* __restrict__ q_a, const double* __restrict__ q_b,
                                                                    const double* __restrict__ t_a, const double* __restrict__ t_b,
                                                                    int64_t* __restrict__ rank) {
    constexpr bool TWO = KIND == KZ_RANK_MP_NORMAL;
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int row = list[batch0 + b];
    const int64_t g = gold[row];
    const double qa = q_a[row], qb = TWO ? q_b[row] : 0.0;
    const int64_t e0 = (int64_t)b * n_i;   // first element of the row in vals
    double wg = kz_rank_reduce<T, KIND, METRIC>(vals[e0 + g], mp, qa, qb, t_a[g], TWO ? t_b[g] : 0.0);
    wg = wg != wg ? INFINITY : wg;
    const int64_t j0 = (int64_t)blockIdx.x * KZ_RANK_CHUNK;
    const int64_t j1 = j0 + KZ_RANK_CHUNK < n_i ? j0 + KZ_RANK_CHUNK : n_i;
    const int64_t a = (e0 + j0 + 1) & ~(int64_t)1;   // first even element at or behind the chunk's start
    const int64_t rem = e0 + j1 - a;                 // (>= 0: the chunk is not empty)
    const int n_pairs = (int)(rem >> 1);
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(vals + a);
    int cnt = 0;   // (wave-uniform: ballots)
    constexpr int U = 8;   // value loads in flight per thread
    for (int p0 = 0; p0 < n_pairs; p0 += 256 * U) {   // (uniform)
        double2 x[U];
        double ta[U][2], tb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const bool in = p < n_pairs;
            const int64_t j = in ? a - e0 + 2 * (int64_t)p : g;   // (past the chunk: the gold's own entries, never compared)
            x[u] = in ? pairs[p] : double2{0.0, 0.0};
            ta[u][0] = t_a[j];
            ta[u][1] = t_a[in ? j + 1 : g];
            tb[u][0] = TWO ? t_b[j] : 0.0;
            tb[u][1] = TWO ? t_b[in ? j + 1 : g] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + 256 * u + tid;
            const int64_t j = a - e0 + 2 * (int64_t)p;
            const double w0 = kz_rank_reduce<T, KIND, METRIC>(x[u].x, mp, qa, qb, ta[u][0], tb[u][0]);
            const double w1 = kz_rank_reduce<T, KIND, METRIC>(x[u].y, mp, qa, qb, ta[u][1], tb[u][1]);
            const bool c0 = p < n_pairs && kz_rank_before(w0, j, wg, g);
            const bool c1 = p < n_pairs && kz_rank_before(w1, j + 1, wg, g);
            cnt += __popcll(__ballot(c0)) + __popcll(__ballot(c1));
        }
    }
    if (wave == 0) {   // the chunk's scalar ends: lane 0 the element before the pairs, lane 1 the one behind them
        bool c = false;
        const bool first = lane == 0 && a > e0 + j0, last = lane == 1 && (rem & 1);
        if (first || last) {
            const int64_t j = first ? j0 : j1 - 1;
            c = kz_rank_before(kz_rank_reduce<T, KIND, METRIC>(vals[e0 + j], mp, qa, qb, t_a[j], TWO ? t_b[j] : 0.0), j, wg, g);
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
// those whose +inf ranking value is a NaN distance, KZ_COSINE for every metric whose ranking value IS the distance returned.
static int kz_rank_out_metric(int metric) {
    if (metric == KZ_EUCLIDEAN || metric == KZ_SEUCLIDEAN || metric == KZ_MINKOWSKI) return metric;
    return metric == KZ_CORRELATION || metric == KZ_DICE || metric == KZ_SOKALSNEATH ? KZ_CORRELATION : KZ_COSINE;
}

template <typename T, int METRIC>
static void kz_rank_count_reduced_launch(kz_ctx* ctx, const KzRankReduction& red, dim3 grid, const double* vals, const kz_matrix* index,
                                         const int* list, int batch0, const int64_t* d_gold, int64_t* d_rank) {
#define KZ_RANK_LAUNCH(KIND)                                                                                                                 \
    hipLaunchKernelGGL((kz_rank_count_reduced_kernel<T, KIND, METRIC>), grid, dim3(256), 0, ctx->stream, vals, index->n, list, batch0, d_gold, \
                       index->mink_p, red.q_a, red.q_b, red.t_a, red.t_b, d_rank)
    switch (red.kind) {
        case KZ_RANK_CSLS: KZ_RANK_LAUNCH(KZ_RANK_CSLS); break;
        case KZ_RANK_LS: KZ_RANK_LAUNCH(KZ_RANK_LS); break;
        case KZ_RANK_NICDM: KZ_RANK_LAUNCH(KZ_RANK_NICDM); break;
        default: KZ_RANK_LAUNCH(KZ_RANK_MP_NORMAL); break;
    }
#undef KZ_RANK_LAUNCH
}

// (the input dtype decides the rounding of the three converted metrics only: the others have one instantiation)
static void kz_rank_count_reduced(kz_ctx* ctx, const KzRankReduction& red, dim3 grid, const double* vals, const kz_matrix* index,
                                  const int* list, int batch0, const int64_t* d_gold, int64_t* d_rank) {
#define KZ_RANK_METRIC(T, METRIC) kz_rank_count_reduced_launch<T, METRIC>(ctx, red, grid, vals, index, list, batch0, d_gold, d_rank)
    const bool f32 = index->dtype == KZ_F32;
    switch (kz_rank_out_metric(index->metric)) {
        case KZ_EUCLIDEAN: if (f32) KZ_RANK_METRIC(float, KZ_EUCLIDEAN); else KZ_RANK_METRIC(double, KZ_EUCLIDEAN); break;
        case KZ_SEUCLIDEAN: if (f32) KZ_RANK_METRIC(float, KZ_SEUCLIDEAN); else KZ_RANK_METRIC(double, KZ_SEUCLIDEAN); break;
        case KZ_MINKOWSKI: if (f32) KZ_RANK_METRIC(float, KZ_MINKOWSKI); else KZ_RANK_METRIC(double, KZ_MINKOWSKI); break;
        case KZ_CORRELATION: KZ_RANK_METRIC(double, KZ_CORRELATION); break;
        default: KZ_RANK_METRIC(double, KZ_COSINE); break;
    }
#undef KZ_RANK_METRIC
}

// The host side of both entry points: the compaction, the value matrix of the exact stage batch by batch, and per batch the count
// -- of the values themselves (red == nullptr: kz_rank_count_kernel) or of their reduced distances.
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
    rc = kz_exact_prepare_index(ctx, index, n_list);
    if (rc != KZ_OK) return rc;
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_batch_rows(ctx, index, n_list, &batch, &vals);
    if (rc != KZ_OK) return rc;
    const int n_chunks = (int)((index->n + KZ_RANK_CHUNK - 1) / KZ_RANK_CHUNK);
    for (int b0 = 0; b0 < n_list; b0 += batch) {
        const int nb = n_list - b0 < batch ? n_list - b0 : batch;
        rc = kz_exact_distances(ctx, fl.get(), b0, nb, q_begin, query, index, vals);
        if (rc != KZ_OK) return rc;
        if (!red)
            hipLaunchKernelGGL(kz_rank_count_kernel, dim3(n_chunks, nb), dim3(256), 0, ctx->stream, (const double*)vals, index->n, fl.get(), b0,
                               d_gold, d_rank);
        else
            kz_rank_count_reduced(ctx, *red, dim3(n_chunks, nb), vals, index, fl.get(), b0, d_gold, d_rank);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (fl goes back to the pool; the caller reads d_rank next)
    if (e != hipSuccess) {
        kz_set_error("%s: exact kernels failed: %s", who, hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    return KZ_OK;
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
    KZ_REQUIRE(kind >= KZ_RANK_CSLS && kind <= KZ_RANK_MP_NORMAL, "kz_gold_ranks_reduced: unknown kind %d (KZ_RANK_CSLS .. KZ_RANK_MP_NORMAL)", kind);
    KZ_REQUIRE(d_q_a && d_t_a, "kz_gold_ranks_reduced: the query-side and index-side state vectors d_q_a / d_t_a are required");
    if (kind == KZ_RANK_MP_NORMAL)
        KZ_REQUIRE(d_q_b && d_t_b, "kz_gold_ranks_reduced: KZ_RANK_MP_NORMAL needs the deviations d_q_b / d_t_b");
    else
        KZ_REQUIRE(!d_q_b && !d_t_b, "kz_gold_ranks_reduced: d_q_b / d_t_b belong to KZ_RANK_MP_NORMAL only and must be NULL for kind %d", kind);
    const KzRankReduction red{kind, d_q_a, d_q_b, d_t_a, d_t_b};
    return kz_gold_ranks_impl("kz_gold_ranks_reduced", ctx, query, q_begin, q_count, index, d_gold, &red, d_rank);
}
