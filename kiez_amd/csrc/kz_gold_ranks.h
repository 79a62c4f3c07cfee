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
// Reference: the n_s x n_t neighbour matrix of SklearnNN(n_candidates = n_target) followed by kiez.evaluate.hits
// (kiez/evaluate/eval_metrics.py:23-61) is the only way the reference reaches a rank.
#pragma once

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

extern "C" int kz_gold_ranks(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                             const int64_t* d_gold, int64_t* d_rank) {
    // (the matrices are logically const for the caller: cosine attaches the lazily built normalised rows to the index, as kz_knn does)
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    {
        const int rcp = kz_require_pair("kz_gold_ranks", ctx, query, q_begin, q_count, index, d_gold, d_rank);
        if (rcp != KZ_OK) return rcp;
    }
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "kz_gold_ranks: more than 2^31 - 1 rows");
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
        hipLaunchKernelGGL(kz_rank_count_kernel, dim3(n_chunks, nb), dim3(256), 0, ctx->stream, (const double*)vals, index->n, fl.get(), b0,
                           d_gold, d_rank);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (fl goes back to the pool; the caller reads d_rank next)
    if (e != hipSuccess) {
        kz_set_error("kz_gold_ranks: exact kernels failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    return KZ_OK;
}
