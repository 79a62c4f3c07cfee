// ROW-WISE SOFT-MIN OVER THE WHOLE INDEX (kz_softmin_rows): per query row r
//     out[r] = softmin_eps over every index row j of (d_rj - off[j])  +  shift,     softmin_eps(x) = m - eps log sum exp(-(x - m) / eps), m = min x
// -- the one primitive behind the Sinkhorn potentials and the inverted softmax (kiez_amd/hubness_reduction.py): a row step is this call,
// a column step the same call with target as query and source as index.  The exact float64 value launchers (kz_exact.h) have a count
// (kz_gold_ranks.h) and a selection (kz_knn_reduced.h) as callers; this is the third, a REDUCTION.  The host loop is kz_knn_reduced's
// over all query rows: the value matrix batch by batch (kz_exact_walk), d of every pair by kz_output_distance<T> -- the conversion
// kz_rank_reduce applies, folded per (dtype, metric) by kz_rank_dispatch_distance -- and two levels whatever the index size:
//   1. kz_softmin_chunk_kernel: one workgroup per (chunk of KZ_SOFTMIN_CHUNK index rows, row of the batch) writes the chunk's
//      (m, s) (KzSoftminPart, kz_reduce.h) to part [nb][n_chunks];
//   2. kz_softmin_fold_kernel (kz_softmin.hip): one wave per row folds the row's n_chunks parts into out[r].
// Why two levels: one workgroup per row would leave a batch of a few hundred rows on a few hundred workgroups with 8 bytes per pair to
// stream; chunks x rows fills the device at any shape, and the second level reads n_chunks x 16 bytes per row.  The alternative -- every
// chunk adding into the row's result -- needs a floating-point atomic or a workgroup that waits for another: neither is used.
//
// THE TREE RULE.  The order in which a row's terms are added is a function of j, index.n and KZ_SOFTMIN_CHUNK only: thread t of the
// chunk's workgroup owns the index rows j0 + 256 u + t (u ascending), read with coalesced 8-byte loads indexed by j -- not the
// address-aligned 16-byte pairs of KzRankChunk, whose lane <-> element map follows the parity of the row's start address -- then the
// 64 lanes of a wave by xor butterflies (both partners add the same two numbers: every lane holds the same bits), the four waves as
// (w0 + w1) + (w2 + w3), the chunks at level 2 in their own fixed tree.  So a row's result has the same bits wherever the row stands in
// the batch, however the call is split into batches or row ranges, and from run to run.
//
// SPECIAL VALUES.  A NaN entry (a NaN distance: correlation against a constant row; a NaN offset) counts as +inf and contributes
// nothing.  The chunk minimum comes first, then the sum: every exponent is <= 0 and the minimum's own term is exactly 1, so no term
// overflows and the sum is >= 1 -- log never sees 0 however small eps is.  A chunk without an entry below +inf is (+inf, 0), one that
// holds a -inf is (-inf, 1); neither evaluates exp.
#pragma once

constexpr int KZ_SOFTMIN_CHUNK = 4096;   // index rows per workgroup of the first level: 16 loads of 8 bytes per thread, all in flight
static_assert(KZ_SOFTMIN_CHUNK == KZ_SOFTMIN_CHUNK_ROWS, "include/kiez_amd.h documents the chunk size");

// level 2 (kz_softmin.hip): out[out0 + b] of the rows b < nb from part [nb][n_chunks], on `stream`
void kz_softmin_fold_launch(hipStream_t stream, const KzSoftminPart* part, int n_chunks, int nb, double eps, double shift, double* out);

// Level 1.  vals [nb][n_i]: the value matrix of the batch.  Workgroup (c, b) owns the index rows [c KZ_SOFTMIN_CHUNK, (c + 1)
// KZ_SOFTMIN_CHUNK) of row b and writes (m, s) of x_j = d_bj - off[j] over them to part[b n_chunks + c].  Places past index.n hold
// +inf: they add exact zeros, the tree stays that of a full chunk.  off (HAS_OFF) is [n_i], read again by every row of the batch: L2
// hits beside the 8 bytes per value that stream from HBM.
template <typename T, int METRIC, bool HAS_OFF>
__global__ __launch_bounds__(256) void kz_softmin_chunk_kernel(const double* __restrict__ vals, int64_t n_i, int n_chunks, double mp, double eps,
                                                               const double* __restrict__ off, KzSoftminPart* __restrict__ part) {
    constexpr int U = KZ_SOFTMIN_CHUNK / 256;   // values per thread
    __shared__ double s_m[4], s_s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, b = blockIdx.y;
    const int64_t j0 = (int64_t)c * KZ_SOFTMIN_CHUNK;
    const double* __restrict__ row = vals + (int64_t)b * n_i;
    double v[U], o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {   // (all loads first: 16, or 32 with offsets, in flight per thread)
        const int64_t j = j0 + 256 * u + tid;
        const bool in = j < n_i;
        v[u] = in ? row[j] : 0.0;
        o[u] = HAS_OFF && in ? off[j] : 0.0;
    }
    // (the conversion in a loop of its own: with Minkowski's pow in the same unrolled body as the selects below, the compiler's
    //  optimiser does not come back from this kernel)
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = kz_output_distance<T>(v[u], METRIC, mp);
    double x[U];
    double m = INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + 256 * u + tid;
        double xu = v[u];
        if (HAS_OFF) xu = xu - o[u];
        xu = j < n_i && xu == xu ? xu : INFINITY;   // (NaN and the places past the row's end: +inf)
        x[u] = xu;
        m = xu < m ? xu : m;
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const double t = __shfl_xor(m, sh, 64);
        m = t < m ? t : m;
    }
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    {
        const double m01 = s_m[1] < s_m[0] ? s_m[1] : s_m[0], m23 = s_m[3] < s_m[2] ? s_m[3] : s_m[2];
        m = m23 < m01 ? m23 : m01;
    }
    KzSoftminPart* out = part + (int64_t)b * n_chunks + c;
    if (m == INFINITY || m == -INFINITY) {   // (uniform)
        if (tid == 0) *out = KzSoftminPart{m, m < 0.0 ? 1.0 : 0.0};
        return;
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) s += exp(-((x[u] - m) / eps));
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) s_s[wave] = s;
    __syncthreads();
    if (tid == 0) *out = KzSoftminPart{m, (s_s[0] + s_s[1]) + (s_s[2] + s_s[3])};
}

extern "C" int kz_softmin_rows(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c, double eps,
                               const double* d_off, double shift, double* d_out) {
    // (the matrices are logically const for the caller: cosine attaches the lazily built normalised rows to the index, as kz_knn does)
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair("kz_softmin_rows", ctx, query, q_begin, q_count, index, d_out, d_out);
    if (rcp != KZ_OK) return rcp;
    KZ_REQUIRE(eps > 0.0 && eps < INFINITY, "kz_softmin_rows: the temperature eps must be finite and > 0, got %g", eps);
    // (a NaN shift would make every result NaN, a -inf one the +inf of a row without a finite entry)
    KZ_REQUIRE(shift > -INFINITY && shift < INFINITY, "kz_softmin_rows: shift must be finite, got %g", shift);
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "kz_softmin_rows: more than 2^31 - 1 rows");
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    // (released when the function returns, stream-ordered: part, fl)
    KzPoolBuf<int> fl;   // every row of the range, as the row list the exact stage takes
    KzPoolBuf<KzSoftminPart> part;
    int rc = fl.alloc(ctx, (size_t)q_count * sizeof(int));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((q_count + 255) / 256)), dim3(256), 0, ctx->stream, fl.get(), (int)q_count);
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_begin(ctx, index, (int)q_count, &batch, &vals);
    if (rc != KZ_OK) return rc;
    const int n_chunks = (int)((index->n + KZ_SOFTMIN_CHUNK - 1) / KZ_SOFTMIN_CHUNK);
    rc = part.alloc(ctx, (size_t)batch * n_chunks * sizeof(KzSoftminPart));
    if (rc != KZ_OK) return rc;
    const int* list = fl.get();
    KzSoftminPart* pt = part.get();
    // A launch that fails is named here, by its batch: the walk's own check would report it as a failure of the exact kernels.
    hipError_t launch_err = hipSuccess;
    int launch_b0 = 0;
    // (the buffers go back to the pool behind the walk's synchronise; the caller reads d_out next)
    rc = kz_exact_walk("kz_softmin_rows", ctx, list, (int)q_count, batch, vals, q_begin, query, index, [&](int b0, int nb) {
        kz_rank_dispatch_distance(index, [&](auto t, auto metric) {
            using T = typename decltype(t)::type;
            constexpr int METRIC = decltype(metric)::value;
            const dim3 grid(n_chunks, nb);
            if (d_off)
                hipLaunchKernelGGL((kz_softmin_chunk_kernel<T, METRIC, true>), grid, dim3(256), 0, ctx->stream, (const double*)vals, index->n, n_chunks,
                                   index->mink_p, eps, d_off, pt);
            else
                hipLaunchKernelGGL((kz_softmin_chunk_kernel<T, METRIC, false>), grid, dim3(256), 0, ctx->stream, (const double*)vals, index->n,
                                   n_chunks, index->mink_p, eps, d_off, pt);
        });
        kz_softmin_fold_launch(ctx->stream, pt, n_chunks, nb, eps, shift, d_out + b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess && launch_err == hipSuccess) {
            launch_err = e;
            launch_b0 = b0;
        }
    });
    if (launch_err != hipSuccess) {
        kz_set_error("kz_softmin_rows: a kernel of the batch at row %d failed to launch: %s", launch_b0, hipGetErrorString(launch_err));
        return KZ_ERR_HIP;
    }
    return rc;
}
