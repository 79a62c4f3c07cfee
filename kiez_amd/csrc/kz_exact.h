// Stage 3 of kz_knn (kz_knn.hip): the EXACT FLOAT64 STAGE -- the distance kernels that answer a batch of query rows against the whole
// index, the selection kernels, and the one host path through them.  Three callers: the fallback of kz_knn_impl
// (kz_exact_whole_index), the speculative rescue (kz_spec_rescue) and the whole-index entry points kz_gold_ranks / kz_knn_reduced
// (kz_exact_walk: kz_exact_distances per batch, then their own count or selection).
// They run the same rule with different launch geometry: what differs is spelled out in KzExactLaunch, nowhere else.
// (kz_range.h launches some of these kernels on gathered segments and representative rows by rules of its own.)
#pragma once

// ---------------------------------------------------------------------------------------------------
// Stage 3: exact float64 brute force for uncertified rows (rare; correctness backstop)
// ---------------------------------------------------------------------------------------------------
// SPECULATIVE launches of the exact kernels (kz_spec_rescue below): the grid is sized for `cap` rows BEFORE the host knows how
// many rows the finalize kernel left uncertified; the count is read from device memory, row b of the grid lives when
// b < count <= cap (count > cap: nothing runs here, the host takes the ordinary re-search).
__device__ __forceinline__ bool kz_spec_row_live(const int* __restrict__ dyn_n, int b, int cap) {
    const int n = *dyn_n;
    return n <= cap && b < n;
}

template <typename T>
__global__ __launch_bounds__(256) void kz_exact_dist_kernel(const int* __restrict__ fail_list, int batch0, int64_t q_begin,
                                                            const T* __restrict__ qraw, const T* __restrict__ yraw,
                                                            const double* __restrict__ qsqn, const double* __restrict__ ysqn,
                                                            int64_t n_i, int d, int metric, double p, double* __restrict__ vals,
                                                            const int* __restrict__ dyn_n = nullptr) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    if (dyn_n && !kz_spec_row_live(dyn_n, b, (int)gridDim.y)) return;
    const int64_t qrow = q_begin + fail_list[batch0 + b];
    // (grid-stride over the index rows: the ordinary callers launch one wave per pair, a speculative launch a bounded grid --
    //  workgroups of a dead row cost their dispatch, and n_i / 4 x R of them would be milliseconds on a 1 M-row index)
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_i; i += (int64_t)gridDim.x * 4) {
        const double v = kz_exact_value<T>(qraw + qrow * (int64_t)d, yraw + i * (int64_t)d, qsqn[qrow], ysqn[i], d, metric, lane, p);
        if (lane == 0) vals[(int64_t)b * n_i + i] = v;
    }
}

// The same values for float32 rows of d <= 256 (d a multiple of 4), many pairs per wave step (round 5).  kz_exact_dist_kernel spends
// a wave on ONE pair -- at d = 64 a quarter of its lanes, re-reading the query row and, for cosine, dividing every element twice:
// 2.9 G pairs/s, 125 us per query row against 301 k index rows; on data with clusters three orders of magnitude tighter than the
// data's extent a tenth of the rows end there, and a 300 k x 300 k call took 8 s (tools/cliff_probe.py).  Here a wave keeps Q = 4
// query rows in registers and walks CONSECUTIVE index rows, G = 64 / LPR of them per step (a row needs LPR = d / 4 lanes rounded up
// to a power of two): one coalesced load serves G x Q pairs.  The arithmetic of a pair is kz_wave_dot's, operation for operation
// -- the lane's four fma in element order, then the butterfly inside the lane group (the steps of the full-wave butterfly that it
// skips add the exact zeros of lanes past the row) -- as in the finalize kernel for many candidates (kz_knn_fin_wide.h), so the
// values are bit for bit those of kz_exact_value, kz_pair_values and the re-rank.  Cosine: the index rows normalised once in
// float64 (kz_matrix_norm64) where that image exists, else the shared-reciprocal division.
template <int LPR, bool NORM, int NV = 1>
__global__ __launch_bounds__(256) void kz_exact_dist_rows_kernel(const int* __restrict__ fail_list, int batch0, int nb, int64_t q_begin,
                                                                 const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                                 const double* __restrict__ ynorm64, const double* __restrict__ qsqn,
                                                                 const double* __restrict__ ysqn, int64_t n_i, int d, int metric,
                                                                 int rows_per_wave, double* __restrict__ vals,
                                                                 const int* __restrict__ dyn_n = nullptr) {
    // NV = 2 (round 6): rows of 260 .. 512 elements -- a lane owns elements 4 sl .. 4 sl + 3 of BOTH 256-element chunks of the row
    // (LPR = 64, one index row per wave step), the second chunk's four fma continue the first's chain: kz_wave_dot's order for d > 256.
    static_assert(NV == 1 || LPR == 64, "two chunks per lane: the whole wave owns one row");
    constexpr int G = 64 / LPR, Q = 4;
    if (dyn_n) {   // (speculative launch: nb was the grid's capacity)
        if (!kz_spec_row_live(dyn_n, blockIdx.y * Q, nb)) return;
        nb = *dyn_n;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / LPR, sl = lane & (LPR - 1);
    const int k0 = 4 * sl;
    bool act[NV];
    int k0r[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        act[c] = k0 + 256 * c < d;
        k0r[c] = act[c] ? k0 + 256 * c : 0;
    }
    const int b0 = blockIdx.y * Q;
    double qk[Q][4 * NV], qs[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int bq = b0 + j < nb ? b0 + j : nb - 1;
        const int64_t qrow = q_begin + fail_list[batch0 + bq];
        qs[j] = qsqn[qrow];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            double t[4] = {0.0, 0.0, 0.0, 0.0};
            if (act[c]) {
                kz_row4(qraw + qrow * (int64_t)d, k0r[c], d, true, t);
                if (metric == KZ_COSINE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = t[e] / qs[j];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) qk[j][4 * c + e] = t[e];
        }
    }
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave;
    const int64_t i1 = i0 + rows_per_wave < n_i ? i0 + rows_per_wave : n_i;
    if (i0 >= i1) return;
    struct Buf {
        float4 f[NV];
        double ys;
        double2 n0[NV], n1[NV];
    };
    auto issue = [&](int64_t i, Buf& b) {   // (rows past the end: the last row again, nothing is written for them)
        const int64_t yi = i + grp < i1 ? i + grp : i1 - 1;
        if (NORM) {
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const double* row = ynorm64 + yi * (int64_t)d + k0r[c];
                b.n0[c] = *reinterpret_cast<const double2*>(row);
                b.n1[c] = *reinterpret_cast<const double2*>(row + 2);
            }
        } else {
            b.ys = ysqn[yi];
#pragma unroll
            for (int c = 0; c < NV; ++c) b.f[c] = *reinterpret_cast<const float4*>(yraw + yi * (int64_t)d + k0r[c]);
        }
    };
    auto reduce = [&](int64_t i, const Buf& b) {
        double yv[4 * NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[4 * c + e] = 0.0;
            if (act[c]) {
                if (NORM) {
                    yv[4 * c] = b.n0[c].x, yv[4 * c + 1] = b.n0[c].y, yv[4 * c + 2] = b.n1[c].x, yv[4 * c + 3] = b.n1[c].y;
                } else {
                    const double yk[4] = {(double)b.f[c].x, (double)b.f[c].y, (double)b.f[c].z, (double)b.f[c].w};
                    if (metric == KZ_COSINE) {
                        const double rcp = 1.0 / b.ys;
                        const bool fin = (((unsigned long long)__double_as_longlong(rcp) >> 52) & 0x7ff) != 0x7ff;
#pragma unroll
                        for (int e = 0; e < 4; ++e) yv[4 * c + e] = fin ? kz_div_shared(yk[e], b.ys, rcp) : yk[e] / b.ys;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) yv[4 * c + e] = yk[e];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            double a = 0.0;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                if (act[c]) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) a = fma(qk[j][4 * c + e], yv[4 * c + e], a);
                }
            }
#pragma unroll
            for (int off = LPR >> 1; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
            double v;
            if (metric == KZ_COSINE)
                v = fmin(fmax(1.0 - a, 0.0), 2.0);
            else
                v = fmax((qs[j] + b.ys) - 2.0 * a, 0.0);
            if (sl == 0 && i + grp < i1 && b0 + j < nb) vals[(int64_t)(b0 + j) * n_i + i + grp] = v;
        }
    };
    Buf ba, bb;
    issue(i0, ba);
    for (int64_t i = i0; i < i1;) {   // (two steps in flight; the conditions are wave-uniform)
        issue(i + G, bb);
        reduce(i, ba);
        i += G;
        if (i >= i1) break;
        issue(i + G, ba);
        reduce(i, bb);
        i += G;
    }
}
// -> true when the kernel above took the batch
static bool kz_launch_exact_rows(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t cq_begin, const kz_matrix* query, const kz_matrix* index,
                                 int metric, double* vals, const int* dyn_n = nullptr, int rows_per_wave = 256) {
    const int d = (int)index->d;
    if (index->dtype != KZ_F32 || (d & 3) != 0 || d > 512 || metric > KZ_COSINE || (((uintptr_t)query->raw | (uintptr_t)index->raw) & 15u) != 0) return false;
    const bool norm = metric == KZ_COSINE && index->norm64 != nullptr;
    const dim3 grid((unsigned)((index->n + 4 * rows_per_wave - 1) / (4 * rows_per_wave)), (unsigned)((nb + 3) / 4));
    const int lanes = (d + 3) >> 2;
#define KZ_EXACT_ROWS(L)                                                                                                                \
    do {                                                                                                                                \
        if (norm)                                                                                                                       \
            hipLaunchKernelGGL((kz_exact_dist_rows_kernel<L, true>), grid, dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin,          \
                               (const float*)query->raw, (const float*)index->raw, index->norm64, query->sqn, index->sqn, index->n, d, \
                               metric, rows_per_wave, vals, dyn_n);                                                                     \
        else                                                                                                                            \
            hipLaunchKernelGGL((kz_exact_dist_rows_kernel<L, false>), grid, dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin,         \
                               (const float*)query->raw, (const float*)index->raw, (const double*)nullptr, query->sqn, index->sqn,      \
                               index->n, d, metric, rows_per_wave, vals, dyn_n);                                                        \
    } while (0)
    if (lanes <= 8)
        KZ_EXACT_ROWS(8);
    else if (lanes <= 16)
        KZ_EXACT_ROWS(16);
    else if (lanes <= 32)
        KZ_EXACT_ROWS(32);
    else if (lanes <= 64)
        KZ_EXACT_ROWS(64);
    else if (norm)   // (260 .. 512 elements: two chunks per lane)
        hipLaunchKernelGGL((kz_exact_dist_rows_kernel<64, true, 2>), grid, dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin, (const float*)query->raw,
                           (const float*)index->raw, index->norm64, query->sqn, index->sqn, index->n, d, metric, rows_per_wave, vals, dyn_n);
    else
        hipLaunchKernelGGL((kz_exact_dist_rows_kernel<64, false, 2>), grid, dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin, (const float*)query->raw,
                           (const float*)index->raw, (const double*)nullptr, query->sqn, index->sqn, index->n, d, metric, rows_per_wave, vals, dyn_n);
#undef KZ_EXACT_ROWS
    return true;
}

#include "kz_exact_lanes.h"
// -> true when the one-pair-per-lane kernel (kz_exact_lanes.h) took the batch: float32 rows of up to 512 elements (a multiple of 4,
// 16-byte aligned), the euclidean family on the raw rows, cosine on the normalised float64 rows where that image exists, and a
// batch of at least KZ_XL_MIN_ROWS query rows (a handful is the cooperative kernel's: it needs no staging and no pre-pass).
constexpr int KZ_XL_MIN_ROWS = 32;
static inline size_t kz_exact_lanes_qd_bytes(int nb, int d) {   // float64 operand rows + squared norms of whole blocks of query rows
    const size_t nb_pad = (size_t)(nb + 4 * KZ_XL_Q - 1) / (4 * KZ_XL_Q) * (4 * KZ_XL_Q);
    return (nb_pad * (size_t)d + nb_pad) * 8;
}
// dyn_n (speculative launch): nb is the capacity of the launch, the row count is read on the device
// groups != nullptr (kz_range.h, grouped ranges): ONE launch for n_groups dense blocks (KzXlGroup) -- fl [n_slots] then holds the
// query row of every operand row of every block (-1: padding), gather the blocks' lists of index rows; nb = n_slots, rows_max /
// q_max = the largest block's index rows / query rows; vals as the blocks' val_off say.
static int kz_launch_exact_lanes(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t cq_begin, const kz_matrix* query, const kz_matrix* index,
                                 int metric, double* vals, bool* took, const int* dyn_n = nullptr, double* qd_buf = nullptr,
                                 const int* gather = nullptr, const KzXlGroup* groups = nullptr, int n_groups = 0, int rows_max = 0,
                                 int q_max = 0) {
    *took = false;
    const int d = (int)index->d;
    if (ctx->exact_rows < 2 || (nb < KZ_XL_MIN_ROWS && !dyn_n) || index->dtype != KZ_F32 || (d & 3) != 0 || d > 512 || metric > KZ_COSINE ||
        (((uintptr_t)query->raw | (uintptr_t)index->raw) & 15u) != 0)
        return KZ_OK;
    const bool cosine = metric == KZ_COSINE && index->norm64 != nullptr && d <= 256;   // (the normalised float64 rows, staged as they are)
    const bool cos_raw = metric == KZ_COSINE && !cosine;                               // (the raw rows, divided by the lane)
    const int d_pad = d;   // (a multiple of 4: whole leaves)
    const int nb_pad = groups ? nb : (nb + 4 * KZ_XL_Q - 1) / (4 * KZ_XL_Q) * (4 * KZ_XL_Q);   // (whole blocks of 4 waves x KZ_XL_Q rows; groups: the slots are padded per block)
    double* qd = qd_buf;   // (a caller that runs these launches on another stream than the pool's brings the buffer: kz_spec_alloc)
    KzPoolBuf<double> qd_own;
    if (!qd) {
        const int rc = qd_own.alloc(ctx, kz_exact_lanes_qd_bytes(nb, d));
        if (rc != KZ_OK) return rc == KZ_ERR_NOMEM ? KZ_OK : rc;   // (no memory for the operand rows: the cooperative kernel)
        qd = qd_own.get();
    }
    double* qsq = qd + (size_t)nb_pad * d_pad;
    if (groups)
        hipLaunchKernelGGL(kz_exact_qprep_slots_kernel, dim3(nb_pad), dim3(256), 0, ctx->stream, fl, cq_begin, (const float*)query->raw, query->sqn, d,
                           d_pad, metric, qd, qsq);
    else
        hipLaunchKernelGGL(kz_exact_qprep_kernel, dim3(nb_pad), dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin, (const float*)query->raw, query->sqn, d,
                           d_pad, metric, qd, qsq, dyn_n);
    const int64_t n_rows = groups ? rows_max : index->n;
    // (groups: a workgroup takes q_chunk = 64 query rows of its block -- four rounds of its 16 -- for one tile of 64 index rows)
    const int q_chunk = 16 * KZ_XL_Q;
    const dim3 grid((unsigned)((n_rows + KZ_XL_ROWS - 1) / KZ_XL_ROWS), groups ? (unsigned)((q_max + q_chunk - 1) / q_chunk) : 1u,
                    groups ? (unsigned)n_groups : 1u);
    const size_t lds = (size_t)(d_pad / 4) * (KZ_XL_ROWS + 1) * (cosine ? 32 : 16);   // (<= 133 KiB: 512 float32 / 256 float64 elements)
    hipError_t e = hipSuccess;
#define KZ_XL_LAUNCH_G(NL, NVV, ELT, CR, GA, rows)                                                                                             \
    do {                                                                                                                                        \
        if (lds > 65536) e = hipFuncSetAttribute((const void*)kz_exact_dist_lanes_kernel<NL, NVV, ELT, CR, GA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e == hipSuccess)                                                                                                                     \
            hipLaunchKernelGGL((kz_exact_dist_lanes_kernel<NL, NVV, ELT, CR, GA>), grid, dim3(256), lds, ctx->stream, nb, (const double*)qd, (const double*)qsq, \
                               (const ELT*)(rows), index->sqn, n_rows, d, d_pad, metric, vals, dyn_n, gather, groups, q_chunk);                 \
    } while (0)
#define KZ_XL_LAUNCH(NL, NVV, ELT, rows)                          \
    do {                                                           \
        if (groups)                                                \
            KZ_XL_LAUNCH_G(NL, NVV, ELT, false, true, rows);       \
        else                                                       \
            KZ_XL_LAUNCH_G(NL, NVV, ELT, false, false, rows);      \
    } while (0)
    if (cos_raw) {
#define KZ_XL_LAUNCH_COS(NL, NVV)                                        \
    do {                                                                  \
        if (groups)                                                       \
            KZ_XL_LAUNCH_G(NL, NVV, float, true, true, index->raw);       \
        else                                                              \
            KZ_XL_LAUNCH_G(NL, NVV, float, true, false, index->raw);      \
    } while (0)
        if (d <= 64)
            KZ_XL_LAUNCH_COS(16, 1);
        else if (d <= 128)
            KZ_XL_LAUNCH_COS(32, 1);
        else if (d <= 256)
            KZ_XL_LAUNCH_COS(64, 1);
        else
            KZ_XL_LAUNCH_COS(64, 2);
#undef KZ_XL_LAUNCH_COS
    } else if (cosine) {
        if (d <= 64)
            KZ_XL_LAUNCH(16, 1, double, index->norm64);
        else if (d <= 128)
            KZ_XL_LAUNCH(32, 1, double, index->norm64);
        else
            KZ_XL_LAUNCH(64, 1, double, index->norm64);
    } else {
        if (d <= 64)
            KZ_XL_LAUNCH(16, 1, float, index->raw);
        else if (d <= 128)
            KZ_XL_LAUNCH(32, 1, float, index->raw);
        else if (d <= 256)
            KZ_XL_LAUNCH(64, 1, float, index->raw);
        else
            KZ_XL_LAUNCH(64, 2, float, index->raw);
    }
#undef KZ_XL_LAUNCH
#undef KZ_XL_LAUNCH_G
    if (e == hipSuccess) e = hipGetLastError();
    qd_own.reset();   // (stream-ordered pool)
    if (e != hipSuccess) {
        kz_set_error("kz_knn: exact distance kernel (one pair per lane) failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    *took = true;
    return KZ_OK;
}

// The Minkowski family beyond p = 2 (KZ_MANHATTAN, KZ_CHEBYSHEV, KZ_MINKOWSKI): no inner-product form, hence no MFMA -- a
// register-tiled VALU kernel.  A workgroup of 256 threads owns 64 queries x 64 index rows, a thread 4 x 4 pairs; the rows are
// staged through LDS DK features at a time, transposed ([feature][row]: a thread reads its four query values and its four index
// values of a feature as one 16- / 32-byte LDS read each).  Per pair and feature: subtract in the input dtype, |.| into float64
// (the conversion carries the abs modifier), add -- three VALU operations; every thread adds the terms of its pairs in feature
// order (kz_common.h: kz_family_term / kz_family_add), which is scikit-learn's order.  VALU-bound: 15 k x 15 k x 300 float32,
// manhattan: see DESIGN section 9.  Output: the same [batch][n_i] float64 value matrix kz_exact_dist_kernel writes.
// Metrics 6 .. 9 (braycurtis, seuclidean, correlation, hamming: kz_common.h, kz_family_step) run on the same tiles: a pair's
// state is two float64 accumulators.  Seuclidean reads V_j at a wave-uniform address; correlation stages the CENTRED float64 values
// (x - row mean, one subtraction per element as the tile is loaded, not per pair), features [0, d & ~1) go through the tiles in
// even / odd pairs and the odd tail term is added at the end.
template <typename T, int METRIC, int DK, int CHAIN>
__global__ __launch_bounds__(256) void kz_family_dist_kernel(const int* __restrict__ fail_list, int batch0, int nb, int64_t q_begin,
                                                             const T* __restrict__ qraw, const T* __restrict__ yraw, int64_t n_i, int d,
                                                             double p, int p_int, double* __restrict__ vals,
                                                             const double* __restrict__ V = nullptr, const double* __restrict__ qcorr = nullptr,
                                                             const double* __restrict__ ycorr = nullptr) {
    using S = typename std::conditional<METRIC == KZ_CORRELATION, double, T>::type;   // (staged type)
    __shared__ __attribute__((aligned(32))) S sQ[DK][64];
    __shared__ __attribute__((aligned(32))) S sY[DK][64];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t y0 = (int64_t)blockIdx.x * 64;
    const int b0 = blockIdx.y * 64;
    // staging: thread t copies DK / 4 consecutive features of row (t & 63) of both tiles (rows past the end: the last row again)
    const int lrow = t & 63, lseg = (t >> 6) * (DK / 4);
    const int bq = b0 + lrow < nb ? b0 + lrow : nb - 1;
    const int64_t qrow_l = q_begin + fail_list[batch0 + bq];
    const int64_t yrow_l = y0 + lrow < n_i ? y0 + lrow : n_i - 1;
    const T* __restrict__ qp = qraw + qrow_l * (int64_t)d;
    const T* __restrict__ yp = yraw + yrow_l * (int64_t)d;
    // correlation: the features the tiles cover (the odd tail is added at the end) and the staged rows' means
    const int d_tiles = METRIC == KZ_CORRELATION ? (d & ~1) : d;
    double mq = 0.0, my = 0.0;
    if constexpr (METRIC == KZ_CORRELATION) {
        mq = qcorr[2 * qrow_l];
        my = ycorr[2 * yrow_l];
    }
    double acc[4][4], acc2[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = acc2[a][c] = 0.0;
    for (int k0 = 0; k0 < d_tiles; k0 += DK) {
        S rq[DK / 4], ry[DK / 4];
#pragma unroll
        for (int u = 0; u < DK / 4; ++u) {
            const int k = k0 + lseg + u;
            if constexpr (METRIC == KZ_CORRELATION) {
                rq[u] = k < d_tiles ? (double)qp[k] - mq : 0.0;   // (0 x 0 adds +0: changes no sum)
                ry[u] = k < d_tiles ? (double)yp[k] - my : 0.0;
            } else {
                rq[u] = k < d ? qp[k] : (T)0;
                ry[u] = k < d ? yp[k] : (T)0;   // (|0 - 0| = 0 changes no sum and no maximum; nor 0 != 0, nor 0 0 / 1)
            }
        }
        __syncthreads();   // (the previous chunk has been read)
#pragma unroll
        for (int u = 0; u < DK / 4; ++u) {
            sQ[lseg + u][lrow] = rq[u];
            sY[lseg + u][lrow] = ry[u];
        }
        __syncthreads();
        if constexpr (METRIC == KZ_CORRELATION) {
            // (fully unrolled: the parity of a feature -- which partial sum it goes to -- is known at compile time)
#pragma unroll
            for (int j = 0; j < DK; ++j) {
                S q4[4], y4[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    q4[a] = sQ[j][ty * 4 + a];
                    y4[a] = sY[j][tx * 4 + a];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c) kz_family_step<T, METRIC, CHAIN>(acc[a][c], acc2[a][c], q4[a], y4[c], p, p_int, 1.0, (j & 1) != 0);
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < DK; ++j) {
                // (seuclidean: a wave-uniform read of V_j; past the end 1: the padded term is 0 / 1)
                const double v_j = METRIC == KZ_SEUCLIDEAN ? (k0 + j < d ? V[k0 + j] : 1.0) : 1.0;
                S q4[4], y4[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    q4[a] = sQ[j][ty * 4 + a];
                    y4[a] = sY[j][tx * 4 + a];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c) kz_family_step<T, METRIC, CHAIN>(acc[a][c], acc2[a][c], q4[a], y4[c], p, p_int, v_j, false);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int b = b0 + ty * 4 + a;
        if (b >= nb) continue;
        double nq = 0.0, tq = 0.0;
        const T* qrow = nullptr;
        if constexpr (METRIC == KZ_CORRELATION) {
            const int64_t qr = q_begin + fail_list[batch0 + b];
            nq = qcorr[2 * qr + 1];
            qrow = qraw + qr * (int64_t)d;
            if (d & 1) tq = (double)qrow[d - 1] - qcorr[2 * qr];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t i = y0 + tx * 4 + c;
            if (i >= n_i) continue;
            double ny = 0.0, tail = 0.0;
            if constexpr (METRIC == KZ_CORRELATION) {
                ny = ycorr[2 * i + 1];
                if (d & 1) tail = tq * ((double)yraw[i * (int64_t)d + d - 1] - ycorr[2 * i]);
            }
            vals[(int64_t)b * n_i + i] = kz_family_finish<T, METRIC>(acc[a][c], acc2[a][c], d, tail, nq, ny);
        }
    }
}
template <typename T>
static void kz_launch_family_dist(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t cq_begin, const kz_matrix* query, const kz_matrix* index,
                                  double* vals) {
    constexpr int DK = kz_f32_rows<T> ? 32 : 16;
    const dim3 grid((unsigned)((index->n + 63) / 64), (unsigned)((nb + 63) / 64));
    const int p_int = kz_family_p_int(index->metric, index->mink_p, kz_f32_rows<T>);
#define KZ_FAMILY_LAUNCH_DK(M, C, DKM)                                                                                                    \
    hipLaunchKernelGGL((kz_family_dist_kernel<T, M, DKM, C>), grid, dim3(256), 0, ctx->stream, fl, b0, nb, cq_begin, (const T*)query->raw, \
                       (const T*)index->raw, index->n, (int)index->d, index->mink_p, p_int, vals, index->seu_v, query->corr, index->corr)
#define KZ_FAMILY_LAUNCH(M, C) KZ_FAMILY_LAUNCH_DK(M, C, DK)
    if (index->metric == KZ_MANHATTAN)
        KZ_FAMILY_LAUNCH(KZ_MANHATTAN, -1);
    else if (index->metric == KZ_CHEBYSHEV)
        KZ_FAMILY_LAUNCH(KZ_CHEBYSHEV, -1);
    else if (index->metric == KZ_BRAYCURTIS)
        KZ_FAMILY_LAUNCH(KZ_BRAYCURTIS, -1);
    else if (index->metric == KZ_SEUCLIDEAN)
        KZ_FAMILY_LAUNCH(KZ_SEUCLIDEAN, -1);
    else if (index->metric == KZ_CORRELATION)
        KZ_FAMILY_LAUNCH_DK(KZ_CORRELATION, -1, 16);   // (float64 tiles whatever the input dtype)
    else if (index->metric == KZ_HAMMING)
        KZ_FAMILY_LAUNCH(KZ_HAMMING, -1);
    else if (p_int == 3)
        KZ_FAMILY_LAUNCH(KZ_MINKOWSKI, 3);     // (float32 inputs, p = 3 or 4: a product with one rounding, no pow() in the kernel)
    else if (p_int == 4)
        KZ_FAMILY_LAUNCH(KZ_MINKOWSKI, 4);
    else
        KZ_FAMILY_LAUNCH(KZ_MINKOWSKI, -1);
#undef KZ_FAMILY_LAUNCH
#undef KZ_FAMILY_LAUNCH_DK
}

// First level of the exact selection on a long row: the k_eff smallest (value, index row) pairs of every CHUNK of KZ_EXACT_CHUNK
// values (the smallest k_eff of the row are among the smallest k_eff of their chunks); kz_exact_select_kernel then picks from
// n_chunks x k_eff survivors instead of passing k_eff times over the whole row with one workgroup (1 M index rows, k = 10: 2 ms
// per query row before, the distance kernel's time now).  One workgroup per (chunk, query row); a thread holds 16 values.
constexpr int KZ_EXACT_CHUNK = 4096;
__global__ __launch_bounds__(256) void kz_exact_chunk_kernel(const double* __restrict__ vals, int64_t n_i, int k_eff, int n_chunks,
                                                             double* __restrict__ cand_v, int* __restrict__ cand_i,
                                                             const int* __restrict__ dyn_n = nullptr) {
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, b = blockIdx.y;
    if (dyn_n && !kz_spec_row_live(dyn_n, b, (int)gridDim.y)) return;
    const double* v = vals + (int64_t)b * n_i;
    const int64_t i0 = (int64_t)c * KZ_EXACT_CHUNK;
    constexpr int PER = KZ_EXACT_CHUNK / 256;
    double x[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int64_t i = i0 + tid + 256 * u;
        x[u] = i < n_i ? v[i] : INFINITY;
    }
    double* ov = cand_v + ((int64_t)b * n_chunks + c) * k_eff;
    int* oi = cand_i + ((int64_t)b * n_chunks + c) * k_eff;
    double pv = -1.0;  // values are >= 0
    int pi = -1;
    for (int r = 0; r < k_eff; ++r) {
        double bv = INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int64_t i = i0 + tid + 256 * u;
            const int id = i < n_i ? (int)i : 0x7fffffff;   // (places past the end of the row: (+inf, INT_MAX), after every real entry)
            const bool after = (x[u] > pv) || (x[u] == pv && id > pi);
            if (after && (x[u] < bv || (x[u] == bv && id < bi))) {
                bv = x[u];
                bi = id;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double o_v = __shfl_xor(bv, off, 64);
            const int o_i = __shfl_xor(bi, off, 64);
            if (o_v < bv || (o_v == bv && o_i < bi)) {
                bv = o_v;
                bi = o_i;
            }
        }
        if (lane == 0) {
            s_v[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
        for (int ww = 1; ww < 4; ++ww) {
            if (s_v[ww] < bv || (s_v[ww] == bv && s_i[ww] < bi)) {
                bv = s_v[ww];
                bi = s_i[ww];
            }
        }
        if (tid == 0) {
            ov[r] = bv;
            oi[r] = bi;
        }
        pv = bv;
        pi = bi;
        __syncthreads();
    }
}

// The same first level for MANY neighbours (k_eff >= 24): the k_eff-th smallest value of the chunk by a workgroup-wide radix
// selection on the float64 bit patterns (non-negative doubles order like their patterns; a thread holds 16 of them, a counting pass
// is 16 compares, a wave sum and one exchange through LDS -- ~55 passes below the common prefix whatever k is, against k_eff rounds
// of a workgroup-wide arg-min: k = 50: 0.96 -> see r05_notes), then everything below it and, of the entries equal to it, those with
// the smallest index rows.  The survivors come out in no particular order: kz_exact_select_kernel orders by (value, index row).
__global__ __launch_bounds__(256) void kz_exact_chunk_radix_kernel(const double* __restrict__ vals, int64_t n_i, int k_eff, int n_chunks,
                                                                   double* __restrict__ cand_v, int* __restrict__ cand_i,
                                                                   const int* __restrict__ dyn_n = nullptr) {
    __shared__ unsigned long long s_or[4], s_and[4];
    __shared__ int s_cnt[4];
    __shared__ int s_pos;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, b = blockIdx.y;
    if (dyn_n && !kz_spec_row_live(dyn_n, b, (int)gridDim.y)) return;
    const double* v = vals + (int64_t)b * n_i;
    const int64_t i0 = (int64_t)c * KZ_EXACT_CHUNK;
    constexpr int PER = KZ_EXACT_CHUNK / 256;
    const int nvalid = (int)(n_i - i0 < KZ_EXACT_CHUNK ? n_i - i0 : KZ_EXACT_CHUNK);
    double* ov = cand_v + ((int64_t)b * n_chunks + c) * k_eff;
    int* oi = cand_i + ((int64_t)b * n_chunks + c) * k_eff;
    unsigned long long x[PER];
    unsigned long long all_or = 0ull, all_and = ~0ull;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = tid + 256 * u;
        const bool in = e < nvalid;
        x[u] = in ? (unsigned long long)__double_as_longlong(v[i0 + e]) : ~0ull;   // (places past the end: above every value)
        all_or |= in ? x[u] : 0ull;
        all_and &= x[u];
    }
    if (nvalid <= k_eff) {   // (a short last chunk: every entry survives; the unused places hold (+inf, INT_MAX))
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u;
            if (e < nvalid) {
                ov[e] = __longlong_as_double((long long)x[u]);
                oi[e] = (int)(i0 + e);
            }
        }
        for (int e = nvalid + tid; e < k_eff; e += 256) {
            ov[e] = INFINITY;
            oi[e] = 0x7fffffff;
        }
        return;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    if (lane == 0) {
        s_or[wave] = all_or;
        s_and[wave] = all_and;
    }
    if (tid == 0) s_pos = 0;
    __syncthreads();
    all_or = s_or[0] | s_or[1] | s_or[2] | s_or[3];
    all_and = s_and[0] & s_and[1] & s_and[2] & s_and[3];
    auto block_sum = [&](int cnt) {   // (every thread gets the workgroup's total)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        __syncthreads();   // (the previous round's readers are done with s_cnt)
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    };
    const unsigned long long differ = all_or ^ all_and;
    const int top = differ ? 63 - __clzll(differ) : -1;
    // thr = the k_eff-th smallest pattern: the largest prefix with fewer than k_eff entries below it, bit by bit
    unsigned long long thr = top >= 63 ? 0ull : (top < 0 ? all_and : (all_and & ~((2ull << top) - 1ull)));
    for (int bit = top; bit >= 0; --bit) {
        const unsigned long long cand = thr | (1ull << bit);
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < PER; ++u) cnt += x[u] < cand ? 1 : 0;
        if (block_sum(cnt) < k_eff) thr = cand;
    }
    // everything below thr
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (x[u] < thr) {
            const int pos = atomicAdd(&s_pos, 1);
            ov[pos] = __longlong_as_double((long long)x[u]);
            oi[pos] = (int)(i0 + tid + 256 * u);
        }
    }
    int ties = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) ties += x[u] == thr ? 1 : 0;
    const int T = block_sum(ties);   // (its barriers also publish s_pos)
    const int L = s_pos;
    const int m = k_eff - L;         // places left for entries equal to thr: 1 <= m <= T
    if (T == m) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (x[u] == thr) {
                const int pos = atomicAdd(&s_pos, 1);
                ov[pos] = __longlong_as_double((long long)thr);
                oi[pos] = (int)(i0 + tid + 256 * u);
            }
        }
        return;
    }
    // more ties at the k_eff-th place than places: those with the smallest index rows, one per round
    int last = -1;
    for (int r = 0; r < m; ++r) {
        int best = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int id = (int)(i0 + tid + 256 * u);
            if (x[u] == thr && id > last && id < best) best = id;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
        __syncthreads();
        if (lane == 0) s_cnt[wave] = best;
        __syncthreads();
        best = min(min(s_cnt[0], s_cnt[1]), min(s_cnt[2], s_cnt[3]));
        if (tid == 0) {
            ov[L + r] = __longlong_as_double((long long)thr);
            oi[L + r] = best;
        }
        last = best;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void kz_exact_select_kernel(const int* __restrict__ fail_list, int batch0, int64_t q_begin,
                                                              const double* __restrict__ vals, const int* __restrict__ cand_idx,
                                                              int64_t n_entries, int64_t n_i, int k,
                                                              int exclude_self, const int64_t* __restrict__ self_ids,
                                                              int metric, double p, double* __restrict__ out_dist,
                                                              int64_t* __restrict__ out_ind, const int* __restrict__ dyn_n = nullptr,
                                                              const long long* __restrict__ seg_off = nullptr, int* __restrict__ left = nullptr,
                                                              int* __restrict__ left_cnt = nullptr, const long long* __restrict__ idx_off = nullptr,
                                                              const int* __restrict__ seg_len = nullptr) {
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    extern __shared__ __attribute__((aligned(16))) char sel_sm[];   // k_eff doubles + k_eff ints (any k the host admits)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    if (dyn_n && !kz_spec_row_live(dyn_n, b, (int)gridDim.x)) return;
    const int q = fail_list[batch0 + b];
    if (q < 0) return;   // (grouped ranges, kz_range.h: a padding slot of a block)
    // the row's values: all n_i of them (cand_idx == nullptr: entry i is index row i), or the survivors of kz_exact_chunk_kernel
    // (n_entries (value, index row) pairs; unused places hold (+inf, INT_MAX) and are never reached: k_eff <= n_i real entries exist)
    const double* v = vals + (int64_t)b * n_entries;
    const int* vid = cand_idx ? cand_idx + (int64_t)b * n_entries : nullptr;
    const int k_eff = (int)min((int64_t)(k + (exclude_self ? 1 : 0)), n_i);
    if (seg_off) {
        // range re-search (kz_range.h): row b's entries are the segment [seg_off[b], seg_off[b + 1]) of vals / cand_idx; a segment
        // with fewer than k entries cannot answer its row -- the row is handed back (left)
        const long long s0 = seg_off[b];
        n_entries = seg_len ? (int64_t)seg_len[b] : seg_off[b + 1] - s0;   // (seg_len: the segments are not adjacent)
        if (n_entries < k_eff) {
            if (tid == 0) left[atomicAdd(left_cnt, 1)] = q;
            return;
        }
        v = vals + s0;
        vid = cand_idx + (idx_off ? idx_off[b] : s0);   // (idx_off: the rows of a group share one list of index rows)
    }
    // LONG SEGMENTS (a group's range: thousands of values per row, kz_range.h): k passes over all of them -- 82 k rows x 10 x 5 000
    // loads, 4 ms of a 79 ms search -- become two.  Pass 1: every thread's smallest value; the k-th smallest T of those 256 minima is
    // at or above the k-th smallest value of the segment.  Pass 2: the entries <= T (all ties included) go to a list in LDS; the k
    // rounds below then run over that list.  The k smallest by (value, row) all lie at or below T: the same selection.  A list
    // that would not fit (values dense at the bottom, duplicates) leaves the segment where it is.
    constexpr int SEL_CAP = 1536;
    __shared__ double c_v[SEL_CAP];
    __shared__ int c_i[SEL_CAP];
    __shared__ double s_min[256];
    __shared__ double s_T;
    __shared__ int s_cnt;
    if (seg_off && n_entries >= 2048 && k_eff <= 256) {   // (uniform; every thread then owns >= 8 entries)
        double m = INFINITY;
        for (int64_t i = tid; i < n_entries; i += 256) m = fmin(m, v[i]);
        s_min[tid] = m;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        int rank = 0;
        for (int o = 0; o < 256; ++o) {
            const double om = s_min[o];
            rank += (om < m || (om == m && o < tid)) ? 1 : 0;
        }
        if (rank == k_eff - 1) s_T = m;
        __syncthreads();
        const double Tv = s_T;
        for (int64_t i = tid; i < n_entries; i += 256) {
            const double x = v[i];
            if (x <= Tv) {
                const int pos = atomicAdd(&s_cnt, 1);
                if (pos < SEL_CAP) {
                    c_v[pos] = x;
                    c_i[pos] = vid ? vid[i] : (int)i;
                }
            }
        }
        __syncthreads();
        if (s_cnt <= SEL_CAP) {   // (uniform)
            v = c_v;
            vid = c_i;
            n_entries = s_cnt;
        }
    }
    double* s_sv = reinterpret_cast<double*>(sel_sm);
    int* s_si = reinterpret_cast<int*>(s_sv + k_eff);
    double pv = -1.0;  // values are >= 0
    int pi = -1;
    for (int r = 0; r < k_eff; ++r) {
        double bv = INFINITY;
        int bi = 0x7fffffff;
        for (int64_t i = tid; i < n_entries; i += 256) {
            const double x = v[i];
            const int id = vid ? vid[i] : (int)i;
            const bool after = (x > pv) || (x == pv && id > pi);
            if (after && (x < bv || (x == bv && id < bi))) {
                bv = x;
                bi = id;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov < bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_v[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
        for (int ww = 1; ww < 4; ++ww) {
            if (s_v[ww] < bv || (s_v[ww] == bv && s_i[ww] < bi)) {
                bv = s_v[ww];
                bi = s_i[ww];
            }
        }
        if (tid == 0) {
            s_sv[r] = bv;
            s_si[r] = bi;
        }
        pv = bv;
        pi = bi;
        __syncthreads();
    }
    if (wave == 0)
        kz_emit_sorted<T>(s_sv, s_si, k_eff, k, exclude_self, self_ids ? self_ids[q] : q_begin + q, metric,
                          out_dist + (int64_t)q * k, out_ind + (int64_t)q * k, lane, p);
}

// The dynamic LDS of a kz_exact_select_kernel<T> launch that selects k_sel neighbours per row -- the ONE rule of every launch site
// (the whole-index fallback and kz_spec_rescue below, the grouped and per-row ranges of kz_range.h): k_sel doubles + k_sel ints.
// The kernel's STATIC LDS (the lists of the long-segment pre-selection) comes on top of it: the runtime is asked for that size,
// once per instantiation -- no constant here to keep in step with the kernel -- and a workgroup that needs more than 64 KiB in
// all (k_sel >= 3749 of the 4096 the exact-only route admits) opts in, as every other launcher of this library does.  Beyond the
// 160 KiB of a CU's LDS no launch can be made: KZ_ERR_UNSUPPORTED (unreachable while KZ_EXACT_MAX_K = 4096: 68.2 KiB).
template <typename T>
static int kz_exact_select_lds(int k_sel, size_t* dyn_bytes) {
    static std::atomic<long long> static_cache{-1};
    long long static_bytes = static_cache.load(std::memory_order_relaxed);
    if (static_bytes < 0) {
        hipFuncAttributes fa;
        KZ_HIP(hipFuncGetAttributes(&fa, (const void*)kz_exact_select_kernel<T>));
        static_bytes = (long long)fa.sharedSizeBytes;
        static_cache.store(static_bytes, std::memory_order_relaxed);
    }
    const size_t dyn = (size_t)k_sel * 12 + 16;
    const size_t total = (size_t)static_bytes + dyn;
    if (total > (size_t)160 * 1024) {
        kz_set_error("kz_knn: %d neighbours per query need %zu bytes of LDS in the exact selection kernel (%lld static), more than the 163840 of a CU",
                     k_sel, total, static_bytes);
        return KZ_ERR_UNSUPPORTED;
    }
    if (total > 65536)   // (per device: set whenever it is needed, the call is host bookkeeping)
        KZ_HIP(hipFuncSetAttribute((const void*)kz_exact_select_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    *dyn_bytes = dyn;
    return KZ_OK;
}

// neighbours per query on the exact-only route.  Selection state: 12 bytes per neighbour, 48 KiB of dynamic LDS at 4096 -- on top
// of kz_exact_select_kernel's ~20 KiB of static LDS: more than 64 KiB in all from 3749 neighbours on, hence the opt-in of
// kz_exact_select_lds (68.2 KiB of a CU's 160 at 4096)
// (KZ_EXACT_MAX_K = 4096: kz_route.h)

// What differs between the callers of the stage.  The defaults are the whole-index fallback's (and kz_gold_ranks'); kz_spec_rescue
// sets every field.
struct KzExactLaunch {
    const int* dyn_n = nullptr;   // speculative launch: the row count lives on the device, nb is the CAPACITY of the launch (kz_spec_row_live);
                                  // the chunk and selection kernels get it too
    bool try_lanes = true;        // try the one-pair-per-lane kernel (which itself wants KZ_XL_MIN_ROWS rows of a host-side count)
    double* lanes_qd = nullptr;   // that kernel's operand buffer where the caller brings it (launches on another stream than the pool's)
    int rows_per_wave = 256;      // kz_launch_exact_rows: index rows a wave walks
    int pair_blocks_max = 0;      // one pair per wave: most workgroups along the index (grid-stride); 0 = one wave per pair
    int two_level_from = 5;       // chunks of KZ_EXACT_CHUNK values from which the selection runs in two levels
};

// vals [nb][index->n]: the float64 ranking values of rows q_begin + fl[b0 .. b0 + nb) of `query` against every index row.  THE dtype /
// metric dispatch of the stage, first match: a precomputed matrix (no arithmetic: kz_precomputed.hip gathers the listed rows or
// columns), one pair per lane, boolean, Minkowski family, four rows in registers, one pair per
// wave.  (The float32-only kernels decline float64 rows themselves.)  Launch errors are the caller's hipGetLastError.
static int kz_exact_distances(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t q_begin, const kz_matrix* query, const kz_matrix* index,
                              double* vals, const KzExactLaunch& ln = KzExactLaunch()) {
    const int metric = index->metric;
    if (metric == KZ_PRECOMPUTED) {
        kz_precomputed_launch_values(ctx, fl, b0, nb, q_begin, query, index, vals);
        return KZ_OK;
    }
    const bool no_gemm_form = metric >= KZ_MANHATTAN;
    const bool f32 = index->dtype == KZ_F32;
    bool lanes = false;
    if (f32 && !no_gemm_form && ln.try_lanes) {
        const int rc = kz_launch_exact_lanes(ctx, fl, b0, nb, q_begin, query, index, metric, vals, &lanes, ln.dyn_n, ln.lanes_qd);
        if (rc != KZ_OK) return rc;
    }
    if (lanes) {
    } else if (kz_is_bool_metric(metric))
        kz_bool_launch_dist(ctx, fl, b0, nb, q_begin, query, index, vals);
    else if (no_gemm_form) {
        return kz_dispatch_rows(index->dtype, "kz_knn", [&](auto e) {
            using T = typename decltype(e)::type;
            if constexpr (kz_half_rows<T>) {   // (kz_matrix_create refuses the pair: the family's differences are taken in float32 / float64)
                kz_set_error("kz_knn: metric %d is not supported for %s rows", metric, kz_dtype_name(index->dtype));
                return (int)KZ_ERR_UNSUPPORTED;
            } else {
                kz_launch_family_dist<T>(ctx, fl, b0, nb, q_begin, query, index, vals);
                return (int)KZ_OK;
            }
        });
    } else if (f32 && ctx->exact_rows && kz_launch_exact_rows(ctx, fl, b0, nb, q_begin, query, index, metric, vals, ln.dyn_n, ln.rows_per_wave)) {
    } else {
        int64_t blocks = (index->n + 3) / 4;
        if (ln.pair_blocks_max > 0 && blocks > ln.pair_blocks_max) blocks = ln.pair_blocks_max;
        const dim3 grid((unsigned)blocks, (unsigned)nb);
        return kz_dispatch_rows(index->dtype, "kz_knn", [&](auto e) {
            using T = typename decltype(e)::type;
            hipLaunchKernelGGL(kz_exact_dist_kernel<T>, grid, dim3(256), 0, ctx->stream, fl, b0, q_begin, (const T*)query->raw, (const T*)index->raw,
                               query->sqn, index->sqn, index->n, (int)index->d, metric, index->mink_p, vals, ln.dyn_n);
            return (int)KZ_OK;
        });
    }
    return KZ_OK;
}

// The selection of k_sel neighbours per row of a value matrix: one level (kz_exact_select_kernel passes over the whole row), or two
// (the k_sel best of every chunk first -- the single-level kernel passes k_sel times over the row with ONE workgroup: 135 us for
// 15 k values at k = 10, where the chunk kernel selects from registers).
struct KzExactSelection {
    int k_sel = 0;
    int n_chunks = 0;
    bool two_level = false;
    size_t lds = 0;   // kz_exact_select_lds
    size_t cand_entries(int rows) const { return two_level ? (size_t)rows * n_chunks * k_sel : 0; }   // cand_v / cand_i the caller brings
};
static int kz_exact_selection(const kz_matrix* index, int k_eff, int two_level_from, KzExactSelection* sel) {
    sel->k_sel = (int)(k_eff < index->n ? k_eff : index->n);
    sel->n_chunks = (int)((index->n + KZ_EXACT_CHUNK - 1) / KZ_EXACT_CHUNK);
    sel->two_level = sel->n_chunks >= two_level_from && sel->k_sel <= KZ_EXACT_CHUNK;
    return kz_dispatch_values(index->dtype, "kz_knn", [&](auto e) { return kz_exact_select_lds<typename decltype(e)::type>(sel->k_sel, &sel->lds); });
}
// The k best of every row of vals [nb][index->n] (kz_exact_distances), written to rows q_begin + fl[b0 + b] of out_dist / out_ind as
// every route writes them.  cand_v / cand_i [sel.cand_entries(nb)]: the survivors of the first level (unused on one level).
static void kz_exact_select(kz_ctx* ctx, const KzExactSelection& sel, const int* fl, int b0, int nb, int64_t q_begin, const kz_matrix* index,
                            int k, int exclude_self, const int64_t* d_self_ids, const double* vals, double* cand_v, int* cand_i,
                            double* out_dist, int64_t* out_ind, const int* dyn_n = nullptr) {
    if (sel.two_level)
        hipLaunchKernelGGL(sel.k_sel >= 24 && ctx->exact_rows ? kz_exact_chunk_radix_kernel : kz_exact_chunk_kernel, dim3(sel.n_chunks, nb),
                           dim3(256), 0, ctx->stream, vals, index->n, sel.k_sel, sel.n_chunks, cand_v, cand_i, dyn_n);
    const double* sel_v = sel.two_level ? (const double*)cand_v : vals;
    const int* sel_i = sel.two_level ? (const int*)cand_i : (const int*)nullptr;
    const int64_t n_entries = sel.two_level ? (int64_t)sel.n_chunks * sel.k_sel : index->n;
    // (an element type that is none of the four never comes here: kz_exact_selection, which made `sel`, has refused it)
    (void)kz_dispatch_values(index->dtype, "kz_knn", [&](auto e) {
        using T = typename decltype(e)::type;
        hipLaunchKernelGGL(kz_exact_select_kernel<T>, dim3(nb), dim3(256), sel.lds, ctx->stream, fl, b0, q_begin, sel_v, sel_i, n_entries, index->n,
                           k, exclude_self ? 1 : 0, d_self_ids, index->metric, index->mink_p, out_dist, out_ind, dyn_n);
        return (int)KZ_OK;
    });
}

// The begin of a walk over n_rows listed rows against the whole index.  Many rows of a cosine search: the normalised float64 index rows,
// once -- what the float32 kernels then read.  -> query rows per batch: 256 MiB of values, at most a grid's y extent; vals: the
// context's scratch block.
static int kz_exact_begin(kz_ctx* ctx, kz_matrix* index, int n_rows, int* batch_out, double** vals) {
    if (index->metric == KZ_COSINE && n_rows >= 64 && ctx->exact_rows) {
        const int rc = kz_matrix_norm64(index);
        if (rc != KZ_OK) return rc;
    }
    int64_t batch = ((int64_t)256 << 20) / (index->n * 8);
    if (batch < 1) batch = 1;
    if (batch > n_rows) batch = n_rows;
    if (batch > 65535) batch = 65535;
    *batch_out = (int)batch;
    void* v = nullptr;
    const int rc = kz_scratch(ctx, (size_t)batch * (size_t)index->n * 8, &v);
    *vals = (double*)v;
    return rc;
}
// The walk of the whole-index entry points (kz_gold_ranks.h, kz_knn_reduced.h) behind kz_exact_begin: per batch of rows
// q_begin + fl[b0 .. b0 + nb) the value matrix (kz_exact_distances), then per_batch(b0, nb) -- the caller's launches on it.  Ends
// synchronised with the stream.
template <typename F>
static int kz_exact_walk(const char* who, kz_ctx* ctx, const int* fl, int n_rows, int batch, double* vals, int64_t q_begin, const kz_matrix* query,
                         const kz_matrix* index, F per_batch) {
    for (int b0 = 0; b0 < n_rows; b0 += batch) {
        const int nb = n_rows - b0 < batch ? n_rows - b0 : batch;
        const int rc = kz_exact_distances(ctx, fl, b0, nb, q_begin, query, index, vals);
        if (rc != KZ_OK) return rc;
        per_batch(b0, nb);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        kz_set_error("%s: exact kernels failed: %s", who, hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    return KZ_OK;
}

// (kz_range.h needs kz_knn_impl and therefore comes later in the translation unit)
static int kz_range_rescue(kz_ctx* ctx, kz_matrix* query, int64_t q0, const int* fl, const double* tau, int n_fail, kz_matrix* index, int k,
                           int exclude_self, const int64_t* d_self_ids, double* out_dist, int64_t* out_ind, int* left, int* n_left,
                           long long* n_pairs_out, long long* n_grouped_out, bool grouped_only, int per_row_max);

struct KzExactTaken {   // what the range re-search took off a fallback, and the time of all of it
    int64_t range_rows = 0, range_pairs = 0, range_group_rows = 0;
    float ms = 0;
};
// THE WHOLE-INDEX FALLBACK of kz_knn_impl: rows q_begin + fail_list[0 .. n_fail) get their exact float64 neighbours.  fail_list /
// fail_tau live in the context's scratch block, which the value matrix re-carves: they are copied first.  try_range: the range
// re-search (kz_range.h) goes first -- the exact kernels on the pairs that can matter; the rows it hands back go on against the whole
// index in batches.  Ends synchronised with the stream.
static int kz_exact_whole_index(kz_ctx* ctx, kz_matrix* query, int64_t q_begin, const int* fail_list, const double* fail_tau, int n_fail,
                                bool try_range, kz_matrix* index, int k, int exclude_self, const int64_t* d_self_ids, double* out_dist,
                                int64_t* out_ind, KzExactTaken* taken) {
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    // (released when this function ends, stream-ordered: fl, cand_v, cand_i)
    KzPoolBuf<int> cand_i;
    KzPoolBuf<double> cand_v;
    KzPoolBuf<int> fl;
    int rc = fl.alloc(ctx, (size_t)n_fail * sizeof(int));  // stream-ordered pool: no device sync
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemcpyAsync(fl.get(), fail_list, (size_t)n_fail * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    if (try_range) {
        KzPoolBuf<int> left;
        KzPoolBuf<double> tau;
        rc = tau.alloc(ctx, (size_t)n_fail * 8);
        if (rc == KZ_OK) rc = left.alloc(ctx, (size_t)n_fail * sizeof(int));
        if (rc == KZ_OK && hipMemcpyAsync(tau.get(), fail_tau, (size_t)n_fail * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            kz_set_error("kz_knn: copying the bounds of the uncertified rows failed");
            rc = KZ_ERR_HIP;
        }
        long long pairs = 0, grouped = 0;
        int n_dense = n_fail;
        const bool no_mem = rc == KZ_ERR_NOMEM;   // (no room for the lists: the whole-index kernels as before)
        if (rc == KZ_OK)
            rc = kz_range_rescue(ctx, query, q_begin, fl.get(), tau.get(), n_fail, index, k, exclude_self, d_self_ids, out_dist, out_ind,
                                 left.get(), &n_dense, &pairs, &grouped, false, 0);
        tau.reset();
        if (no_mem) {
            left.reset();
        } else {
            if (rc != KZ_OK) return rc;
            taken->range_rows += n_fail - n_dense;
            taken->range_pairs += pairs;
            taken->range_group_rows += grouped;
            fl = std::move(left);   // (the rows handed back take the list's place)
            n_fail = n_dense;
        }
    }
    if (n_fail > 0) {
        int batch = 0;
        double* vals = nullptr;
        rc = kz_exact_begin(ctx, index, n_fail, &batch, &vals);
        if (rc != KZ_OK) return rc;
        KzExactSelection sel;
        rc = kz_exact_selection(index, k + (exclude_self ? 1 : 0), KzExactLaunch().two_level_from, &sel);
        if (rc != KZ_OK) return rc;
        if (sel.two_level) {
            rc = cand_v.alloc(ctx, sel.cand_entries(batch) * 8);
            if (rc == KZ_OK) rc = cand_i.alloc(ctx, sel.cand_entries(batch) * 4);
            if (rc != KZ_OK) return rc;
        }
        for (int b0 = 0; b0 < n_fail; b0 += batch) {
            const int nb = n_fail - b0 < batch ? n_fail - b0 : batch;
            rc = kz_exact_distances(ctx, fl.get(), b0, nb, q_begin, query, index, vals);
            if (rc != KZ_OK) return rc;
            kz_exact_select(ctx, sel, fl.get(), b0, nb, q_begin, index, k, exclude_self, d_self_ids, vals, cand_v.get(), cand_i.get(), out_dist, out_ind);
        }
    } else {
        fl.reset();
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[4], ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        kz_set_error("kz_knn: exact fallback failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    KZ_HIP(hipEventElapsedTime(&taken->ms, ctx->ev[3], ctx->ev[4]));
    return KZ_OK;
}
