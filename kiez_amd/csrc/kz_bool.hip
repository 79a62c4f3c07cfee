// scipy's boolean metrics (jaccard, dice, rogerstanimoto, russellrao, sokalmichener, sokalsneath, yule) on bit-packed rows:
// the pack kernel, the tiled popcount distance kernel of the exact route and the pair kernel of kz_pair_values.
// (kz_bool.h: the finish -- the four integers of a pair to scipy's value; DESIGN.md section 3.1b: the kernel's bounds.)
#include "kz_bool.h"

// ---- the image ----------------------------------------------------------------------------------------------------
// One wave per row.  A step takes 64 consecutive features (one coalesced read), the ballot of x != 0 is two image words; lane 0
// stores them.  The row is written up to its padded length W (a multiple of four words): features past d are false.
template <typename T>
__global__ __launch_bounds__(256) void kz_bool_pack_kernel(const T* __restrict__ raw, int64_t n, int d, int W, uint32_t* __restrict__ bits,
                                                           int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;   // (whole wave)
    const T* __restrict__ x = raw + r * (int64_t)d;
    uint32_t* __restrict__ out = bits + r * (int64_t)W;
    int total = 0;
    for (int s = 0; s < W / 2; ++s) {
        const int j = s * 64 + lane;
        const bool on = j < d && x[j] != (T)0;
        const unsigned long long mask = __ballot(on);
        total += __popcll(mask);
        if (lane == 0) {
            out[2 * s] = (uint32_t)mask;
            out[2 * s + 1] = (uint32_t)(mask >> 32);
        }
    }
    if (lane == 0) cnt[r] = total;
}

int kz_bool_image(kz_matrix* m) {
    kz_ctx* ctx = m->ctx;
    const int W = (int)(((m->d + 31) / 32 + 3) / 4) * 4;
    m->bits_words = W;
    if (kz_pool_alloc(ctx, (size_t)m->n * (size_t)W * 4, (void**)&m->bits) != KZ_OK ||
        kz_pool_alloc(ctx, (size_t)m->n * 4, (void**)&m->bits_cnt) != KZ_OK) {
        kz_set_error("kz_matrix_create: out of device memory (bit image of the boolean metrics)");
        return KZ_ERR_NOMEM;
    }
    const dim3 grid((unsigned)((m->n + 3) / 4));
    const int rcd = kz_dispatch_rows(m->dtype, "kz_matrix_create", [&](auto el) {
        using T = typename decltype(el)::type;
        if constexpr (kz_half_rows<T>) {   // (kz_matrix_create refuses the pair before it comes here)
            kz_set_error("kz_matrix_create: the boolean metrics take float32 / float64 rows");
            return (int)KZ_ERR_UNSUPPORTED;
        } else {
            hipLaunchKernelGGL(kz_bool_pack_kernel<T>, grid, dim3(256), 0, ctx->stream, (const T*)m->raw, m->n, (int)m->d, W, m->bits, m->bits_cnt);
            return (int)KZ_OK;
        }
    });
    if (rcd != KZ_OK) return rcd;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kz_set_error("kz_matrix_create: bit-pack kernel failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    return KZ_OK;
}

void kz_bool_image_free(kz_matrix* m) {
    kz_pool_free(m->ctx, m->bits, 0);
    kz_pool_free(m->ctx, m->bits_cnt, 0);
}

// ---- the distance kernel --------------------------------------------------------------------------------------------
// The tile shape of kz_family_dist_kernel: 256 threads own 64 queries x 64 index rows, a thread 4 x 4 pairs.  The image words are
// staged through LDS KZ_BOOL_WK words at a time, transposed ([word][row]): thread t copies four consecutive words (one 16-byte
// load; rows are padded to four words) of row (t & 63) of both tiles, and reads its four query rows' and its four index rows' word
// as one 16-byte LDS read each.  Per pair and word: one AND, one popcount that adds into the pair's int32 count.  The finish, once
// per pair: kz_bool_finish -- the metric is a run-time argument, one kernel serves all seven; self_zero: the pair of a row with itself
// is 0 (kz_bool.h: kz_bool_self_zero).  Output: the [batch][n_i] float64
// value matrix the exact selection kernels read, as kz_family_dist_kernel writes it.
#define KZ_BOOL_WK 16
__global__ __launch_bounds__(256) void kz_bool_dist_kernel(const int* __restrict__ fail_list, int batch0, int nb, int64_t q_begin,
                                                           const uint32_t* __restrict__ qbits, const uint32_t* __restrict__ ybits,
                                                           const int32_t* __restrict__ qcnt, const int32_t* __restrict__ ycnt, int64_t n_i,
                                                           int W, int d, int metric, int self_zero, double* __restrict__ vals) {
    __shared__ __attribute__((aligned(16))) uint32_t sQ[KZ_BOOL_WK][64];
    __shared__ __attribute__((aligned(16))) uint32_t sY[KZ_BOOL_WK][64];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t y0 = (int64_t)blockIdx.x * 64;
    const int b0 = blockIdx.y * 64;
    // staging: rows past the end read the last row again (their pairs are never written)
    const int lrow = t & 63, lseg = (t >> 6) * 4;
    const int bq = b0 + lrow < nb ? b0 + lrow : nb - 1;
    const int64_t qrow_l = q_begin + fail_list[batch0 + bq];
    const int64_t yrow_l = y0 + lrow < n_i ? y0 + lrow : n_i - 1;
    const uint32_t* __restrict__ qp = qbits + qrow_l * (int64_t)W;
    const uint32_t* __restrict__ yp = ybits + yrow_l * (int64_t)W;
    int acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0;
    for (int k0 = 0; k0 < W; k0 += KZ_BOOL_WK) {
        const int k = k0 + lseg;
        uint4 rq = make_uint4(0u, 0u, 0u, 0u), ry = make_uint4(0u, 0u, 0u, 0u);
        if (k < W) {   // (W is a multiple of 4: the four words are inside the row or all behind it)
            rq = *reinterpret_cast<const uint4*>(qp + k);
            ry = *reinterpret_cast<const uint4*>(yp + k);
        }
        __syncthreads();   // (the previous chunk has been read)
        sQ[lseg][lrow] = rq.x;
        sQ[lseg + 1][lrow] = rq.y;
        sQ[lseg + 2][lrow] = rq.z;
        sQ[lseg + 3][lrow] = rq.w;
        sY[lseg][lrow] = ry.x;
        sY[lseg + 1][lrow] = ry.y;
        sY[lseg + 2][lrow] = ry.z;
        sY[lseg + 3][lrow] = ry.w;
        __syncthreads();
        const int jn = W - k0 < KZ_BOOL_WK ? W - k0 : KZ_BOOL_WK;   // (a multiple of 4)
#pragma unroll 4
        for (int j = 0; j < jn; ++j) {
            const uint4 q4 = *reinterpret_cast<const uint4*>(&sQ[j][ty * 4]);
            const uint4 y4 = *reinterpret_cast<const uint4*>(&sY[j][tx * 4]);
            const uint32_t q[4] = {q4.x, q4.y, q4.z, q4.w};
            const uint32_t y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] += __popc(q[a] & y[c]);
        }
    }
    int ny[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t i = y0 + tx * 4 + c;
        ny[c] = i < n_i ? ycnt[i] : 0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int b = b0 + ty * 4 + a;
        if (b >= nb) continue;
        const int64_t qrow = q_begin + fail_list[batch0 + b];
        const int nx = qcnt[qrow];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t i = y0 + tx * 4 + c;
            if (i >= n_i) continue;
            vals[(int64_t)b * n_i + i] = (self_zero && i == qrow) ? 0.0 : kz_bool_finish(metric, d, nx, ny[c], acc[a][c]);
        }
    }
}

void kz_bool_launch_dist(kz_ctx* ctx, const int* fail_list, int b0, int nb, int64_t q_begin, const kz_matrix* query, const kz_matrix* index,
                         double* vals) {
    const dim3 grid((unsigned)((index->n + 63) / 64), (unsigned)((nb + 63) / 64));
    hipLaunchKernelGGL(kz_bool_dist_kernel, grid, dim3(256), 0, ctx->stream, fail_list, b0, nb, q_begin, (const uint32_t*)query->bits,
                       (const uint32_t*)index->bits, (const int32_t*)query->bits_cnt, (const int32_t*)index->bits_cnt, index->n, index->bits_words,
                       (int)index->d, index->metric, kz_bool_self_zero(query, index) ? 1 : 0, vals);
}

// ---- kz_pair_values ---------------------------------------------------------------------------------------------------
// One wave per query row, one lane per pair: the same integers, the same finish -- the values that travel between GPUs ARE the
// search's values.  An index outside the matrix: +inf, as for every other metric.
__global__ __launch_bounds__(256) void kz_bool_pair_values_kernel(const uint32_t* __restrict__ qbits, const int32_t* __restrict__ qcnt,
                                                                  int64_t q_begin, int64_t q_count, const uint32_t* __restrict__ ybits,
                                                                  const int32_t* __restrict__ ycnt, int64_t n_i, int W, int d, int metric,
                                                                  const int64_t* __restrict__ ind, int K, int self_zero, double* __restrict__ val) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q_count) return;
    const int64_t qrow = q_begin + r;
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(qbits + qrow * (int64_t)W);
    const int nx = qcnt[qrow];
    for (int c = threadIdx.x & 63; c < K; c += 64) {
        const int64_t yi = ind[r * (int64_t)K + c];
        double v = INFINITY;
        if (yi >= 0 && yi < n_i) {
            const uint4* __restrict__ y = reinterpret_cast<const uint4*>(ybits + yi * (int64_t)W);
            int ntt = 0;
            for (int w = 0; w < W / 4; ++w) {
                const uint4 a = q[w], b = y[w];
                ntt += __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w);
            }
            v = (self_zero && yi == qrow) ? 0.0 : kz_bool_finish(metric, d, nx, ycnt[yi], ntt);
        }
        val[r * (int64_t)K + c] = v;
    }
}

void kz_bool_launch_pair_values(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                                const int64_t* d_ind, int k, double* d_val) {
    hipLaunchKernelGGL(kz_bool_pair_values_kernel, dim3((unsigned)((q_count + 3) / 4)), dim3(256), 0, ctx->stream, (const uint32_t*)query->bits,
                       (const int32_t*)query->bits_cnt, q_begin, q_count, (const uint32_t*)index->bits, (const int32_t*)index->bits_cnt, index->n,
                       index->bits_words, (int)query->d, query->metric, d_ind, k, kz_bool_self_zero(query, index) ? 1 : 0, d_val);
}
