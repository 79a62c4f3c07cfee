// Level 2 of kz_softmin_rows (kz_softmin.h holds the host side and level 1, inside kz_knn.hip's translation unit, where the exact
// stage lives; this level needs none of it and compiles apart): the n_chunks parts (m, s) of a row, written by level 1, become
//     out = (mg - eps log sum_c s_c exp(-(m_c - mg) / eps)) + shift,      mg = min_c m_c.
// One wave per row, four rows per workgroup; no LDS, no barrier, nothing waits for another workgroup.
#include "kz_common.h"
#include "kz_reduce.h"   // KzSoftminPart, kz_softmin_rescaled

// part [nb][n_chunks] -> out [nb].  Lane l takes the chunks l, l + 64, ... in ascending order, then the 64 lanes meet in xor
// butterflies (both partners add the same two numbers: every lane ends with the same bits): a tree whose shape is a function of
// n_chunks alone -- up to 64 chunks, 262 144 index rows, it is the butterfly over the chunks themselves.  The chunk that holds the
// row's minimum rescales by exp(-0) = 1, so the sum is >= 1.  No entry below +inf: +inf + shift; a -inf: -inf.
__global__ __launch_bounds__(256) void kz_softmin_fold_kernel(const KzSoftminPart* __restrict__ part, int n_chunks, int nb, double eps, double shift,
                                                              double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nb) return;   // (wave-uniform)
    const KzSoftminPart* __restrict__ p = part + (int64_t)b * n_chunks;
    double m = INFINITY;
    for (int c = lane; c < n_chunks; c += 64) {
        const double t = p[c].m;
        m = t < m ? t : m;
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const double t = __shfl_xor(m, sh, 64);
        m = t < m ? t : m;
    }
    if (m == INFINITY || m == -INFINITY) {   // (wave-uniform)
        if (lane == 0) out[b] = m < 0.0 ? m : m + shift;
        return;
    }
    double s = 0.0;
    for (int c = lane; c < n_chunks; c += 64) s += kz_softmin_rescaled(p[c], m, eps);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) out[b] = (m - eps * log(s)) + shift;
}

void kz_softmin_fold_launch(hipStream_t stream, const KzSoftminPart* part, int n_chunks, int nb, double eps, double shift, double* out) {
    hipLaunchKernelGGL(kz_softmin_fold_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, stream, part, n_chunks, nb, eps, shift, out);
}
