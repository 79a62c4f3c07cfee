// The five POINTWISE hubness reductions: w = f(d, query-side state, target-side state) of one pair's distance d, in float64, as
// the reference evaluates them with separate numpy operations (the library is compiled with -ffp-contract=off: no fused
// multiply-add is formed, so one expression gives one result wherever it is inlined).  Two callers, which must not drift:
//   the transform kernels over the [n, K] candidate arrays        (kz_hubness.hip: kz_csls_kernel, kz_ls_kernel, kz_mp_normal_kernel,
//                                                                  kz_dual_shift_kernel)
//   the count kernel over the whole index row of the value matrix (kz_gold_ranks.h: kz_rank_count_kernel)
// (The fifth, kz_reduce_dual, has no counterpart in the reference: its state comes from kz_softmin_rows, not from neighbour lists.)
//
//   CSLS            kiez/hubness_reduction/csls.py:90-93
//   LocalScaling    kiez/hubness_reduction/local_scaling.py:135-147
//   MutualProximity kiez/hubness_reduction/mutual_proximity.py:177-183 ('normal')
#pragma once

// CSLS: 2 d - r_test - r_train  (r_test: mean of the query's K forward distances; r_train: mean of the target's K reverse ones)
__device__ __forceinline__ double kz_reduce_csls(double d, double r_test, double r_train) {
    double v = 2.0 * d;
    v = v - r_test;
    v = v - r_train;
    return v;
}

// LocalScaling 'standard': 1 - exp(-d^2 / (r_s r_t))  (r_s, r_t: the K-th forward / reverse distance)
__device__ __forceinline__ double kz_reduce_ls(double d, double r_s, double r_t) {
    const double inner = (-1.0 * (d * d)) / (r_s * r_t);
    return 1.0 - exp(inner);
}

// NICDM: d / sqrt(r_s r_t)  (r_s, r_t: the mean forward / reverse distance)
__device__ __forceinline__ double kz_reduce_nicdm(double d, double r_s, double r_t) { return d / sqrt(r_s * r_t); }

// scipy.stats.norm.sf(x, loc, scale) = ndtr(-(x-loc)/scale), cephes ndtr (scipy/special/xsf/cephes/ndtr.h)
__device__ __forceinline__ double kz_ndtr(double a) {
    const double SQRT1_2 = 0.70710678118654752440;
    if (isnan(a)) return a;
    const double x = a * SQRT1_2;
    const double z = fabs(x);
    if (z < SQRT1_2) return 0.5 + 0.5 * erf(x);
    double y = 0.5 * erfc(z);
    if (x > 0) y = 1.0 - y;
    return y;
}

// Dual potentials (Sinkhorn, inverted softmax): (d - f) - g  (f: the source row's potential, g: the target row's -- the soft-min
// potentials of kz_softmin_rows, kz_softmin.h; two subtractions in this order, as numpy's (D - f[:, None]) - g[None, :])
__device__ __forceinline__ double kz_reduce_dual(double d, double f, double g) {
    double v = d - f;
    v = v - g;
    return v;
}

// ---- the soft-min's partial result (kz_softmin.h: level 1 writes one per chunk; kz_softmin.hip: level 2 folds them) ----------
// (m, s) of a set of values x: m = min x, s = sum exp(-(x - m) / eps) over the set, so that softmin_eps = m - eps log s.  Every term
// is exp of a value <= 0 and the minimum's own term is 1: no term overflows and s >= 1 whatever eps is.  A set without a value
// below +inf is (+inf, 0); a set with a -inf is (-inf, 1) -- its s is never read.
struct KzSoftminPart {
    double m, s;
};
// s of the part rescaled to the minimum mg <= part.m of a larger set (mg finite)
__device__ __forceinline__ double kz_softmin_rescaled(KzSoftminPart part, double mg, double eps) {
    return part.m == INFINITY ? 0.0 : part.s * exp(-((part.m - mg) / eps));
}

// MutualProximity 'normal': 1 - sf(d; mu, sd) sf(d; mu_t, sd_t).  Both survival functions underflow towards 0 for a pair far
// beyond both lists: the product is then below 2^-53 and the result is exactly 1.0.
__device__ __forceinline__ double kz_reduce_mp_normal(double d, double mu, double sd, double mu_t, double sd_t) {
    const double p1 = kz_ndtr(-((d - mu) / sd));
    const double p2 = kz_ndtr(-((d - mu_t) / sd_t));
    return 1.0 - p1 * p2;
}
