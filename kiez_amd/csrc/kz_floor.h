// Host-only part of the population floor (kz_knn.hip "POPULATION FLOOR"): the model fitted to the probe.  No HIP dependency
// (tests/host/floor_sanitize.cpp builds it with g++ under AddressSanitizer + UBSan).
#pragma once
#include <cstddef>

// pairs[2 i] = |q_c|^2 of probe row i, pairs[2 i + 1] = the exact key of its k-th neighbour.  Least squares key ~ alpha + beta |q_c|^2;
// the floor of a row is  alpha + beta |q_c|^2 - margin  with margin = (largest amount by which a probe row's key falls short of the
// model) x margin_scale.  By construction no probe row lies below its floor when margin_scale >= 1, and -- the rows being
// exchangeable -- another row does with probability <= 1 / (n_probe + 1).  Returns false (no floor) when the probe's values are not
// finite or there are no probe rows; a probe whose |q_c|^2 are all equal gets beta = 0.
static inline bool kz_floor_fit(const double* pairs, int n_probe, double margin_scale, double* model) {
    model[0] = model[1] = model[2] = 0.0;
    if (n_probe <= 0) return false;
    double sx = 0, sy = 0;
    for (int i = 0; i < n_probe; ++i) {
        sx += pairs[2 * i];
        sy += pairs[2 * i + 1];
    }
    const double mx = sx / n_probe, my = sy / n_probe;
    double sxx = 0, sxy = 0;
    for (int i = 0; i < n_probe; ++i) {
        sxx += (pairs[2 * i] - mx) * (pairs[2 * i] - mx);
        sxy += (pairs[2 * i] - mx) * (pairs[2 * i + 1] - my);
    }
    const double beta = sxx > 0 ? sxy / sxx : 0.0, alpha = my - beta * mx;
    double short_max = 0;
    for (int i = 0; i < n_probe; ++i) {
        const double r = alpha + beta * pairs[2 * i] - pairs[2 * i + 1];   // the model above the row's k-th key by r
        if (r > short_max) short_max = r;
    }
    model[0] = alpha;
    model[1] = beta;
    model[2] = short_max * margin_scale;
    return (alpha - alpha == 0.0) && (beta - beta == 0.0) && (model[2] - model[2] == 0.0);
}

// Share of the variance of the probe's k-th keys that the straight line explains (pairs as for kz_floor_fit): the squared
// correlation of key and |q_c|^2.  0 when either is constant, when there are fewer than two rows or when a value is not finite.
static inline double kz_floor_r2(const double* pairs, int n_probe) {
    if (n_probe < 2) return 0.0;
    double sx = 0, sy = 0;
    for (int i = 0; i < n_probe; ++i) {
        sx += pairs[2 * i];
        sy += pairs[2 * i + 1];
    }
    const double mx = sx / n_probe, my = sy / n_probe;
    double sxx = 0, sxy = 0, syy = 0;
    for (int i = 0; i < n_probe; ++i) {
        const double dx = pairs[2 * i] - mx, dy = pairs[2 * i + 1] - my;
        sxx += dx * dx;
        sxy += dx * dy;
        syy += dy * dy;
    }
    if (!(sxx > 0) || !(syy > 0)) return 0.0;
    const double r2 = sxy * sxy / (sxx * syy);
    return r2 - r2 == 0.0 ? (r2 < 1.0 ? r2 : 1.0) : 0.0;
}

// MODEL THRESHOLDS of the shared sweep (kz_knn_dual.h "MODEL THRESHOLDS"): the same fit for the rows of b against all of a, from a
// probe that kept k_p >= k neighbours per row.  rows[i (k_p + 1)] = |t_c|^2 of probe row i, followed by the exact keys of its k_p
// nearest rows in descending order.  tau(t) = alpha + beta |t_c|^2 - margin, margin as kz_floor_fit takes it (from the k-th key).
// With that tau, count = the neighbours of a probe row at or above its threshold: the events the row would get, observed as long
// as count < k_p (count == k_p: SATURATED, the row has an unknown number of further events) -- and at least k unless the row is
// SHORT (margin_scale < 1 only).
struct KzThetaFit {
    double alpha, beta, margin;
    double mean_count;
    int max_count, n_saturated, n_short;
};
static inline bool kz_theta_fit(const double* rows, int n_probe, int k_p, int k, double margin_scale, KzThetaFit* out) {
    out->alpha = out->beta = out->margin = out->mean_count = 0.0;
    out->max_count = out->n_saturated = out->n_short = 0;
    if (n_probe <= 0 || k < 1 || k_p < k) return false;
    const size_t w = (size_t)k_p + 1;
    double sx = 0, sy = 0;
    for (int i = 0; i < n_probe; ++i) {
        sx += rows[i * w];
        sy += rows[i * w + k];
    }
    const double mx = sx / n_probe, my = sy / n_probe;
    double sxx = 0, sxy = 0;
    for (int i = 0; i < n_probe; ++i) {
        sxx += (rows[i * w] - mx) * (rows[i * w] - mx);
        sxy += (rows[i * w] - mx) * (rows[i * w + k] - my);
    }
    const double beta = sxx > 0 ? sxy / sxx : 0.0, alpha = my - beta * mx;
    double short_max = 0;
    for (int i = 0; i < n_probe; ++i) {
        const double r = alpha + beta * rows[i * w] - rows[i * w + k];
        if (r > short_max) short_max = r;
    }
    const double margin = short_max * margin_scale;
    if (!((alpha - alpha == 0.0) && (beta - beta == 0.0) && (margin - margin == 0.0))) return false;
    long long total = 0;
    for (int i = 0; i < n_probe; ++i) {
        const double tau = alpha + beta * rows[i * w] - margin;
        int c = 0;
        for (int j = 1; j <= k_p; ++j) c += rows[i * w + j] >= tau ? 1 : 0;   // (every key, not a prefix: a non-finite key counts as below)
        total += c;
        if (c > out->max_count) out->max_count = c;
        if (c == k_p) ++out->n_saturated;
        if (c < k) ++out->n_short;
    }
    out->alpha = alpha;
    out->beta = beta;
    out->margin = margin;
    out->mean_count = (double)total / n_probe;
    return true;
}
