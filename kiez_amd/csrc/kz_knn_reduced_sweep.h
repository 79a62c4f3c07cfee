// WHOLE-INDEX REDUCED TOP-K ON THE fp16 SWEEP (kz_knn_reduced_sweep, opt-in): the lists of kz_knn_reduced -- the same bytes for every
// input -- with the float64 value matrix replaced by a first pass on the fp16 MFMA sweep.  The fast pass only
// decides WHICH pairs need the exact value (section 4):
//   1. seeds: any k distinct index rows of a query row give an upper bound tau_i of its k-th smallest w over the whole index -- the
//      k-th smallest exact w among them (kz_r1_seed_w_kernel: kz_exact_value + kz_rank_reduce, the exact route's expression and bits;
//      kz_r1_tau_kernel).  After a fit the forward candidate lists are such rows;
//   2. "w_ij <= tau_i" is a bound on the pair's ranking value that is rank one plus separable, v_ij <= P_i + Q_i U_j + V_j
//      (kz_r1_forms below); kz_r1_index_kernel writes the index side (V folded into a copy of the image's bias row, U, per-tile
//      Umin / Umax), kz_r1_query_kernel the query side {P', Q'} in key units, lowered by the rounding bound;
//   3. kz_knn_emit_r1_h_kernel (kz_knn_emit_r1_16.h) logs every pair the fp16 tier cannot exclude;
//   4. the log is ordered by (query row, index row) (kz_cert_order_log: two stable sort passes); kz_r1_resolve_kernel evaluates
//      every entry exactly and checks the bound on it; kz_r1_select_kernel writes each row's k smallest by (w, index row) in
//      kz_knn_reduced's integer order and checks the row: at least k entries with w <= tau_i, every seed that defined tau_i among them.
// The WHOLE call takes kz_knn_reduced -- route_taken = 0, never an error -- for a shape outside the sweep (kz_rank_sweep_shapes_ok),
// k > 128, k_seed > 1024, KZ_RANK_MP_NORMAL (not rank one), a state that makes a form invalid, a log that overflowed, a violated bound
// or row check.  There is no per-row fallback yet.
//
// THE FORMS.  d = the distance the reduction is fed (kz_output_distance<float>): d = v under cosine / sqeuclidean; under euclidean
// d = fl32(sqrt(fl32 v)), for which kz_radius_band_kernel's bracket gives  d <= D  =>  v <= D^2 (1 + 8 u) + 2^-140,  u = 2^-24.
// With a = q_a[i], b = t_a[j] and rho = 2^-20 = 16 u (below: why that covers every rounding between v and the compared w):
//   CSLS   w = fl(fl(2 d - a) - b) <= tau   =>  d <= (c + b') / 2,  c = tau + a + rho (|tau| + |a|),  b' = b + rho |b|
//            d = v:  P = c / 2, Q = 0, V = b' / 2;           euclidean:  v <= (c + b')^2 / 4:  P = c^2 / 4, Q = c / 2, U = b', V = b'^2 / 4
//   DUAL   w = fl(fl(d - f) - g) <= tau     =>  d <= p + g',       p = tau + f + rho (|tau| + |f|),  g' = g + rho |g|
//            d = v:  P = p, Q = 0, V = g';                   euclidean:  v <= (p + g')^2:      P = p^2, Q = 2 p, U = g', V = g'^2
//   NICDM  w = d / sqrt(a b) <= tau         =>  d <= tau sqrt(a) sqrt(b) (1 + 2^-50)            (a, b > 0, tau >= 0)
//            d = v:  Q = tau sqrt(a), U = sqrt(b);           euclidean:  v <= tau^2 a b:       Q = tau^2 a, U = b
//   LS     w = 1 - exp(-d^2 / (a b)) <= tau =>  d^2 <= L a b,  L = -log1p(-tau) (1 + rho) + 2^-30   (a, b > 0, 0 <= tau <= 1 - 2^-20)
//            d = v:  Q = sqrt(L a), U = sqrt(b);             euclidean:  v <= L a b:           Q = L a, U = b
// The squares admit pairs the true condition excludes when c + b' < 0 (no d >= 0 satisfies it): the sweep need only produce a
// SUPERSET, the exact resolve orders everything.  Every P, Q, V above is then widened OUTWARD once more: P (1 + rho), V (1 + rho) for
// the squared terms, Q (1 + rho) where Q >= 0 is a product, and rho |Q| max|U| + 2^-140 is added to P for the cross term.
// Why rho = 2^-20 is enough: (i) the float64 roundings of w's expression are a few 2^-53 of the magnitudes |tau|, |a|, |b|, d that
// rho multiplies -- not of their possibly cancelling sum, which is why c carries rho (|tau| + |a|) and not rho |tau + a|; (ii) the
// float32 bracket 8 u of euclidean distances multiplies a sum of terms each of which gets 16 u of its own magnitude; (iii) the
// inversion of exp (an error of one or two 2^-53 of a value in [2^-20, 1], moving its logarithm by at most 2^-32) sits inside
// 2^-30; sqrt(a b) against sqrt(a) sqrt(b) differs by 2^-52.  A state outside the brackets named above raises the fallback flag.
//
// THE KEY-UNIT BOUND.  The fp16 tier's key of a pair is key = qc2 / 2 - h v (h = 1 under cosine, 1/2 otherwise) and the kernel's
// acc = key~ with |key~ scale - key| <= eps_i = kz_h_key_eps (the ONE expression, unchanged).  The condition v <= P + Q U_j + V_j is
//     key + h V_j + h Q U_j >= qc2 / 2 - h P .
// The kernel evaluates t = fma(Qf, Uf_j, key~ + fl(bias_j + h V_j / scale)) >= Pf.  Beyond eps_i the left side errs by
//   * the float rounding of the shifted bias, 2^-24 |bias'_j| <= 2^-24 W, W = max_j |bias'_j| scale;
//   * the float32 accumulation that now starts from bias' instead of bias: kz_gamma_acc_h bounds a sum by gamma x the sum of its
//     terms' magnitudes, so the start value adds gamma W (eps_i already carries the image's own bias; counting it twice only widens);
//   * the float conversions of Q' and U_j: 2 x 2^-24 |h Q| max|U| (+ second order);
//   * the FMA's own rounding: NONE -- rounding is monotone and Pf is a float, so x >= Pf implies fl(x) >= Pf;
//   * the float conversion of P': Pf is rounded DOWN and one float step further.
// E_i = eps_i + eps_mult ((gamma + 2^-23) W + 3 x 2^-24 |h Q_i| max|U|) is what Pf is lowered by, and what the resolve kernel checks
// on every entry: |t scale - (key + h V_j + h Q_i U_j)| / E_i <= 1 with the exact key and the float64 V, U, Q.
// Pad index rows keep bias -inf (U = 0); pad query rows get P' = +inf, Q' = 0.
#pragma once
#include "kz_knn_emit_r1_16.h"
#include "kz_cert_sweep.h"

enum { KZ_R1_F_INVALID = 1, KZ_R1_F_VIOLATED = 2 };
constexpr int KZ_R1_MAX_K = 128;
constexpr int KZ_R1_MAX_SEEDS = 1024;
// (log size: max(KZ_CERT_LOG_PER_ROW, 4 k) entries per query row -- the radius sweep's sizing choice, scaled with k)
#define KZ_R1_RHO 9.5367431640625e-07 /* 2^-20 */

// Query side (P, Q) from (tau, a); index side (U, V) from b.  EUC: the metric is euclidean (d = sqrt v).
template <int KIND, bool EUC>
__device__ __forceinline__ void kz_r1_query_form(double tau, double a, double umax, double* P, double* Q, bool* ok) {
    const double rho = KZ_R1_RHO, tiny = 7.174648137343064e-43 /* 2^-140 */;
    double p = 0.0, q = 0.0;
    bool good = true;
    if (KIND == KZ_RANK_CSLS || KIND == KZ_RANK_DUAL) {
        const double c = tau + a + rho * (fabs(tau) + fabs(a));
        if (KIND == KZ_RANK_CSLS) {
            p = EUC ? 0.25 * c * c : 0.5 * c;
            q = EUC ? 0.5 * c : 0.0;
        } else {
            p = EUC ? c * c : c;
            q = EUC ? 2.0 * c : 0.0;
        }
        if (EUC) p = p * (1.0 + rho);
    } else {
        good = a > 0.0 && tau >= 0.0;
        double s = tau;   // d <= s sqrt(a) sqrt(b)  /  d^2 <= s a b
        if (KIND == KZ_RANK_LS) {
            good = good && tau <= 1.0 - rho;
            s = -log1p(-tau) * (1.0 + rho) + 9.313225746154785e-10 /* 2^-30 */;
            q = EUC ? s * a : sqrt(s * a);
        } else {
            q = EUC ? tau * tau * a : tau * sqrt(a);
        }
        q = q * (1.0 + rho);
    }
    p += rho * fabs(q) * umax + tiny;
    *P = p;
    *Q = q;
    *ok = good && fabs(p) < (double)INFINITY && fabs(q) < (double)INFINITY && fabs(tau) < (double)INFINITY;
}
template <int KIND, bool EUC>
__device__ __forceinline__ void kz_r1_index_form(double b, double* U, double* V, bool* ok) {
    const double rho = KZ_R1_RHO;
    double u = 0.0, v = 0.0;
    bool good = fabs(b) < (double)INFINITY;
    if (KIND == KZ_RANK_CSLS || KIND == KZ_RANK_DUAL) {
        const double bw = b + rho * fabs(b);
        if (KIND == KZ_RANK_CSLS)
            v = EUC ? 0.25 * bw * bw * (1.0 + rho) : 0.5 * bw;
        else
            v = EUC ? bw * bw * (1.0 + rho) : bw;
        u = EUC ? bw : 0.0;
    } else {
        good = good && b > 0.0;
        u = EUC ? b : sqrt(b);
    }
    *U = u;
    *V = v;
    *ok = good && fabs(u) < (double)INFINITY && fabs(v) < (double)INFINITY;
}

// One wave per seed pair (r, s): seed_w [r k_seed + s] = the exact w of (query row q_begin + r, index row seed[r, s]); an id outside
// the index gives NaN (ranked as +inf: no seed).
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_r1_seed_w_kernel(const int64_t* __restrict__ seed, long long n_pairs, int k_seed, int64_t q_begin,
                                                           const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                           const double* __restrict__ qsqn, const double* __restrict__ ysqn, int64_t n_i, int d,
                                                           int metric, double mp, const double* __restrict__ q_a, const double* __restrict__ t_a,
                                                           double* __restrict__ seed_w) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_pairs; e += n_waves) {
        const int64_t j = seed[e];
        if (j < 0 || j >= n_i) {   // (wave-uniform)
            if (lane == 0) seed_w[e] = NAN;
            continue;
        }
        const int64_t r = e / k_seed, qrow = q_begin + r;
        const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + j * (int64_t)d, qsqn[qrow], ysqn[j], d, metric, lane);
        if (lane == 0) seed_w[e] = kz_rank_reduce<T, KIND, METRIC>(v, mp, q_a[r], 0.0, t_a[j], 0.0);
    }
}

// One wave per query row r.  seed_key [r, s] = the order key of seed s's w, KZ_KNNR_PAD for an id outside the index or one that an
// earlier seed of the row names too; tau [r] = the w of the row's k-th smallest (key, seed place) -- NaN / +inf (fewer than k valid,
// distinct seeds, or a w that is not finite) raises the fallback flag.
__global__ __launch_bounds__(256) void kz_r1_tau_kernel(const int64_t* __restrict__ seed, const double* __restrict__ seed_w, int n_rows, int k_seed,
                                                        int k, int64_t n_i, unsigned long long* __restrict__ seed_key, double* __restrict__ tau,
                                                        int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = r < n_rows;
    const int64_t* sd = seed + (int64_t)(live ? r : 0) * k_seed;
    const double* sw = seed_w + (int64_t)(live ? r : 0) * k_seed;
    unsigned long long* sk = seed_key + (int64_t)(live ? r : 0) * k_seed;
    if (live) {
        for (int s = lane; s < k_seed; s += 64) {
            const int64_t j = sd[s];
            bool dead = j < 0 || j >= n_i;
            for (int t = 0; t < s && !dead; ++t) dead = sd[t] == j;
            sk[s] = dead ? KZ_KNNR_PAD : kz_knnr_key(sw[s]);
        }
    }
    __syncthreads();   // (the keys of the row, written by this wave: visible to all of its lanes)
    if (!live) return;
    bool found = false;
    for (int s = lane; s < k_seed; s += 64) {
        const unsigned long long key = sk[s];
        int before = 0;
        for (int t = 0; t < k_seed; ++t) {
            const unsigned long long kt = sk[t];
            before += kt < key || (kt == key && t < s) ? 1 : 0;
        }
        if (before == k - 1) {
            const double w = key == KZ_KNNR_PAD ? (double)INFINITY : sw[s];
            tau[r] = w;
            if (!(fabs(w) < (double)INFINITY)) atomicOr(flag, KZ_R1_F_INVALID);
            found = true;
        }
    }
    (void)found;
}

// One workgroup of 128 threads per index tile: row j = tile x 128 + thread.  bias2 [j] = fl(bias[j] + h V_j / scale), yu [j] = fl(U_j),
// the float64 V (key units) and U for the resolve kernel, per tile {min, max} of the real rows' float U, and the launch's maxima
// gmax[0] = max |U| (float bits), gmax[1] = max |bias2| (float bits: non-negative floats order as integers).
template <int KIND, bool EUC>
__global__ __launch_bounds__(128) void kz_r1_index_kernel(const float* __restrict__ bias, const double* __restrict__ t_a, int64_t n_i, double h,
                                                          const double* __restrict__ hscale, float* __restrict__ bias2, float* __restrict__ yu,
                                                          double* __restrict__ vkey, double* __restrict__ ud, float2* __restrict__ urange,
                                                          unsigned* __restrict__ gmax, int* __restrict__ flag) {
    __shared__ float s_min[2], s_max[2], s_ua[2], s_wa[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j = (int64_t)blockIdx.x * KZ_TILE + tid;
    float bf = bias[j], uf = 0.0f;
    float umin = INFINITY, umax = -INFINITY, ua = 0.0f, wa = 0.0f;
    if (j < n_i) {
        double U, V;
        bool ok;
        kz_r1_index_form<KIND, EUC>(t_a[j], &U, &V, &ok);
        const double vk = h * V;
        bf = (float)((double)bf + vk / hscale[1]);
        uf = (float)U;
        ok = ok && fabsf(bf) < INFINITY && fabsf(uf) < INFINITY;
        if (!ok) atomicOr(flag, KZ_R1_F_INVALID);
        vkey[j] = vk;
        ud[j] = U;
        umin = umax = uf;
        ua = fabsf(uf);
        wa = fabsf(bf);
    }
    bias2[j] = bf;
    yu[j] = uf;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        umin = fminf(umin, __shfl_xor(umin, o, 64));
        umax = fmaxf(umax, __shfl_xor(umax, o, 64));
        ua = fmaxf(ua, __shfl_xor(ua, o, 64));
        wa = fmaxf(wa, __shfl_xor(wa, o, 64));
    }
    if (lane == 0) {
        s_min[wave] = umin;
        s_max[wave] = umax;
        s_ua[wave] = ua;
        s_wa[wave] = wa;
    }
    __syncthreads();
    if (tid == 0) {
        umin = fminf(s_min[0], s_min[1]);
        umax = fmaxf(s_max[0], s_max[1]);
        if (!(umin <= umax)) umin = umax = 0.0f;   // (a NaN state: the flag is up, the sweep does not run)
        urange[blockIdx.x] = make_float2(umin, umax);
        ua = fmaxf(s_ua[0], s_ua[1]);
        wa = fmaxf(s_wa[0], s_wa[1]);
        if (ua == ua) atomicMax(gmax, __float_as_uint(ua));
        if (wa == wa) atomicMax(gmax + 1, __float_as_uint(wa));
    }
}

// One thread per query row r of the image (row q_begin + r of the query): pq [r] = {P', Q'} in the image's key units, E [r] the
// bound, qd [r] = h Q in exact key units (for the resolve kernel).  Pad rows: {+inf, 0}.
template <int KIND, bool EUC>
__global__ __launch_bounds__(256) void kz_r1_query_kernel(int64_t n_rows, int64_t n_pad, int64_t q_begin, const double* __restrict__ qsqn, int metric,
                                                          const double* __restrict__ tau, const double* __restrict__ q_a,
                                                          const double* __restrict__ rowq, const double* __restrict__ y_hmax,
                                                          const double* __restrict__ hscale, const double* __restrict__ ystats, double eps_mult,
                                                          double gamma_acc, const unsigned* __restrict__ gmax, float2* __restrict__ pq,
                                                          double* __restrict__ e_out, double* __restrict__ qd, int* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pad) return;
    if (r >= n_rows) {
        pq[r] = make_float2(INFINITY, 0.0f);
        return;
    }
    const double scale = hscale[1], h = metric == KZ_COSINE ? 1.0 : 0.5;
    const double umax = (double)__uint_as_float(gmax[0]), W = (double)__uint_as_float(gmax[1]) * scale;
    const double qs = qsqn[q_begin + r];
    const double qc2 = rowq[r * 3];
    const double eps = kz_h_key_eps(rowq + r * 3, y_hmax, ystats, metric == KZ_COSINE ? 0.0 : qs, metric, eps_mult, gamma_acc);
    double P, Q;
    bool ok;
    kz_r1_query_form<KIND, EUC>(tau[r], q_a[r], umax, &P, &Q, &ok);
    const double hq = h * Q;
    const double E = eps + eps_mult * ((gamma_acc + 1.1920928955078125e-07 /* 2^-23 */) * W + 1.788139343261719e-07 /* 3 x 2^-24 */ * fabs(hq) * umax);
    const double want = (0.5 * qc2 - h * P - E) / scale;
    const float pf = kz_round_below(want);
    const float qf = (float)(hq / scale);
    ok = ok && fabs(qs) < (double)INFINITY && fabs(E) < (double)INFINITY && fabsf(pf) < INFINITY && fabsf(qf) < INFINITY;
    e_out[r] = E;
    qd[r] = hq;
    if (!ok) {
        pq[r] = make_float2(INFINITY, 0.0f);
        atomicOr(flag, KZ_R1_F_INVALID);
        return;
    }
    pq[r] = make_float2(pf, qf);
}

// One wave per place e of the ordered log: entry pos[e] = {query row, index row, t}.  Its exact w, the w's order key and the index
// row go to place e; the bound checks itself: |t scale - (key + V_j + hQ_i U_j)| / E_i <= 1, the largest ratio is kept.
// An entry on a pad index row (bias -inf) or a pad query row (P' = +inf) never occurs; it would get the pad key, not be read.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_r1_resolve_kernel(const i32x2e* __restrict__ log_meta, const float* __restrict__ log_key,
                                                            const int* __restrict__ pos, long long n_entries, int n_rows, int64_t q_begin,
                                                            const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                            const double* __restrict__ qsqn, const double* __restrict__ ysqn, int64_t n_i, int d,
                                                            int metric, double mp, const double* __restrict__ q_a, const double* __restrict__ t_a,
                                                            const double* __restrict__ rowq, const double* __restrict__ hscale,
                                                            const double* __restrict__ E, const double* __restrict__ qd,
                                                            const double* __restrict__ vkey, const double* __restrict__ ud, int* __restrict__ flag,
                                                            unsigned long long* __restrict__ max_ratio_bits, double* __restrict__ w_out,
                                                            unsigned long long* __restrict__ key_out, int* __restrict__ idx_out) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_entries; e += n_waves) {
        const long long at = pos[e];
        const i32x2e mt = log_meta[at];
        const int q = mt.x;
        const int64_t j = mt.y;
        if (j < 0 || j >= n_i || q < 0 || q >= n_rows) {   // (wave-uniform)
            if (lane == 0) {
                w_out[e] = INFINITY;
                key_out[e] = KZ_KNNR_PAD;
                idx_out[e] = 0x7fffffff;
            }
            continue;
        }
        const int64_t qrow = q_begin + q;
        const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + j * (int64_t)d, qsqn[qrow], ysqn[j], d, metric, lane);
        if (lane == 0) {   // (every lane holds v; the wave meets again at the next entry's butterfly)
            const double w = kz_rank_reduce<T, KIND, METRIC>(v, mp, q_a[q], 0.0, t_a[j], 0.0);
            const double key = 0.5 * (rowq[(int64_t)q * 3] - (metric == KZ_COSINE ? 2.0 * v : v));
            const double lhs = key + vkey[j] + qd[q] * ud[j];
            if (!kz_bound_holds((double)log_key[at] * hscale[1], lhs, E[q], max_ratio_bits)) atomicOr(flag, KZ_R1_F_VIOLATED);
            w_out[e] = w;
            key_out[e] = kz_knnr_key(w);
            idx_out[e] = (int)j;
        }
    }
}

// One wave per query row q over the ordered log (row_key ascending; within a row ascending by index row): its run [a, b) by two
// binary searches.  An entry whose key is <= key(tau_q) takes the place = the number of the run's entries before it by (key, index
// row) -- a count, no order of execution in it -- and, with a place below k, is written.  The row's own check: at least k such
// entries, and every seed with key <= key(tau_q) is an index row of the run.
__global__ __launch_bounds__(256) void kz_r1_select_kernel(const int* __restrict__ row_key, int n, int n_rows, int k, const double* __restrict__ tau,
                                                           const double* __restrict__ w_in, const unsigned long long* __restrict__ key_in,
                                                           const int* __restrict__ idx_in, const int64_t* __restrict__ seed,
                                                           const unsigned long long* __restrict__ seed_key, int k_seed, int* __restrict__ flag,
                                                           double* __restrict__ d_w, int64_t* __restrict__ d_ind) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;   // (wave-uniform)
    const int a = kz_run_lower(row_key, n, q), b = kz_run_lower(row_key, n, q + 1);
    const unsigned long long tk = kz_knnr_key(tau[q]);
    int under = 0;   // (uniform)
    for (int e0 = a; e0 < b; e0 += 64) {   // (uniform)
        const int e = e0 + lane;
        const bool in = e < b && key_in[e] <= tk;
        under += __popcll(__ballot(in));
        if (in) {
            const unsigned long long key = key_in[e];
            int place = 0;
            for (int t = a; t < b && place < k; ++t) {
                const unsigned long long kt = key_in[t];
                place += kt < key || (kt == key && t < e) ? 1 : 0;
            }
            if (place < k) {
                d_w[(int64_t)q * k + place] = w_in[e];
                d_ind[(int64_t)q * k + place] = idx_in[e];
            }
        }
    }
    bool bad = under < k;
    for (int s = lane; s < k_seed; s += 64) {
        if (seed_key[(int64_t)q * k_seed + s] > tk) continue;
        const int j = (int)seed[(int64_t)q * k_seed + s];
        int lo = a, hi = b;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (idx_in[mid] < j)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (!(lo < b && idx_in[lo] == j)) bad = true;
    }
    if (bad) atomicOr(flag, KZ_R1_F_VIOLATED);
}

// (kind, metric) -> f(KzRankC<KIND>, bool_constant<EUC>) for the four rank-one kinds
template <typename F>
static void kz_r1_dispatch(int kind, int metric, F f) {
    auto by_metric = [&](auto kd) {
        if (metric == KZ_EUCLIDEAN)
            f(kd, std::true_type());
        else
            f(kd, std::false_type());
    };
    switch (kind) {
        case KZ_RANK_CSLS: by_metric(KzRankC<KZ_RANK_CSLS>()); break;
        case KZ_RANK_LS: by_metric(KzRankC<KZ_RANK_LS>()); break;
        case KZ_RANK_NICDM: by_metric(KzRankC<KZ_RANK_NICDM>()); break;
        default: by_metric(KzRankC<KZ_RANK_DUAL>()); break;
    }
}

// The sweep route.  *done = 0: nothing the caller may keep was decided -- the exact route rewrites every output.
static int kz_knn_reduced_sweep_run(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, int k, int kind,
                                    const double* d_q_a, const double* d_t_a, const int64_t* d_seed, int k_seed, double* d_w, int64_t* d_ind,
                                    kz_knn_reduced_sweep_stats* st, int* done) {
    *done = 0;
    const int d = (int)index->d, metric = index->metric;
    const int n_rows = (int)q_count;
    const double mp = index->mink_p;
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    KzSweepQuery qs;
    int rc = qs.init(ctx, query, q_begin, n_rows, nullptr, index);
    if (rc != KZ_OK) return rc;
    const int n_ytiles = (int)index->n_tiles;
    const int64_t n_pad = qs.n_pad, y_pad = (int64_t)n_ytiles * KZ_TILE;
    // ---- buffers --------------------------------------------------------------------------------------------------------------------
    const size_t n_seed = (size_t)n_rows * k_seed;
    KzSweepLog log;            // counters: [4] flags, [6..7] max |U|, max |bias'| (float bits); no extras
    KzPoolBuf<double> dq;      // tau [n_rows] | E [n_rows] | hQ [n_rows] | seed_w [n_seed]
    KzPoolBuf<double> dy;      // V key [y_pad] | U [y_pad]
    KzPoolBuf<unsigned long long> seed_key;
    KzPoolBuf<float> fy;       // bias' [y_pad] | U [y_pad]
    KzPoolBuf<float2> urange, pq;
    rc = log.alloc(ctx, 4ll * k > KZ_CERT_LOG_PER_ROW ? 4ll * k : KZ_CERT_LOG_PER_ROW, n_rows, true, 0);
    if (rc == KZ_OK) rc = dq.alloc(ctx, (3 * (size_t)n_rows + n_seed) * sizeof(double));
    if (rc == KZ_OK) rc = dy.alloc(ctx, 2 * (size_t)y_pad * sizeof(double));
    if (rc == KZ_OK) rc = seed_key.alloc(ctx, n_seed * 8);
    if (rc == KZ_OK) rc = fy.alloc(ctx, 2 * (size_t)y_pad * sizeof(float));
    if (rc == KZ_OK) rc = urange.alloc(ctx, (size_t)n_ytiles * sizeof(float2));
    if (rc == KZ_OK) rc = pq.alloc(ctx, (size_t)n_pad * sizeof(float2));
    if (rc != KZ_OK) return rc;
    unsigned long long* counters = log.counters();
    int* flag = log.words.get() + 4;
    unsigned* gmax = (unsigned*)(log.words.get() + 6);
    double *tau = dq.get(), *E = tau + n_rows, *qd = E + n_rows, *seed_w = qd + n_rows;
    double *vkey = dy.get(), *ud = vkey + y_pad;
    float *bias2 = fy.get(), *yu = bias2 + y_pad;
    const float* yraw = (const float*)index->raw;
    const float* qraw = (const float*)query->raw;
    const kz_himage *qi = qs.m->himg, *ii = index->himg;
    const double* hscale = (const double*)ii->center->d_scale;
    hipLaunchKernelGGL(kz_radius_clear_kernel, dim3(1), dim3(256), 0, ctx->stream, log.words.get(), (int64_t)log.n_words);
    // ---- tau from the seeds; the index side, then the query side of the threshold ---------------------------------------------------
    {
        const long long wgs = ((long long)n_seed + 3) / 4;
        kz_rank_dispatch(kind, index, [&](auto t, auto kd, auto mt) {
            hipLaunchKernelGGL((kz_r1_seed_w_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(mt)::value>),
                               dim3((unsigned)(wgs < 65536 ? wgs : 65536)), dim3(256), 0, ctx->stream, d_seed, (long long)n_seed, k_seed, q_begin, qraw, yraw,
                               (const double*)query->sqn, (const double*)index->sqn, index->n, d, metric, mp, d_q_a, d_t_a, seed_w);
        });
        hipLaunchKernelGGL(kz_r1_tau_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, d_seed, (const double*)seed_w, n_rows, k_seed, k,
                           index->n, seed_key.get(), tau, flag);
        KZ_HIP(hipGetLastError());
    }
    kz_r1_dispatch(kind, metric, [&](auto kd, auto euc) {
        constexpr int KD = decltype(kd)::value;
        constexpr bool EUC = decltype(euc)::value;
        hipLaunchKernelGGL((kz_r1_index_kernel<KD, EUC>), dim3((unsigned)n_ytiles), dim3(128), 0, ctx->stream, (const float*)ii->bias, d_t_a, index->n,
                           metric == KZ_COSINE ? 1.0 : 0.5, hscale, bias2, yu, vkey, ud, urange.get(), gmax, flag);
        hipLaunchKernelGGL((kz_r1_query_kernel<KD, EUC>), dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)n_rows, n_pad, q_begin,
                           (const double*)query->sqn, metric, (const double*)tau, d_q_a, (const double*)qi->rowq, (const double*)ii->d_max, hscale,
                           (const double*)index->d_stats, ctx->eps_scale, kz_gamma_acc_h(index->kg), (const unsigned*)gmax, pq.get(), E, qd, flag);
    });
    KZ_HIP(hipGetLastError());
    // a state that makes the form invalid: known before the sweep, which then does not run
    int h_flag = 0;
    KZ_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    st->n_rows = n_rows;
    if (h_flag) return KZ_OK;
    // ---- the sweep ------------------------------------------------------------------------------------------------------------------
    const int n_slices = index->kg / 4;
    const KzCountKernel kern = kz_cert_lookup(n_slices, kz_emit_r1_lookup_lo, kz_emit_r1_lookup_hi);
    KzSweepWork work;
    rc = kz_cert_plan(who, ctx, kern, "sweep", n_slices, qs.n_qtiles, n_ytiles, &work);
    if (rc != KZ_OK) return rc;
    KnnEmitR1Params ep;
    memset(&ep, 0, sizeof(ep));
    ep.qpack = (const float*)qi->packed;
    ep.ypack = (const float*)ii->packed;
    ep.ybias = bias2;
    ep.yu = yu;
    ep.urange = urange.get();
    ep.work = work.d_work.get();
    ep.n_ytiles = n_ytiles;
    ep.pq = pq.get();
    ep.log_cnt = counters;
    ep.log_cap = log.cap;
    ep.log_meta = log.meta.get();
    ep.log_key = log.key.get();
    rc = kz_cert_launch(ctx, kern, ep, work.pl.W);
    if (rc != KZ_OK) return rc;
    KzSweepCounters hc;
    rc = kz_cert_sweep_done(ctx, who, log, &hc, st);
    if (rc != KZ_OK || st->overflowed) return rc;
    const int n = (int)hc.n_log;
    if (n < n_rows) return KZ_OK;   // (fewer entries than rows: some row lacks its own seeds -- the row check would say so)
    // ---- order the log by (query row, index row); exact w of every entry; the k smallest of every row ---------------------------
    KzLogOrder ord;
    KzPoolBuf<int> idx;
    KzPoolBuf<double> wbuf;
    KzPoolBuf<unsigned long long> kbuf;
    rc = kz_cert_order_log(ctx, log.meta.get(), n, &ord);
    if (rc == KZ_OK) rc = idx.alloc(ctx, (size_t)n * 4);
    if (rc == KZ_OK) rc = wbuf.alloc(ctx, (size_t)n * 8);
    if (rc == KZ_OK) rc = kbuf.alloc(ctx, (size_t)n * 8);
    if (rc != KZ_OK) return rc;
    {
        const long long wgs = ((long long)n + 3) / 4;
        kz_rank_dispatch(kind, index, [&](auto t, auto kd, auto mt) {
            hipLaunchKernelGGL((kz_r1_resolve_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(mt)::value>),
                               dim3((unsigned)(wgs < 65536 ? wgs : 65536)), dim3(256), 0, ctx->stream, (const i32x2e*)log.meta.get(), (const float*)log.key.get(),
                               ord.pos(), (long long)n, n_rows, q_begin, qraw, yraw, (const double*)query->sqn, (const double*)index->sqn, index->n, d,
                               metric, mp, d_q_a, d_t_a, (const double*)qi->rowq, hscale, (const double*)E, (const double*)qd, (const double*)vkey,
                               (const double*)ud, flag, counters + 1, wbuf.get(), kbuf.get(), idx.get());
        });
    }
    hipLaunchKernelGGL(kz_r1_select_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, ord.row_key(), n, n_rows, k, (const double*)tau,
                       (const double*)wbuf.get(), (const unsigned long long*)kbuf.get(), (const int*)idx.get(), d_seed,
                       (const unsigned long long*)seed_key.get(), k_seed, flag, d_w, d_ind);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    rc = log.read(ctx, who, "resolving the log", &hc);
    if (rc != KZ_OK) return rc;
    memcpy(&st->max_err_ratio, &hc.ratio_bits, 8);
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    st->resolve_ms = ms;
    if (hc.flag) return KZ_OK;   // (a violated bound or row check: nothing of the above is trusted)
    *done = 1;
    return KZ_OK;
}

extern "C" int kz_knn_reduced_sweep(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c, int k, int kind,
                                    const double* d_q_a, const double* d_q_b, const double* d_t_a, const double* d_t_b, const int64_t* d_seed_ind,
                                    int k_seed, double* d_w, int64_t* d_ind, kz_knn_reduced_sweep_stats* stats) {
    const char* who = "kz_knn_reduced_sweep";
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair(who, ctx, query, q_begin, q_count, index, d_w, d_ind);
    if (rcp != KZ_OK) return rcp;
    kz_knn_reduced_sweep_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    // (the requirements of kz_knn_reduced, in its words: the two routes refuse the same calls)
    KZ_REQUIRE(k >= 1 && k <= index->n, "%s: Expected n_neighbors <= n_samples_fit and >= 1, but n_neighbors = %d, n_samples_fit = %lld", who, k,
               (long long)index->n);
    if (k > KZ_KNN_REDUCED_MAX_K) {
        kz_set_error("%s: k = %d exceeds the maximum of %d neighbours per query (beyond it, kz_gold_ranks_reduced ranks any row)", who, k,
                     KZ_KNN_REDUCED_MAX_K);
        return KZ_ERR_UNSUPPORTED;
    }
    const int rcr = kz_rank_require_reduction(who, kind, d_q_a, d_q_b, d_t_a, d_t_b);
    if (rcr != KZ_OK) return rcr;
    KZ_REQUIRE(d_seed_ind && k_seed >= k, "%s: d_seed_ind [q_count, k_seed] with k_seed >= k is required, got k_seed = %d, k = %d", who, k_seed, k);
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    int done = 0;
    if (kind != KZ_RANK_MP_NORMAL && k <= KZ_R1_MAX_K && k_seed <= KZ_R1_MAX_SEEDS && (long long)q_count * k_seed < 0x7fffffffLL &&
        kz_rank_sweep_shapes_ok(ctx, query, index)) {
        const int rc = kz_knn_reduced_sweep_run(who, ctx, query, q_begin, q_count, index, k, kind, d_q_a, d_t_a, d_seed_ind, k_seed, d_w, d_ind, &st, &done);
        if (rc != KZ_OK) return rc;
    }
    if (done) {
        st.route_taken = 1;
    } else {
        const int rc = kz_cert_exact_route(ctx, &st.fallback_ms, [&] {
            return kz_knn_reduced(ctx, query, q_begin, q_count, index, k, kind, d_q_a, d_q_b, d_t_a, d_t_b, d_w, d_ind);
        });
        if (rc != KZ_OK) return rc;
        st.n_rows = q_count;
    }
    if (stats) *stats = st;
    return KZ_OK;
}
