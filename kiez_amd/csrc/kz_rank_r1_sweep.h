// REDUCED GOLD RANKS ON THE fp16 COUNT SWEEP (kz_gold_ranks_reduced_sweep, opt-in): the ranks of kz_gold_ranks_reduced -- the same
// integers on every row -- with the float64 value matrix replaced by a first pass on the fp16 MFMA sweep.
// The fast pass only decides WHICH pairs need the exact w (section 4).  kz_gold_ranks_sweep's steps, under a rank-one threshold:
//   1. kz_r1_index_kernel (kz_knn_reduced_sweep.h, unchanged): the index side of the forms -- V folded into a copy of the image's bias
//      row, U, per-tile Umin / Umax; kz_rank_r1_extent_kernel: max |V| over the index;
//   2. kz_rank_r1_query_kernel: per listed row tau_i = the exact w of its gold pair (kz_exact_value + kz_rank_reduce: the exact
//      route's expression and bits) and the two edges {P_lo', P_hi'} with Q' in key units (below);
//   3. kz_knn_count_r1_h_kernel (kz_knn_cnt_r1_16.h): counts t > P_hi' into d_rank, logs P_lo' <= t <= P_hi' -- the band;
//   4. kz_rank_r1_resolve_kernel: the exact w of every band entry, compared with (w_g, g) by the rule of kz_rank_before; the bound
//      checks itself on every entry;
//   5. kz_rank_fallback_kernel (kz_rank_sweep.h, unchanged): rows that are not trusted -- a tau or an edge that is not finite or lies
//      outside a form's domain, a band beyond the per-row cap, a violated bound, a gold row that did not show up in its own band,
//      every row when the log overflowed -- are reset and go through the exact walk (kz_gold_ranks_walk with the reduction).
// The WHOLE call takes kz_gold_ranks_reduced's route -- route_taken = 0, never an error -- for a shape outside the sweep
// (kz_rank_sweep_shapes_ok), KZ_RANK_MP_NORMAL (not rank one) and a STATE outside a form's domain (an entry that is not finite;
// NICDM / LS: an entry <= 0).
//
// THE LOW EDGE is the reduced-list sweep's Pf at tau_i (kz_knn_reduced_sweep.h "THE FORMS", "THE KEY-UNIT BOUND"): the outward form
//     w_ij <= tau_i   =>   v_ij <= P + Q U_j + V_j =: B_out(j)
// lowered by E_i.  So t < P_lo' implies v > B_out(j), hence w_j > w_g: surely farther, ties excluded.
//
// THE INWARD FORMS (the high edge).  t > P_hi' must imply w_j < w_g STRICTLY.  With rho = 2^-20, u = 2^-24, ma = |tau| + |a| and
// every widening of THE FORMS turned inward:
//   CSLS (s = 2) / DUAL (s = 1):   s d < c_in + b_in,  c_in = tau + a - rho ma,  b_in = b - rho |b|   =>   w < tau.
//       (d >= 0: kz_exact_value clamps.  The two float64 roundings of w are below 6 x 2^-53 M with M = ma + |b|, and s d < M under
//        the premise, so w < tau - rho M + 6 x 2^-53 M <= tau; M = 0 admits no d.)
//   NICDM:   d < tau sqrt(a) sqrt(b) (1 - 2^-48)   =>   w < tau        (three roundings of w, two of the square roots)
//   LS:      d^2 < L_in a b,  L_in = -log1p(-tau) (1 - rho) - 2^-30   =>   w < tau
//       (exp(-z (1 + 3 x 2^-53)) >= (1 - tau)(1 + 2^-30) for z below L_in; 1 - tau >= 2^-20 in the form's domain, so the margin
//        2^-51 is above the roundings of exp and of the subtraction.  L_in <= 0: no pair is surely closer.)
//   euclidean (d = fl32 sqrt fl32 v):   D >= 0 and v < D^2 (1 - 8 u) - 2^-140   =>   d < D     (kz_radius_band_kernel's bracket)
// THE GAP.  The index-side images U_j, V_j and the one Q' of a row are SHARED with the low edge and outward-widened, so the kernel
// tests v < P_hi + Q U_j + V_j with the outward Q, U, V.  P_hi = P_out - G_i with G_i >= max over index rows of
// B_out(j) - B_in(j) makes that imply the inward form for every j.  In the magnitudes a row knows (umax = max |U|,
// vmax = max |V| over the index: kz_r1_index_kernel, kz_rank_r1_extent_kernel):
//   CSLS / DUAL, d = v:   B_out - B_in = (c_out - c_in + b_out - b_in) / s <= 2 rho (ma + bmax) / s,  bmax = s vmax (1 + 2 rho)
//   NICDM / LS:           B_out - B_in = P_out + (Q_out - Q_in) U_j <= P_out + (Q_out - Q_in) umax    (U is not widened, U >= 0)
//   CSLS / DUAL, euclidean:   B(j) = (x_j / s)^2 with x_j = c + b_j, outward x_j, inward y_j = x_j - delta_j,
//       delta_j = 2 rho (ma + |b_j|) <= dmax.  Rows with y_j > 0:  x^2 - y^2 <= 2 dmax |x| <= 2 dmax (|c| + umax), plus rho umax^2 for
//       V's widening and 8 u (|c| + umax)^2 for the bracket: G_i.  Rows with y_j <= 0 have NO d below their bound, but the square of
//       the outward form admits them -- harmless at the low edge (a superset), fatal at the high one: no shift of P_hi that is worth
//       having excludes them (it would have to be the square of the most negative x_j: a band as wide as the index).  They are told
//       apart PER ELEMENT, by U_j = b'_j alone: the row carries two more numbers, and the kernel
//         drops an element with U_j < U_far  = -c_out - 2^-22 umax:  x_j < 0, the OUTWARD bound is negative, no d >= 0 gives
//                                                                   w_j <= tau: surely farther whatever its key;
//         counts an element only with U_j > U_good = -c_in + 2 rho (1 + 2 rho) umax + 2^-22 umax:  y_j > 0, the premise of G_i;
//         and can only LOG what lies between the two (a sliver of width ~ rho).
//       (2^-22 umax: twice the float conversions of U_j and of the threshold, which is rounded outward and one step further.)
//       The other forms pass -inf for both.
// G_i and E_i go into P_hi' together: P_hi' = (qc2 / 2 - h (P_out - G_i) + E_i) / scale, rounded UP and one float step further.
// TIES.  A pair with w_j == w_g satisfies neither strict implication: it is in the band and the resolve kernel orders it by row --
// the gold pair itself among them (KZ_RANK_F_GOLD_SEEN), which is the row's own check that its band was logged.
#pragma once
#include "kz_knn_cnt_r1_16.h"
#include "kz_cert_sweep.h"

// One workgroup: ext[0] = max |V| in key units (vkey) over the real rows.
__global__ __launch_bounds__(256) void kz_rank_r1_extent_kernel(const double* __restrict__ vkey, int64_t n_i, double* __restrict__ ext) {
    __shared__ double s_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double vmax = 0.0;
    for (int64_t j = tid; j < n_i; j += 256) vmax = fmax(vmax, fabs(vkey[j]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o, 64));
    if (lane == 0) s_max[wave] = vmax;
    __syncthreads();
    if (tid == 0) ext[0] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
}

// P_hi in value units ("THE GAP" above) and the two thresholds on U (-inf where the form needs none).  p_out, q_out:
// kz_r1_query_form's; umax (already widened by the float conversion); vmax: max |V| in value units.
template <int KIND, bool EUC>
__device__ __forceinline__ double kz_r1_inward_p(double tau, double a, double p_out, double q_out, double umax, double vmax, double* u_good,
                                                  double* u_far) {
    const double rho = KZ_R1_RHO, tiny = 7.174648137343064e-43 /* 2^-140 */, u8 = 4.76837158203125e-07 /* 8 x 2^-24 */;
    double p;
    *u_good = *u_far = -(double)INFINITY;
    if (KIND == KZ_RANK_CSLS || KIND == KZ_RANK_DUAL) {
        const double kap = KIND == KZ_RANK_CSLS ? 0.5 : 1.0, ma = fabs(tau) + fabs(a);
        if (!EUC) {
            const double bmax = vmax / kap * (1.0 + 2.0 * rho);
            const double c_in = tau + a - rho * ma;
            p = kap * (c_in - 4.0 * rho * bmax) - 9.094947017729282e-13 /* 2^-40 */ * kap * (ma + bmax) - tiny;
        } else {
            const double c = tau + a + rho * ma;
            const double dmax = 2.0 * rho * (1.0 + 2.0 * rho) * (ma + umax);
            const double s = fabs(c) + umax;
            const double ga = kap * kap * (2.0 * dmax * s + rho * umax * umax + u8 * s * s);
            p = kap * kap * c * c - 2.0 * ga - tiny;
            // the rows this bound may be used on / may be dropped on, as thresholds on the float image of U_j = b'_j (within
            // 2^-24 umax of b'_j):  y_j = c_in + b_in,j >= c_in + b'_j - 2 rho (1 + 2 rho) umax > 0 behind u_good;
            // x_j = c + b'_j < 0 before u_far
            const double c_in = tau + a - rho * ma, f24 = 2.384185791015625e-07 /* 2^-22 */ * umax;
            *u_good = -c_in + 2.0 * rho * (1.0 + 2.0 * rho) * umax + f24;
            *u_far = -c - f24;
        }
    } else {
        double q_in;
        if (KIND == KZ_RANK_NICDM) {
            q_in = EUC ? tau * tau * a * (1.0 - 7.105427357601002e-15 /* 2^-47 */) * (1.0 - u8) : tau * sqrt(a) * (1.0 - 3.552713678800501e-15 /* 2^-48 */);
        } else {
            const double l_in = -log1p(-tau) * (1.0 - rho) - 9.313225746154785e-10 /* 2^-30 */;
            if (!(l_in > 0.0))
                q_in = 0.0;
            else
                q_in = EUC ? l_in * a * (1.0 - 7.105427357601002e-15) * (1.0 - u8) : sqrt(l_in * a) * (1.0 - 3.552713678800501e-15);
        }
        q_in = fmax(fmin(q_in, q_out), 0.0);
        p = -((q_out - q_in) * umax * (1.0 + 9.313225746154785e-10) + tiny);
    }
    return fmin(p, p_out);
}

// One wave per listed row r (row list[r] of the call).  wg [r] = tau = the exact w of its gold pair, plq [2 r] = {P_lo', P_hi', Q', 0}, plq [2 r + 1] = {U_good, U_far}
// in the image's key units, E [r] the bound, qd [r] = h Q in exact key units (for the resolve kernel).  A tau or an edge that is not
// finite or outside the form's domain: {+inf, +inf, 0}, {-inf, -inf} and the row's fallback flag.  A query-side STATE outside the domain raises
// gflag (the whole call then takes the exact route).  Pad rows: {+inf, +inf, 0}, no flag.
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_rank_r1_query_kernel(const int* __restrict__ list, int n_list, int64_t n_pad, int64_t q_begin,
                                                               const int64_t* __restrict__ gold, const float* __restrict__ qraw,
                                                               const float* __restrict__ yraw, const double* __restrict__ qsqn,
                                                               const double* __restrict__ ysqn, int d, int metric, double mp,
                                                               const double* __restrict__ q_a, const double* __restrict__ t_a,
                                                               const double* __restrict__ rowq, const double* __restrict__ y_hmax,
                                                               const double* __restrict__ hscale, const double* __restrict__ ystats, double eps_mult,
                                                               double gamma_acc, const unsigned* __restrict__ gmax, const double* __restrict__ ext,
                                                               float4* __restrict__ plq, double* __restrict__ wg, double* __restrict__ e_out,
                                                               double* __restrict__ qd, int* __restrict__ flag, int* __restrict__ gflag) {
    constexpr bool EUC = METRIC == KZ_EUCLIDEAN;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_pad) return;
    if (r >= n_list) {
        if (lane == 0) {
            plq[2 * r] = make_float4(INFINITY, INFINITY, 0.0f, 0.0f);
            plq[2 * r + 1] = make_float4(-INFINITY, -INFINITY, 0.0f, 0.0f);
        }
        return;
    }
    const int row = list[r];
    const int64_t qrow = q_begin + row;
    const int64_t g = gold[row];
    const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + g * (int64_t)d, qsqn[qrow], ysqn[g], d, metric, lane);
    if (lane != 0) return;
    const double a = q_a[row];
    const double tau = kz_rank_reduce<T, KIND, METRIC>(v, mp, a, 0.0, t_a[g], 0.0);
    const double scale = hscale[1], h = metric == KZ_COSINE ? 1.0 : 0.5;
    const double umax = (double)__uint_as_float(gmax[0]), W = (double)__uint_as_float(gmax[1]) * scale;
    const double qs = qsqn[qrow];
    const double qc2 = rowq[r * 3];
    const double eps = kz_h_key_eps(rowq + r * 3, y_hmax, ystats, metric == KZ_COSINE ? 0.0 : qs, metric, eps_mult, gamma_acc);
    double P, Q;
    bool ok;
    kz_r1_query_form<KIND, EUC>(tau, a, umax, &P, &Q, &ok);
    const bool state_ok = fabs(a) < (double)INFINITY && (KIND == KZ_RANK_CSLS || KIND == KZ_RANK_DUAL || a > 0.0);
    if (!state_ok) atomicOr(gflag, KZ_R1_F_INVALID);
    double u_good, u_far;
    const double p_hi = kz_r1_inward_p<KIND, EUC>(tau, a, P, Q, umax * (1.0 + 1.1920928955078125e-07 /* 2^-23 */), ext[0] / h, &u_good, &u_far);
    const float ug = kz_round_above(u_good), uf = kz_round_below(u_far);   // (-inf stays)
    const double hq = h * Q;
    const double E = eps + eps_mult * ((gamma_acc + 1.1920928955078125e-07 /* 2^-23 */) * W + 1.788139343261719e-07 /* 3 x 2^-24 */ * fabs(hq) * umax);
    const double want_lo = (0.5 * qc2 - h * P - E) / scale, want_hi = (0.5 * qc2 - h * p_hi + E) / scale;
    const float lo = kz_round_below(want_lo), hi = kz_round_above(want_hi);
    const float qf = (float)(hq / scale);
    ok = ok && state_ok && fabs(tau) < (double)INFINITY && fabs(qs) < (double)INFINITY && fabs(E) < (double)INFINITY && fabsf(lo) < INFINITY &&
         fabsf(hi) < INFINITY && fabsf(qf) < INFINITY && lo <= hi;
    wg[r] = tau;
    e_out[r] = E;
    qd[r] = hq;
    ok = ok && ug == ug && uf == uf && ug < INFINITY;
    if (!ok) flag[r] = KZ_RANK_F_NONFINITE;
    plq[2 * r] = ok ? make_float4(lo, hi, qf, 0.0f) : make_float4(INFINITY, INFINITY, 0.0f, 0.0f);
    plq[2 * r + 1] = ok ? make_float4(ug, uf, 0.0f, 0.0f) : make_float4(-INFINITY, -INFINITY, 0.0f, 0.0f);
}

// One wave per band entry {listed row q, index row j, t}: the pair's exact w; +1 for the row when (w_j, j) orders before (w_g, g) --
// NaN as +inf by row, the exact route's order; the gold row itself adds nothing -- and the bound's own check
// |t scale - (key + h V_j + h Q_i U_j)| / E_i <= 1 with the exact key and the float64 V, U, Q.  Entries of rows beyond the per-row cap
// are skipped (the row falls back).
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_rank_r1_resolve_kernel(const i32x2e* __restrict__ log_meta, const float* __restrict__ log_key, long long n_entries,
                                                                 const int* __restrict__ list, int64_t q_begin, const int64_t* __restrict__ gold,
                                                                 const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                                 const double* __restrict__ qsqn, const double* __restrict__ ysqn, int64_t n_i, int d,
                                                                 int metric, double mp, const double* __restrict__ q_a, const double* __restrict__ t_a,
                                                                 const double* __restrict__ rowq, const double* __restrict__ hscale,
                                                                 const double* __restrict__ wg, const double* __restrict__ E,
                                                                 const double* __restrict__ qd, const double* __restrict__ vkey,
                                                                 const double* __restrict__ ud, const int* __restrict__ band_cnt, int* __restrict__ flag,
                                                                 unsigned long long* __restrict__ max_ratio_bits, int64_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_entries; e += n_waves) {
        const i32x2e mt = log_meta[e];
        const int q = mt.x;
        const int64_t j = mt.y;
        if (j < 0 || j >= n_i || band_cnt[q] > KZ_RANK_BAND_ROW_CAP) continue;   // (wave-uniform)
        const int row = list[q];
        const int64_t qrow = q_begin + row, g = gold[row];
        const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + j * (int64_t)d, qsqn[qrow], ysqn[j], d, metric, lane);
        if (lane == 0) {   // (every lane holds v; the wave meets again at the next entry's butterfly)
            const double w = kz_rank_reduce<T, KIND, METRIC>(v, mp, q_a[row], 0.0, t_a[j], 0.0);
            const double key = 0.5 * (rowq[(int64_t)q * 3] - (metric == KZ_COSINE ? 2.0 * v : v));
            const double lhs = key + vkey[j] + qd[q] * ud[j];
            int f = j == g ? KZ_RANK_F_GOLD_SEEN : 0;
            if (!kz_bound_holds((double)log_key[e] * hscale[1], lhs, E[q], max_ratio_bits)) f |= KZ_RANK_F_VIOLATED;
            if (f) atomicOr(flag + q, f);
            double wgq = wg[q];
            wgq = wgq != wgq ? (double)INFINITY : wgq;
            if (kz_rank_before(w, j, wgq, g)) atomicAdd(reinterpret_cast<unsigned long long*>(rank + row), 1ull);
        }
    }
}

// The sweep route over the compacted list fl [n_list].  *done = 0: a state outside a form's domain -- nothing the caller may keep was
// decided, the exact route rewrites every output.
static int kz_gold_ranks_r1_run(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, kz_matrix* index, const int64_t* d_gold,
                                const KzRankReduction& red, const int* fl, int n_list, int64_t* d_rank, kz_rank_sweep_stats* st, int* done) {
    *done = 0;
    const int d = (int)index->d, metric = index->metric, kind = red.kind, n_ytiles = (int)index->n_tiles;
    const double mp = index->mink_p;
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    KzSweepQuery qs;
    int rc = qs.init(ctx, query, q_begin, n_list, fl, index);
    if (rc != KZ_OK) return rc;
    const int64_t n_pad = qs.n_pad, y_pad = (int64_t)n_ytiles * KZ_TILE;
    // ---- buffers --------------------------------------------------------------------------------------------------------------
    KzSweepLog log;           // counters: [4] state flag, [6..7] max |U|, max |bias'|; extras: flag [n_pad] | band_cnt [n_pad]
    KzPoolBuf<double> dq;     // wg [n_list] | E [n_list] | hQ [n_list] | extent [1]
    KzPoolBuf<double> dy;     // V key [y_pad] | U [y_pad]
    KzPoolBuf<float> fy;      // bias' [y_pad] | U [y_pad]
    KzPoolBuf<float2> urange;
    KzPoolBuf<float4> plq;
    KzPoolBuf<KnnCountR1Out> d_out;
    rc = log.alloc(ctx, KZ_CERT_LOG_PER_ROW, n_list, false, 2 * (size_t)n_pad);
    if (rc == KZ_OK) rc = dq.alloc(ctx, (3 * (size_t)n_list + 1) * sizeof(double));
    if (rc == KZ_OK) rc = dy.alloc(ctx, 2 * (size_t)y_pad * sizeof(double));
    if (rc == KZ_OK) rc = fy.alloc(ctx, 2 * (size_t)y_pad * sizeof(float));
    if (rc == KZ_OK) rc = urange.alloc(ctx, (size_t)n_ytiles * sizeof(float2));
    if (rc == KZ_OK) rc = plq.alloc(ctx, 2 * (size_t)n_pad * sizeof(float4));
    if (rc == KZ_OK) rc = d_out.alloc(ctx, sizeof(KnnCountR1Out));
    if (rc != KZ_OK) return rc;
    int* gflag = log.words.get() + 4;
    unsigned* gmax = (unsigned*)(log.words.get() + 6);
    int *flag = log.extra(), *band_cnt = flag + n_pad;
    double *wg = dq.get(), *E = wg + n_list, *qd = E + n_list, *ext = qd + n_list;
    double *vkey = dy.get(), *ud = vkey + y_pad;
    float *bias2 = fy.get(), *yu = bias2 + y_pad;
    const float* yraw = (const float*)index->raw;
    const float* qraw = (const float*)query->raw;
    const kz_himage *qi = qs.m->himg, *ii = index->himg;
    const double* hscale = (const double*)ii->center->d_scale;
    KZ_HIP(hipMemsetAsync(log.words.get(), 0, log.n_words * sizeof(int), ctx->stream));
    // ---- the index side, then tau and the two edges of every listed row ---------------------------------------------------------
    kz_r1_dispatch(kind, metric, [&](auto kd, auto euc) {
        hipLaunchKernelGGL((kz_r1_index_kernel<decltype(kd)::value, decltype(euc)::value>), dim3((unsigned)n_ytiles), dim3(128), 0, ctx->stream,
                           (const float*)ii->bias, red.t_a, index->n, metric == KZ_COSINE ? 1.0 : 0.5, hscale, bias2, yu, vkey, ud, urange.get(), gmax, gflag);
    });
    hipLaunchKernelGGL(kz_rank_r1_extent_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)vkey, index->n, ext);
    kz_rank_dispatch(kind, index, [&](auto t, auto kd, auto mt) {
        hipLaunchKernelGGL((kz_rank_r1_query_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(mt)::value>), dim3((unsigned)((n_pad + 3) / 4)),
                           dim3(256), 0, ctx->stream, fl, n_list, n_pad, q_begin, d_gold, qraw, yraw, (const double*)query->sqn, (const double*)index->sqn, d,
                           metric, mp, red.q_a, red.t_a, (const double*)qi->rowq, (const double*)ii->d_max, hscale, (const double*)index->d_stats,
                           ctx->eps_scale, kz_gamma_acc_h(index->kg), (const unsigned*)gmax, (const double*)ext, plq.get(), wg, E, qd, flag, gflag);
    });
    KZ_HIP(hipGetLastError());
    // a state that makes a form invalid: known before the sweep, which then does not run
    int h_flag = 0;
    KZ_HIP(hipMemcpyAsync(&h_flag, gflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (h_flag) return KZ_OK;
    // ---- the sweep ------------------------------------------------------------------------------------------------------------
    const int n_slices = index->kg / 4;
    const KzCountKernel kern = kz_cert_lookup(n_slices, kz_count_r1_lookup_lo, kz_count_r1_lookup_hi);
    KzSweepWork work;
    rc = kz_cert_plan(who, ctx, kern, "count", n_slices, qs.n_qtiles, n_ytiles, &work);
    if (rc != KZ_OK) return rc;
    KnnCountR1Out ho;   // (pageable: alive until the synchronisation behind the sweep)
    memset(&ho, 0, sizeof(ho));
    ho.list = fl;
    ho.rank = (long long*)d_rank;
    ho.band_cnt = band_cnt;
    ho.log_cnt = log.counters();
    ho.log_cap = log.cap;
    ho.log_meta = log.meta.get();
    ho.log_key = log.key.get();
    ho.n_list = n_list;
    KZ_HIP(hipMemcpyAsync(d_out.get(), &ho, sizeof(ho), hipMemcpyHostToDevice, ctx->stream));
    KnnCountR1Params cp;
    memset(&cp, 0, sizeof(cp));
    cp.qpack = (const float*)qi->packed;
    cp.ypack = (const float*)ii->packed;
    cp.ybias = bias2;
    cp.yu = yu;
    cp.urange = urange.get();
    cp.work = work.d_work.get();
    cp.n_ytiles = n_ytiles;
    cp.plq = plq.get();
    cp.out = d_out.get();
    rc = kz_cert_launch(ctx, kern, cp, work.pl.W);
    if (rc != KZ_OK) return rc;
    // ---- the band, the rows that are not trusted --------------------------------------------------------------------------------
    rc = kz_rank_sweep_finish(who, ctx, query, q_begin, index, d_gold, &red, fl, n_list, n_pad, log, d_rank, st, [&](long long n_band, dim3 grid) {
        kz_rank_dispatch(kind, index, [&](auto t, auto kd, auto mt) {
            hipLaunchKernelGGL((kz_rank_r1_resolve_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(mt)::value>), grid, dim3(256), 0, ctx->stream,
                               (const i32x2e*)log.meta.get(), (const float*)log.key.get(), n_band, fl, q_begin, d_gold, qraw, yraw, (const double*)query->sqn,
                               (const double*)index->sqn, index->n, d, metric, mp, red.q_a, red.t_a, (const double*)qi->rowq, hscale, (const double*)wg,
                               (const double*)E, (const double*)qd, (const double*)vkey, (const double*)ud, (const int*)band_cnt, flag, log.counters() + 1,
                               d_rank);
        });
    });
    if (rc != KZ_OK) return rc;
    *done = 1;
    return KZ_OK;
}

extern "C" int kz_gold_ranks_reduced_sweep(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                           const int64_t* d_gold, int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a,
                                           const double* d_t_b, int64_t* d_rank, kz_rank_sweep_stats* stats) {
    const char* who = "kz_gold_ranks_reduced_sweep";
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const KzRankReduction red{kind, d_q_a, d_q_b, d_t_a, d_t_b};
    return kz_rank_sweep_call(who, ctx, query, q_begin, q_count, index, d_gold, &red, d_rank, stats, [&](const int* fl, int n_list, kz_rank_sweep_stats* st, int* done) {
        return kz_gold_ranks_r1_run(who, ctx, query, q_begin, index, d_gold, red, fl, n_list, d_rank, st, done);
    });
}
