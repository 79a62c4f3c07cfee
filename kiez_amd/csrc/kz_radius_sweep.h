// RADIUS NEIGHBOURS ON THE fp16 SWEEP (kz_radius_neighbors_sweep, opt-in): the CSR of kz_radius_neighbors -- the same bytes for every
// input -- with the float64 value matrix replaced by a first pass on the fp16 MFMA sweep.  A radius is a
// per-row threshold on the sweep's key; the fast pass only decides WHICH pairs need the exact value (section 4), and that value is
// what the call returns for them:
//   1. kz_radius_band_kernel: per query row the interval [lo, hi] of approximate keys that the fp16 tier's rounding bound
//      (kz_h_key_eps, kz_range.h) cannot order against the radius;
//   2a. capacity == 0: kz_knn_count_h_kernel (kz_knn_cnt16.h, unchanged) counts the keys above hi into a count vector and logs the
//      band; kz_radius_resolve_kernel<false> adds the band entries whose exact w is <= radius;
//   2b. capacity > 0: kz_knn_emit_h_kernel (kz_knn_emit16.h) logs every key >= lo; the log is ordered by (query row, index row)
//      (kz_cert_order_log, kz_cert_sweep.h: two stable passes of kz_sort_pairs_f32_i32); kz_radius_resolve_kernel<true> evaluates every entry
//      -- kz_exact_value, kz_output_distance<float>: the bits of the exact route -- and the predicate w <= radius;
//   3. kz_radius_rows_kernel: one wave per query row finds its run of the ordered log (two binary searches), counts the kept entries
//      and, in its second launch, writes them at d_indptr[row] + ballot prefix: ascending by index row, no atomics on the output;
//      kz_radius_scan_batch_kernel (kz_radius.h) turns the counts into d_indptr; `sorted` runs kz_radius_sort_kernel as the exact
//      route does.
// The bound checks itself on every evaluated entry (|key~ scale - key| / eps <= 1; an entry logged as "above hi" must pass the
// predicate).  The WHOLE call takes kz_radius_impl -- route_taken = 0, never an error -- for a shape outside the sweep
// (kz_plain_sweep_shapes_ok), a radius that is not finite or is negative, a log that overflowed, a violated bound and a row whose
// norm or interval is not finite: rows of a CSR are not independent the way ranks are, so there is no per-row fallback.
// Rows of 80 .. 128 slices (d = 1025 .. 2048): both sweeps are builds of kz_knn_cntx_h_kernel (kz_knn_cntx16.h), two workgroups an item.
#pragma once
#include "kz_cert_sweep.h"

enum { KZ_RSW_F_NONFINITE = 1, KZ_RSW_F_VIOLATED = 2 };

// One thread per query row r of the image (row q_begin + r of the query): lohi [r], eps [r].
// Threshold in ranking-value units: v_r = radius (sqeuclidean, cosine: w is the value itself); euclidean: w = fl32(sqrt(fl32(v))) is
// monotone in v, and with u = 2^-24 and both roundings to nearest w = sqrt(v) (1 + t), |t| <= u / 2 + u + O(u^2) < 2 u for a normal
// fl32(v), so w <= radius is decided by v alone outside radius^2 (1 -+ 4 u); the bracket used is radius^2 (1 -+ 8 u) -+ 2^-140 --
// twice that width, the float64 rounding of radius^2 (2^-53) and of the two products far inside it, and the absolute term covers
// fl32 of a subnormal v (absolute error <= 2^-150).  Key of a value: (qc2 - v) / 2 (cosine: (qc2 - 2 v) / 2), kz_rank_band_kernel's.
// lo = (key(v_hi) - eps) / scale rounded down and one float step further; hi = (key(v_lo) + eps) / scale rounded up and one further.
// Pad rows: lo = hi = +inf, nothing logged.  A row whose norm or interval is not finite raises the fallback flag -- a NaN operand
// among them: host rows with a NaN are refused when the matrix is made, and for device rows that carry one the exact route's
// fmax(NaN, 0) makes every value of the row 0, a FULL row, which no threshold on keys reproduces.
__global__ __launch_bounds__(256) void kz_radius_band_kernel(int64_t n_rows, int64_t n_pad, int64_t q_begin, const double* __restrict__ qsqn, int metric,
                                                             double radius, const double* __restrict__ rowq, const double* __restrict__ y_hmax,
                                                             const double* __restrict__ hscale, const double* __restrict__ ystats, double eps_mult,
                                                             double gamma_acc, float2* __restrict__ lohi, double* __restrict__ eps_out,
                                                             int* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pad) return;
    if (r >= n_rows) {
        lohi[r] = make_float2(INFINITY, INFINITY);
        return;
    }
    const double qs = qsqn[q_begin + r];
    const double qc2 = rowq[r * 3];
    const double eps = kz_h_key_eps(rowq + r * 3, y_hmax, ystats, metric == KZ_COSINE ? 0.0 : qs, metric, eps_mult, gamma_acc);
    eps_out[r] = eps;
    double v_lo = radius, v_hi = radius;
    if (metric == KZ_EUCLIDEAN) {
        const double r2 = radius * radius, w = 4.76837158203125e-07 /* 8 x 2^-24 */, a = 7.174648137343064e-43 /* 2^-140 */;
        v_lo = r2 * (1.0 - w) - a;
        v_hi = r2 * (1.0 + w) + a;
    }
    const double key_hi = 0.5 * (qc2 - (metric == KZ_COSINE ? 2.0 * v_lo : v_lo)), key_lo = 0.5 * (qc2 - (metric == KZ_COSINE ? 2.0 * v_hi : v_hi));
    const double want_lo = (key_lo - eps) / hscale[1], want_hi = (key_hi + eps) / hscale[1];
    const float lo = kz_round_below(want_lo), hi = kz_round_above(want_hi);
    const bool ok = fabs(qs) < (double)INFINITY && fabs(eps) < (double)INFINITY && fabsf(lo) < INFINITY && fabsf(hi) < INFINITY;
    if (!ok) {
        lohi[r] = make_float2(INFINITY, INFINITY);
        atomicOr(flag, KZ_RSW_F_NONFINITE);
        return;
    }
    lohi[r] = make_float2(lo, hi);
}

// One wave per log entry.  EMIT: place e of the ordered log is entry pos[e] = {query row | above bit, index row, key~}; its exact w
// goes to w_out [e] and keep [e] = (w <= radius).  !EMIT (the count call): the entries are the band of kz_knn_count_h_kernel, in log
// order, and a kept entry adds one to its row's count.  Both: the bound's own check, the largest ratio, the violation flag.
// An entry on a pad index row (bias -inf: below every finite lo) or a pad query row (lo = +inf) never occurs; it would be dropped,
// not read.
template <bool EMIT>
__global__ __launch_bounds__(256) void kz_radius_resolve_kernel(const i32x2e* __restrict__ log_meta, const float* __restrict__ log_key,
                                                                const int* __restrict__ pos, long long n_entries, int n_rows, int64_t q_begin,
                                                                const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                                const double* __restrict__ qsqn, const double* __restrict__ ysqn, int64_t n_i, int d,
                                                                int metric, double radius, const double* __restrict__ rowq,
                                                                const double* __restrict__ hscale, const double* __restrict__ eps,
                                                                int* __restrict__ flag, unsigned long long* __restrict__ max_ratio_bits,
                                                                int* __restrict__ keep, double* __restrict__ w_out, long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_entries; e += n_waves) {
        const long long at = EMIT ? pos[e] : e;
        const i32x2e mt = log_meta[at];
        const int q = mt.x & ~KZ_EMIT_ABOVE;
        const bool above = (mt.x & KZ_EMIT_ABOVE) != 0;
        const int64_t j = mt.y;
        if (j < 0 || j >= n_i || q >= n_rows) {   // (wave-uniform)
            if (EMIT && lane == 0) keep[e] = 0;
            continue;
        }
        const int64_t qrow = q_begin + q;
        const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + j * (int64_t)d, qsqn[qrow], ysqn[j], d, metric, lane);
        if (lane == 0) {   // (every lane holds v; the wave meets again at the next entry's butterfly)
            const double w = kz_output_distance<float>(v, metric);
            const bool in = w <= radius;   // (NaN: false)
            const double key = 0.5 * (rowq[(int64_t)q * 3] - (metric == KZ_COSINE ? 2.0 * v : v));
            if (!kz_bound_holds((double)log_key[at] * hscale[1], key, eps[q], max_ratio_bits) || (above && !in)) atomicOr(flag, KZ_RSW_F_VIOLATED);
            if (EMIT) {
                keep[e] = in ? 1 : 0;
                w_out[e] = w;
            } else if (in) {
                atomicAdd(reinterpret_cast<unsigned long long*>(count + q), 1ull);
            }
        }
    }
}

// One wave per query row q over the ordered log (row_key ascending; within a row ascending by index row): its run [a, b) by two
// binary searches.  !WRITE: row_n[q] = the kept entries of the run.  WRITE: for a row that ends within `capacity`, the kept entries
// (index row, w) at indptr[q] + (kept entries of the run before it) -- a ballot prefix per 64 entries.
template <bool WRITE>
__global__ __launch_bounds__(256) void kz_radius_rows_kernel(const int* __restrict__ row_key, const int* __restrict__ pos, int n, int n_rows,
                                                             const int* __restrict__ keep, const double* __restrict__ w_in,
                                                             const i32x2e* __restrict__ log_meta, int* __restrict__ row_n,
                                                             const int64_t* __restrict__ indptr, int64_t capacity, int64_t* __restrict__ d_ind,
                                                             double* __restrict__ d_dist) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_rows) return;   // (wave-uniform)
    int64_t out = 0, row_end = 0;
    if (WRITE) {
        out = indptr[q];
        row_end = indptr[q + 1];
        if (row_end > capacity || row_end == out) return;
    }
    const int a = kz_run_lower(row_key, n, q), b = kz_run_lower(row_key, n, q + 1);
    int kept = 0;   // (uniform)
    for (int e0 = a; e0 < b; e0 += 64) {   // (uniform)
        const int e = e0 + lane;
        const bool k = e < b && keep[e] != 0;
        const unsigned long long m = __ballot(k);
        if (WRITE && k) {
            const int64_t place = out + kept + __popcll(m & ((1ull << lane) - 1ull));
            if (place < row_end) {
                d_ind[place] = log_meta[pos[e]].y;
                d_dist[place] = w_in[e];
            }
        }
        kept += __popcll(m);
    }
    if (!WRITE && lane == 0) row_n[q] = kept;
}

// (the count call: the count vector the sweep and the band added into, as the row counts the scan takes; zero: clears both)
__global__ __launch_bounds__(256) void kz_radius_narrow_kernel(const long long* __restrict__ count, int n_rows, int* __restrict__ row_n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) row_n[i] = (int)count[i];
}
__global__ __launch_bounds__(256) void kz_radius_clear_kernel(int* __restrict__ words, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) words[i] = 0;
}

static KzCountKernel kz_emit_lookup(int n_slices) {
    return kz_cert_lookup(n_slices, kz_emit_lookup_lo, kz_emit_lookup_hi, kz_emit_lookup_w, kz_emit_lookup_x);
}

// The sweep route.  *done = 0: nothing the caller may keep was decided (overflow, a violated or non-finite bound) -- the exact route
// rewrites every output.  stats: the sweep's share is filled here.
static int kz_radius_sweep_run(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, double radius,
                               int sorted, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, double* d_dist, int64_t* h_total,
                               kz_radius_sweep_stats* st, int* done) {
    *done = 0;
    const int d = (int)index->d, metric = index->metric;
    const int n_rows = (int)q_count;
    const bool emit = capacity > 0;
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    KzSweepQuery qs;
    int rc = qs.init(ctx, query, q_begin, n_rows, nullptr, index);
    if (rc != KZ_OK) return rc;
    const int n_ytiles = (int)index->n_tiles;
    const int64_t n_pad = qs.n_pad;
    // ---- intervals, counters, the log ---------------------------------------------------------------------------------------------
    KzPoolBuf<float2> lohi;
    KzPoolBuf<double> epsb;     // [n_rows]
    KzSweepLog log;             // counters: [4] flags, [8..11] the scan's running base and the longest row; extras, the count call:
                                // count [n_rows] int64 | band_cnt [n_pad]
    KzPoolBuf<int> row_n;       // [n_rows]
    rc = lohi.alloc(ctx, (size_t)n_pad * sizeof(float2));
    if (rc == KZ_OK) rc = epsb.alloc(ctx, (size_t)n_rows * sizeof(double));
    if (rc == KZ_OK) rc = log.alloc(ctx, KZ_CERT_LOG_PER_ROW, n_rows, true, emit ? 0 : (size_t)n_pad + 2 * (size_t)n_rows);
    if (rc == KZ_OK) rc = row_n.alloc(ctx, (size_t)n_rows * sizeof(int));
    if (rc != KZ_OK) return rc;
    unsigned long long* counters = log.counters();
    int* flag = log.words.get() + 4;
    int64_t* scan_state = (int64_t*)(log.words.get() + 8);
    long long* count = (long long*)log.extra();
    int* band_cnt = log.extra() + 2 * (size_t)n_rows;   // (the count kernel's per-row band counter: written, not read here)
    hipLaunchKernelGGL(kz_radius_clear_kernel, dim3((unsigned)((log.n_words + 255) / 256)), dim3(256), 0, ctx->stream, log.words.get(), (int64_t)log.n_words);
    const kz_himage *qi = qs.m->himg, *ii = index->himg;
    hipLaunchKernelGGL(kz_radius_band_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)n_rows, n_pad, q_begin,
                       (const double*)query->sqn, metric, radius, (const double*)qi->rowq, (const double*)ii->d_max,
                       (const double*)ii->center->d_scale, (const double*)index->d_stats, ctx->eps_scale, kz_gamma_acc_h(index->kg), lohi.get(),
                       epsb.get(), flag);
    KZ_HIP(hipGetLastError());
    // ---- the sweep ------------------------------------------------------------------------------------------------------------------
    const int n_slices = kz_h_nsr(index->kg);   // (the padded count the images are packed with)
    const KzCountKernel kern = emit ? kz_emit_lookup(n_slices) : kz_count_lookup(n_slices);
    KzSweepWork work;
    rc = kz_cert_plan(who, ctx, kern, "sweep", n_slices, qs.n_qtiles, n_ytiles, &work);
    if (rc != KZ_OK) return rc;
    if (emit) {
        KnnEmitParams ep;
        memset(&ep, 0, sizeof(ep));
        ep.qpack = (const float*)qi->packed;
        ep.ypack = (const float*)ii->packed;
        ep.ybias = ii->bias;
        ep.work = work.d_work.get();
        ep.n_ytiles = n_ytiles;
        ep.lohi = lohi.get();
        ep.log_cnt = counters;
        ep.log_cap = log.cap;
        ep.log_meta = log.meta.get();
        ep.log_key = log.key.get();
        rc = kz_cert_launch(ctx, kern, ep, work.pl.W);
    } else {
        // the count kernel as it is: the row list is the identity, the count vector stands where the rank vector stood
        KnnCountParams cp;
        memset(&cp, 0, sizeof(cp));
        rc = qs.identity(&cp.list);
        if (rc != KZ_OK) return rc;
        cp.qpack = (const float*)qi->packed;
        cp.ypack = (const float*)ii->packed;
        cp.ybias = ii->bias;
        cp.work = work.d_work.get();
        cp.n_ytiles = n_ytiles;
        cp.lohi = lohi.get();
        cp.n_list = n_rows;
        cp.rank = count;
        cp.band_cnt = band_cnt;
        cp.log_cnt = counters;
        cp.log_cap = log.cap;
        cp.log_meta = log.meta.get();
        cp.log_key = log.key.get();
        rc = kz_cert_launch(ctx, kern, cp, work.pl.W);
    }
    if (rc != KZ_OK) return rc;
    KzSweepCounters h;
    rc = kz_cert_sweep_done(ctx, who, log, &h, st);
    if (rc != KZ_OK) return rc;
    st->n_rows = n_rows;
    if (st->overflowed || h.flag) return KZ_OK;   // (flag: a non-finite interval)
    // ---- from the log to the CSR ---------------------------------------------------------------------------------------------------
    const int n = (int)h.n_log;
    KzLogOrder ord;
    KzPoolBuf<int> keep;
    KzPoolBuf<double> wbuf;
    const float* yraw = (const float*)index->raw;
    const float* qraw = (const float*)query->raw;
    if (emit) {
        if (n > 0) {
            rc = kz_cert_order_log(ctx, log.meta.get(), n, &ord);
            if (rc == KZ_OK) rc = keep.alloc(ctx, (size_t)n * 4);
            if (rc == KZ_OK) rc = wbuf.alloc(ctx, (size_t)n * 8);
            if (rc != KZ_OK) return rc;
            const long long wgs = ((long long)n + 3) / 4;
            hipLaunchKernelGGL(kz_radius_resolve_kernel<true>, dim3((unsigned)(wgs < 65536 ? wgs : 65536)), dim3(256), 0, ctx->stream,
                               (const i32x2e*)log.meta.get(), (const float*)log.key.get(), ord.pos(), (long long)n, n_rows, q_begin, qraw, yraw,
                               (const double*)query->sqn, (const double*)index->sqn, index->n, d, metric, radius, (const double*)qi->rowq,
                               (const double*)ii->center->d_scale, (const double*)epsb.get(), flag, counters + 1, keep.get(), wbuf.get(),
                               (long long*)nullptr);
        }
        hipLaunchKernelGGL(kz_radius_rows_kernel<false>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, ord.row_key(),
                           ord.pos(), n, n_rows, (const int*)keep.get(), (const double*)wbuf.get(), (const i32x2e*)log.meta.get(), row_n.get(),
                           (const int64_t*)nullptr, capacity, (int64_t*)nullptr, (double*)nullptr);
    } else {
        if (n > 0) {
            const long long wgs = ((long long)n + 3) / 4;
            hipLaunchKernelGGL(kz_radius_resolve_kernel<false>, dim3((unsigned)(wgs < 65536 ? wgs : 65536)), dim3(256), 0, ctx->stream,
                               (const i32x2e*)log.meta.get(), (const float*)log.key.get(), (const int*)nullptr, (long long)n, n_rows, q_begin, qraw, yraw,
                               (const double*)query->sqn, (const double*)index->sqn, index->n, d, metric, radius, (const double*)qi->rowq,
                               (const double*)ii->center->d_scale, (const double*)epsb.get(), flag, counters + 1, (int*)nullptr, (double*)nullptr,
                               count);
        }
        hipLaunchKernelGGL(kz_radius_narrow_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, (const long long*)count, n_rows,
                           row_n.get());
    }
    hipLaunchKernelGGL(kz_radius_scan_batch_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)row_n.get(), 0, n_rows, d_indptr, scan_state);
    if (emit)
        hipLaunchKernelGGL(kz_radius_rows_kernel<true>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, ord.row_key(),
                           ord.pos(), n, n_rows, (const int*)keep.get(), (const double*)wbuf.get(), (const i32x2e*)log.meta.get(), (int*)nullptr,
                           (const int64_t*)d_indptr, capacity, d_ind, d_dist);
    KZ_HIP(hipGetLastError());
    int64_t h_state[2] = {0, 0};   // the total, the longest row
    KZ_HIP(hipMemcpyAsync(h_state, scan_state, sizeof(h_state), hipMemcpyDeviceToHost, ctx->stream));
    rc = log.read(ctx, who, "resolving the log", &h);
    if (rc != KZ_OK) return rc;
    memcpy(&st->max_err_ratio, &h.ratio_bits, 8);
    if (h.flag) return KZ_OK;   // (a violated bound: nothing of the above is trusted)
    if (sorted && emit && h_state[1] >= 2) {
        KzPoolBuf<double> tmp_w;   // the radix path of the sort, as kz_radius_impl
        KzPoolBuf<int64_t> tmp_i;
        if (h_state[1] > KZ_RADIUS_SORT_LDS) {
            const size_t n_out = (size_t)(h_state[0] < capacity ? h_state[0] : capacity);
            rc = tmp_w.alloc(ctx, n_out * sizeof(double));
            if (rc == KZ_OK) rc = tmp_i.alloc(ctx, n_out * sizeof(int64_t));
            if (rc != KZ_OK) return rc;
        }
        hipLaunchKernelGGL(kz_radius_sort_kernel, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, (const int64_t*)d_indptr, capacity, d_dist, d_ind,
                           tmp_w.get(), tmp_i.get());
        KZ_HIP(hipGetLastError());
    }
    KZ_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    KZ_HIP(hipEventSynchronize(ctx->ev[5]));
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    st->resolve_ms = ms;
    st->n_pairs = h_state[0];
    *h_total = h_state[0];
    *done = 1;
    return KZ_OK;
}

extern "C" int kz_radius_neighbors_sweep(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                         double radius, int sorted, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                                         int64_t* h_total, kz_radius_sweep_stats* stats) {
    const char* who = "kz_radius_neighbors_sweep";
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair(who, ctx, query, q_begin, q_count, index, d_indptr, h_total);
    if (rcp != KZ_OK) return rcp;
    kz_radius_sweep_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    KZ_REQUIRE(radius == radius, "%s: radius is NaN", who);
    KZ_REQUIRE(capacity >= 0, "%s: capacity %lld is negative", who, (long long)capacity);
    KZ_REQUIRE(capacity == 0 || (d_ind && d_dist), "%s: d_ind / d_dist are required for capacity > 0", who);
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    KZ_HIP(hipSetDevice(ctx->device));
    int done = 0;
    if (q_count > 0 && radius >= 0.0 && radius < (double)INFINITY && kz_plain_sweep_shapes_ok(ctx, query, index)) {
        const int rc = kz_radius_sweep_run(who, ctx, query, q_begin, q_count, index, radius, sorted, capacity, d_indptr, d_ind, d_dist, h_total, &st, &done);
        if (rc != KZ_OK) return rc;
    }
    if (done) {
        st.route_taken = 1;
    } else {
        const int rc = kz_cert_exact_route(ctx, &st.fallback_ms, [&] {
            return kz_radius_impl(who, ctx, query, q_begin, q_count, index, radius, sorted, capacity, nullptr, d_indptr, d_ind, d_dist, h_total);
        });
        if (rc != KZ_OK) return rc;
        st.n_rows = q_count;
        st.n_pairs = *h_total;
    }
    if (stats) *stats = st;
    return KZ_OK;
}
