// GOLD RANKS ON THE fp16 COUNT SWEEP (kz_gold_ranks_sweep, opt-in): the ranks of kz_gold_ranks -- the same integers on every row --
// with the float64 value matrix replaced by a first pass on the fp16 MFMA sweep.  The fast pass only decides
// WHICH pairs need the exact value (section 4):
//   1. kz_rank_band_kernel: per listed row the exact value v_g of (row, gold), its key and the interval [lo, hi] of approximate keys
//      that the fp16 tier's rounding bound (kz_h_key_eps, kz_range.h) cannot order against it;
//   2. kz_knn_count_h_kernel (kz_knn_cnt16.h): counts the keys above hi into d_rank, logs the keys inside [lo, hi] -- the band;
//   3. kz_rank_resolve_kernel: the exact value of every band entry (kz_exact_value: the arithmetic of every exact kernel, bit for
//      bit), compared with (v_g, g) by the rule of kz_rank_before; the bound checks itself on every entry (|key~ scale - key| / eps);
//   4. kz_rank_fallback_kernel: rows that are not trusted -- a non-finite value or bound, a band beyond the per-row cap, a violated
//      bound, a gold row that did not show up in its own band, every row when the log overflowed -- are reset and go through the
//      exact walk (kz_gold_ranks_walk), as a compacted list.
// Shapes outside the sweep (kz_plain_sweep_shapes_ok) take kz_gold_ranks_impl whole: same answer, route_taken = 0, never an error.
// Element types: float32 rows run the sweep; float64, float16 and bfloat16 rows take the exact route (the band's values are read by
// the float32 kernels' rule only, as kz_exact_pairs_kernel's are).
#pragma once
#include "kz_cert_sweep.h"

// A sizing choice, not a tuned figure: a row whose band holds more entries than this is cheaper on the exact walk than worth arguing
// about (ties by the thousand, a gold row deep inside a tight cluster).  (The log: KzSweepLog, KZ_CERT_LOG_PER_ROW entries a row.)
constexpr int KZ_RANK_BAND_ROW_CAP = 1024;
enum { KZ_RANK_F_NONFINITE = 1, KZ_RANK_F_VIOLATED = 2, KZ_RANK_F_GOLD_SEEN = 4 };

// One wave per listed row r (row list[r] of the call): vg [r] the exact value of its gold pair, eps [r] the bound, lohi [r] the
// interval in the image's key units -- lo rounded down and one float step further down, hi rounded up and one step further up.
// A value or an interval that is not finite: lo = hi = +inf and the fallback flag.  Pad rows: lo = hi = +inf, no flag.
__global__ __launch_bounds__(256) void kz_rank_band_kernel(const int* __restrict__ list, int n_list, int64_t n_pad, int64_t q_begin,
                                                           const int64_t* __restrict__ gold, const float* __restrict__ qraw,
                                                           const float* __restrict__ yraw, const double* __restrict__ qsqn,
                                                           const double* __restrict__ ysqn, int d, int metric, const double* __restrict__ rowq,
                                                           const double* __restrict__ y_hmax, const double* __restrict__ hscale,
                                                           const double* __restrict__ ystats, double eps_mult, double gamma_acc,
                                                           float2* __restrict__ lohi, double* __restrict__ vg, double* __restrict__ eps_out,
                                                           int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_pad) return;
    if (r >= n_list) {
        if (lane == 0) lohi[r] = make_float2(INFINITY, INFINITY);
        return;
    }
    const int64_t qrow = q_begin + list[r];
    const int64_t g = gold[list[r]];
    const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + g * (int64_t)d, qsqn[qrow], ysqn[g], d, metric, lane);
    if (lane != 0) return;
    const double qc2 = rowq[r * 3];
    const double eps = kz_h_key_eps(rowq + r * 3, y_hmax, ystats, metric == KZ_COSINE ? 0.0 : qsqn[qrow], metric, eps_mult, gamma_acc);
    const double key = 0.5 * (qc2 - (metric == KZ_COSINE ? 2.0 * v : v));
    const double want_lo = (key - eps) / hscale[1], want_hi = (key + eps) / hscale[1];
    const float lo = kz_round_below(want_lo), hi = kz_round_above(want_hi);
    const bool ok = fabs(v) < (double)INFINITY && fabs(eps) < (double)INFINITY && fabsf(lo) < INFINITY && fabsf(hi) < INFINITY;
    lohi[r] = ok ? make_float2(lo, hi) : make_float2(INFINITY, INFINITY);
    vg[r] = v;
    eps_out[r] = eps;
    if (!ok) flag[r] = KZ_RANK_F_NONFINITE;
}

// One wave per band entry {listed row q, index row j, key~}: the pair's exact value; +1 for the row when (v_j, j) orders before
// (v_g, g) -- NaN as +inf, the gold row itself adds nothing -- and the bound's own check.  Entries of rows beyond the per-row cap
// are skipped (the row falls back), entries on pad index rows (lo = -inf cannot happen: such a row is flagged) never occur.
__global__ __launch_bounds__(256) void kz_rank_resolve_kernel(const i32x2e* __restrict__ log_meta, const float* __restrict__ log_key, long long n_entries,
                                                              const int* __restrict__ list, int64_t q_begin, const int64_t* __restrict__ gold,
                                                              const float* __restrict__ qraw, const float* __restrict__ yraw,
                                                              const double* __restrict__ qsqn, const double* __restrict__ ysqn, int64_t n_i, int d,
                                                              int metric, const double* __restrict__ rowq, const double* __restrict__ hscale,
                                                              const double* __restrict__ vg, const double* __restrict__ eps,
                                                              const int* __restrict__ band_cnt, int* __restrict__ flag,
                                                              unsigned long long* __restrict__ max_ratio_bits, int64_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_entries; e += n_waves) {
        const i32x2e mt = log_meta[e];
        const int q = mt.x;
        const int64_t j = mt.y;
        if (j >= n_i || band_cnt[q] > KZ_RANK_BAND_ROW_CAP) continue;   // (wave-uniform)
        const int row = list[q];
        const int64_t qrow = q_begin + row, g = gold[row];
        const double v = kz_exact_value<float>(qraw + qrow * (int64_t)d, yraw + j * (int64_t)d, qsqn[qrow], ysqn[j], d, metric, lane);
        if (lane == 0) {   // (every lane holds v; the wave meets again at the next entry's butterfly)
            const double key = 0.5 * (rowq[(int64_t)q * 3] - (metric == KZ_COSINE ? 2.0 * v : v));
            int f = j == g ? KZ_RANK_F_GOLD_SEEN : 0;
            if (!kz_bound_holds((double)log_key[e] * hscale[1], key, eps[q], max_ratio_bits)) f |= KZ_RANK_F_VIOLATED;
            if (f) atomicOr(flag + q, f);
            if (kz_rank_before(v, j, vg[q], g)) atomicAdd(reinterpret_cast<unsigned long long*>(rank + row), 1ull);
        }
    }
}

// fb [n_list] + count at fb[n_list]: the listed rows that are not trusted, in list order (one workgroup, as kz_rank_compact_kernel);
// their rank entries are reset for the exact walk.
__global__ __launch_bounds__(256) void kz_rank_fallback_kernel(const int* __restrict__ list, int n_list, const int* __restrict__ flag,
                                                               const int* __restrict__ band_cnt, int all, int* __restrict__ fb,
                                                               int64_t* __restrict__ rank) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < n_list; r0 += 256) {
        const int r = r0 + tid;
        bool bad = false;
        if (r < n_list) {
            const int f = flag[r];
            bad = all || (f & (KZ_RANK_F_NONFINITE | KZ_RANK_F_VIOLATED)) || !(f & KZ_RANK_F_GOLD_SEEN) || band_cnt[r] > KZ_RANK_BAND_ROW_CAP;
            if (bad) rank[list[r]] = 0;
        }
        const unsigned long long m = __ballot(bad);
        if (lane == 0) s_w[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        if (bad) fb[off + __popcll(m & ((1ull << lane) - 1ull))] = list[r];
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) fb[n_list] = base;
}

static KzCountKernel kz_count_lookup(int n_slices) {
    return kz_cert_lookup(n_slices, kz_count_lookup_lo, kz_count_lookup_hi, kz_count_lookup_w, kz_count_lookup_x);
}

// Both rank sweeps behind the launch of their count kernel (words of the log: counters | flag [n_pad] | band_cnt [n_pad]): the band's
// size, resolve(n_band, workgroups) -- the call's resolve kernel -- unless the log overflowed, the rows that are not trusted through
// the exact walk (red: the reduction, or null), the statistics.  ev[3] was recorded where the call began.
template <class Resolve>
static int kz_rank_sweep_finish(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, kz_matrix* index, const int64_t* d_gold,
                                const KzRankReduction* red, const int* fl, int n_list, int64_t n_pad, const KzSweepLog& log, int64_t* d_rank,
                                kz_rank_sweep_stats* st, Resolve resolve) {
    unsigned long long* counters = log.counters();
    const int *flag = log.extra(), *band_cnt = flag + n_pad;
    KzPoolBuf<int> fb;   // [n_list + 1]
    int rc = fb.alloc(ctx, ((size_t)n_list + 1) * sizeof(int));
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    unsigned long long n_band = 0;
    KZ_HIP(hipMemcpyAsync(&n_band, counters, 8, hipMemcpyDeviceToHost, ctx->stream));
    rc = kz_cert_sync(ctx, who, "the count sweep");
    if (rc != KZ_OK) return rc;
    const bool over = n_band > (unsigned long long)log.cap;
    if (!over && n_band > 0) {
        const long long wgs = ((long long)n_band + 3) / 4;
        resolve((long long)n_band, dim3((unsigned)(wgs < 65536 ? wgs : 65536)));
    }
    hipLaunchKernelGGL(kz_rank_fallback_kernel, dim3(1), dim3(256), 0, ctx->stream, fl, n_list, flag, band_cnt, over ? 1 : 0, fb.get(), d_rank);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    int n_fb = 0;
    unsigned long long ratio_bits = 0;
    KZ_HIP(hipMemcpyAsync(&n_fb, fb.get() + n_list, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipMemcpyAsync(&ratio_bits, counters + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    rc = kz_cert_sync(ctx, who, "resolving the band");
    if (rc != KZ_OK) return rc;
    if (n_fb > 0) {
        rc = kz_gold_ranks_walk(who, ctx, query, q_begin, index, d_gold, red, fb.get(), n_fb, d_rank);
        if (rc != KZ_OK) return rc;
    }
    KZ_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
    KZ_HIP(hipEventSynchronize(ctx->ev[6]));
    st->n_fallback_rows = n_fb;
    st->n_sweep_rows = n_list - n_fb;
    st->n_band_pairs = (int64_t)n_band;
    memcpy(&st->max_err_ratio, &ratio_bits, 8);
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
    st->sweep_ms = ms;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    st->band_ms = ms;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[6]));
    st->fallback_ms = ms;
    return KZ_OK;
}

// The sweep route over the compacted list fl [n_list] (every buffer is released when the call returns, stream-ordered, behind its
// last synchronisation).  *done = 1: every listed row has its rank.
static int kz_gold_ranks_sweep_run(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, kz_matrix* index, const int64_t* d_gold,
                                   const int* fl, int n_list, int64_t* d_rank, kz_rank_sweep_stats* st, int* done) {
    *done = 0;
    const int d = (int)index->d, metric = index->metric, n_ytiles = (int)index->n_tiles;
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    KzSweepQuery qs;
    int rc = qs.init(ctx, query, q_begin, n_list, fl, index);
    if (rc != KZ_OK) return rc;
    const int64_t n_pad = qs.n_pad;
    // ---- thresholds, counters, the log ----------------------------------------------------------------------------------------
    KzPoolBuf<float2> lohi;
    KzPoolBuf<double> dbuf;   // vg [n_list] | eps [n_list]
    KzSweepLog log;           // extras: flag [n_pad] | band_cnt [n_pad]
    rc = lohi.alloc(ctx, (size_t)n_pad * sizeof(float2));
    if (rc == KZ_OK) rc = dbuf.alloc(ctx, (size_t)n_list * 2 * sizeof(double));
    if (rc == KZ_OK) rc = log.alloc(ctx, KZ_CERT_LOG_PER_ROW, n_list, false, 2 * (size_t)n_pad);
    if (rc != KZ_OK) return rc;
    double *vg = dbuf.get(), *eps = dbuf.get() + n_list;
    int *flag = log.extra(), *band_cnt = flag + n_pad;
    KZ_HIP(hipMemsetAsync(log.words.get(), 0, log.n_words * sizeof(int), ctx->stream));
    const kz_himage *qi = qs.m->himg, *ii = index->himg;
    hipLaunchKernelGGL(kz_rank_band_kernel, dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, ctx->stream, fl, n_list, n_pad, q_begin, d_gold,
                       (const float*)query->raw, (const float*)index->raw, (const double*)query->sqn, (const double*)index->sqn, d, metric,
                       (const double*)qi->rowq, (const double*)ii->d_max, (const double*)ii->center->d_scale, (const double*)index->d_stats,
                       ctx->eps_scale, kz_gamma_acc_h(index->kg), lohi.get(), vg, eps, flag);
    KZ_HIP(hipGetLastError());
    // ---- the sweep ------------------------------------------------------------------------------------------------------------
    const int n_slices = kz_h_nsr(index->kg);   // (the padded count the images are packed with)
    const KzCountKernel kern = kz_count_lookup(n_slices);
    KzSweepWork work;
    rc = kz_cert_plan(who, ctx, kern, "count", n_slices, qs.n_qtiles, n_ytiles, &work);
    if (rc != KZ_OK) return rc;
    KnnCountParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.qpack = (const float*)qi->packed;
    cp.ypack = (const float*)ii->packed;
    cp.ybias = ii->bias;
    cp.work = work.d_work.get();
    cp.n_ytiles = n_ytiles;
    cp.lohi = lohi.get();
    cp.list = fl;
    cp.n_list = n_list;
    cp.rank = (long long*)d_rank;
    cp.band_cnt = band_cnt;
    cp.log_cnt = log.counters();
    cp.log_cap = log.cap;
    cp.log_meta = log.meta.get();
    cp.log_key = log.key.get();
    rc = kz_cert_launch(ctx, kern, cp, work.pl.W);
    if (rc != KZ_OK) return rc;
    // ---- the band, the rows that are not trusted --------------------------------------------------------------------------------
    rc = kz_rank_sweep_finish(who, ctx, query, q_begin, index, d_gold, nullptr, fl, n_list, n_pad, log, d_rank, st, [&](long long n_band, dim3 grid) {
        hipLaunchKernelGGL(kz_rank_resolve_kernel, grid, dim3(256), 0, ctx->stream, (const i32x2e*)log.meta.get(), (const float*)log.key.get(), n_band, fl,
                           q_begin, d_gold, (const float*)query->raw, (const float*)index->raw, (const double*)query->sqn, (const double*)index->sqn,
                           index->n, d, metric, (const double*)qi->rowq, (const double*)ii->center->d_scale, (const double*)vg, (const double*)eps,
                           (const int*)band_cnt, flag, log.counters() + 1, d_rank);
    });
    if (rc != KZ_OK) return rc;
    *done = 1;
    return KZ_OK;
}

// Both rank entry points: the argument checks, the listed rows (kz_rank_compact) through run(fl, n_list, &st, &done) where the sweep
// serves the call, else -- or with done = 0 -- the whole call on the exact route (its time is fallback_ms; no sweep rows, hence no
// fallback rows).  red: the reduction of kz_gold_ranks_reduced_sweep, or null.
template <class Run>
static int kz_rank_sweep_call(const char* who, kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index,
                              const int64_t* d_gold, const KzRankReduction* red, int64_t* d_rank, kz_rank_sweep_stats* stats, Run run) {
    const int rcp = kz_require_pair(who, ctx, query, q_begin, q_count, index, d_gold, d_rank);
    if (rcp != KZ_OK) return rcp;
    const int rcr = red ? kz_rank_require_reduction(who, red->kind, red->q_a, red->q_b, red->t_a, red->t_b) : KZ_OK;
    if (rcr != KZ_OK) return rcr;
    kz_rank_sweep_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    int done = 0;
    if (red ? red->kind != KZ_RANK_MP_NORMAL && kz_rank_sweep_shapes_ok(ctx, query, index) : kz_plain_sweep_shapes_ok(ctx, query, index)) {
        KzPoolBuf<int> fl;
        int n_list = 0;
        int rc = kz_rank_compact(ctx, q_count, index, d_gold, d_rank, fl, &n_list);
        if (rc != KZ_OK) return rc;
        st.n_rows = n_list;
        done = n_list == 0;
        if (!done) rc = run((const int*)fl.get(), n_list, &st, &done);
        if (rc != KZ_OK) return rc;
    }
    if (done) {
        st.route_taken = 1;
    } else {
        int n_listed = 0;
        const int rc = kz_cert_exact_route(ctx, &st.fallback_ms, [&] {
            return kz_gold_ranks_impl(who, ctx, query, q_begin, q_count, index, d_gold, red, d_rank, &n_listed);
        });
        if (rc != KZ_OK) return rc;
        st.n_rows = n_listed;
    }
    if (stats) *stats = st;
    return KZ_OK;
}

extern "C" int kz_gold_ranks_sweep(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                   const int64_t* d_gold, int64_t* d_rank, kz_rank_sweep_stats* stats) {
    const char* who = "kz_gold_ranks_sweep";
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    return kz_rank_sweep_call(who, ctx, query, q_begin, q_count, index, d_gold, nullptr, d_rank, stats, [&](const int* fl, int n_list, kz_rank_sweep_stats* st, int* done) {
        return kz_gold_ranks_sweep_run(who, ctx, query, q_begin, index, d_gold, fl, n_list, d_rank, st, done);
    });
}
