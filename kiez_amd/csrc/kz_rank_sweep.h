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
#include "kz_knn_cntx16.h"

// Sizing choices, not tuned figures: a row whose band holds more entries than this is cheaper on the exact walk than worth arguing
// about (ties by the thousand, a gold row deep inside a tight cluster); the log holds 64 entries per listed row, at least 2^20.
constexpr int KZ_RANK_BAND_ROW_CAP = 1024;
constexpr long long KZ_RANK_LOG_PER_ROW = 64;
constexpr long long KZ_RANK_LOG_MIN = 1ll << 20;
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
    float lo = (float)want_lo, hi = (float)want_hi;
    if ((double)lo > want_lo) lo = nextafterf(lo, -INFINITY);
    lo = nextafterf(lo, -INFINITY);
    if ((double)hi < want_hi) hi = nextafterf(hi, INFINITY);
    hi = nextafterf(hi, INFINITY);
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
            const double ratio = fabs((double)log_key[e] * hscale[1] - key) / eps[q];
            int f = j == g ? KZ_RANK_F_GOLD_SEEN : 0;
            if (!(ratio <= 1.0)) f |= KZ_RANK_F_VIOLATED;
            if (f) atomicOr(flag + q, f);
            if (ratio == ratio) atomicMax(max_ratio_bits, (unsigned long long)__double_as_longlong(ratio));   // (non-negative: ordered as integers)
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

// By slice count (kz_h_nsr): lo / hi (2 .. 24), the wide rows (32 .. 64), the parity-split builds (80 .. 128).  A count without a
// build gets the empty descriptor of the unit that would hold it.
static KzCountKernel kz_count_lookup(int n_slices) {
    if (n_slices > 64) return kz_count_lookup_x(n_slices);
    if (n_slices > 24) return kz_count_lookup_w(n_slices);
    return n_slices <= KZ_CNT_WPS3_MAX ? kz_count_lookup_lo(n_slices) : kz_count_lookup_hi(n_slices);
}
// The count kernel's own occupancy query and launcher (beside kz_sweep_occupancy / kz_sweep_launch: it is no entry of kz_sweep_kernel's
// table, whose contract is "lists of K'").  The builds of 2 .. 24 slices stay below 64 KiB of LDS; the parity-split builds take
// 97.5 KiB, and BOTH the query and the launch raise the function's limit first (kz_raise_lds: neither depends on the other).
static int kz_count_occupancy(kz_ctx* ctx, const KzCountKernel& k, int* blocks_per_cu) {
    const int rc = kz_raise_lds(ctx, k.fn, k.lds_bytes);
    if (rc != KZ_OK) return rc;
    int nb = 0;
    KZ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, 256, k.lds_bytes));
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return KZ_OK;
}
// n_items work items of the plan: wg_per_item workgroups each
static int kz_count_launch(kz_ctx* ctx, const KzCountKernel& k, const KnnCountParams& p, int n_items) {
    const int rc = kz_raise_lds(ctx, k.fn, k.lds_bytes);
    if (rc != KZ_OK) return rc;
    KnnCountParams pc = p;
    void* args[] = {&pc};
    KZ_HIP(hipLaunchKernel(k.fn, dim3(k.wg_per_item * n_items), dim3(256), args, (size_t)k.lds_bytes, ctx->stream));
    return KZ_OK;
}

// Where the sweeps exist.  The rank-one sweeps (kz_rank_r1_sweep.h, kz_knn_reduced_sweep.h) have builds of 2 .. 24 slices; the plain
// count and emit sweeps (here, kz_radius_sweep.h) of every slice count of the fp16 tier (kz_h_slices_ok: 2 .. 24 and 32 .. 128,
// d = 17 .. 384 and 497 .. 2048).
static bool kz_sweep_operands_ok(const kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index) {
    return !query->pre && !index->pre && ctx->precision != 1 && index->dtype == KZ_F32 && query->dtype == KZ_F32 && index->metric <= KZ_COSINE &&
           query->kg == index->kg && index->n >= KZ_TILE;
}
static bool kz_rank_sweep_shapes_ok(const kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index) {
    const int n_slices = index->kg / 4;
    return kz_sweep_operands_ok(ctx, query, index) && n_slices >= 2 && n_slices <= 24;
}
static bool kz_plain_sweep_shapes_ok(const kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index) {
    return kz_sweep_operands_ok(ctx, query, index) && kz_h_slices_ok(index->kg);
}

extern "C" int kz_gold_ranks_sweep(kz_ctx* ctx, const kz_matrix* query_c, int64_t q_begin, int64_t q_count, const kz_matrix* index_c,
                                   const int64_t* d_gold, int64_t* d_rank, kz_rank_sweep_stats* stats) {
    const char* who = "kz_gold_ranks_sweep";
    kz_matrix* query = const_cast<kz_matrix*>(query_c);
    kz_matrix* index = const_cast<kz_matrix*>(index_c);
    const int rcp = kz_require_pair(who, ctx, query, q_begin, q_count, index, d_gold, d_rank);
    if (rcp != KZ_OK) return rcp;
    kz_rank_sweep_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    KZ_REQUIRE(q_count < 0x7fffffff && index->n < 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    float ms = 0;
    if (!kz_plain_sweep_shapes_ok(ctx, query, index)) {   // the whole call on the exact route
        KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        int n_listed = 0;
        const int rc = kz_gold_ranks_impl(who, ctx, query, q_begin, q_count, index, d_gold, nullptr, d_rank, &n_listed);
        if (rc != KZ_OK) return rc;
        KZ_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
        KZ_HIP(hipEventSynchronize(ctx->ev[4]));
        KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
        st.n_rows = n_listed;   // (no sweep rows, hence no fallback rows: the time of the exact route is fallback_ms)
        st.fallback_ms = ms;
        if (stats) *stats = st;
        return KZ_OK;
    }
    // (every buffer below is released when the call returns, stream-ordered, behind its last synchronisation)
    KzPoolBuf<int> fl;
    int n_list = 0;
    int rc = kz_rank_compact(ctx, q_count, index, d_gold, d_rank, fl, &n_list);
    if (rc != KZ_OK) return rc;
    st.route_taken = 1;
    st.n_rows = n_list;
    if (n_list == 0) {
        if (stats) *stats = st;
        return KZ_OK;
    }
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    // ---- the listed rows as a matrix of their own, its fp16 image beside the index's ------------------------------------------
    const int d = (int)index->d, metric = index->metric;
    const size_t row_bytes = (size_t)d * 4;
    KzPoolBuf<void> sub_raw;
    KzMatrixPtr qsub;
    rc = sub_raw.alloc(ctx, (size_t)n_list * row_bytes);
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_gather_rows_kernel, dim3(n_list), dim3(256), 0, ctx->stream, (const char*)query->raw, fl.get(), q_begin, n_list, (int64_t)row_bytes,
                       (char*)sub_raw.get(), (int64_t*)nullptr, (const int64_t*)nullptr);
    KZ_HIP(hipGetLastError());
    {
        kz_matrix* m = nullptr;
        rc = kz_matrix_create(ctx, sub_raw.get(), 2, n_list, d, query->dtype, query->metric, &m);
        qsub.reset(m);
        if (rc == KZ_OK) rc = kz_himage_ensure(qsub.get(), index);
        if (rc != KZ_OK) return rc;
    }
    const int n_qtiles = (int)qsub->n_tiles, n_ytiles = (int)index->n_tiles;
    const int64_t n_pad = (int64_t)n_qtiles * KZ_TILE;
    // ---- thresholds, counters, the log ----------------------------------------------------------------------------------------
    size_t mem_free = 0, mem_total = 0;
    KZ_HIP(hipMemGetInfo(&mem_free, &mem_total));
    long long log_cap = KZ_RANK_LOG_PER_ROW * n_list > KZ_RANK_LOG_MIN ? KZ_RANK_LOG_PER_ROW * n_list : KZ_RANK_LOG_MIN;
    if (log_cap > (long long)(mem_free / 4 / 12)) log_cap = (long long)(mem_free / 4 / 12);   // (12 bytes an entry, a quarter of what is free)
    KzPoolBuf<float2> lohi;
    KzPoolBuf<double> dbuf;   // vg [n_list] | eps [n_list]
    KzPoolBuf<int> ibuf;      // counters (16 ints: [0..1] log entries, [2..3] max ratio bits) | flag [n_pad] | band_cnt [n_pad]
    KzPoolBuf<int> fb;        // [n_list + 1]
    KzPoolBuf<i32x2e> log_meta;
    KzPoolBuf<float> log_key;
    KzPoolBuf<int4> d_work;
    rc = lohi.alloc(ctx, (size_t)n_pad * sizeof(float2));
    if (rc == KZ_OK) rc = dbuf.alloc(ctx, (size_t)n_list * 2 * sizeof(double));
    if (rc == KZ_OK) rc = ibuf.alloc(ctx, (16 + 2 * (size_t)n_pad) * sizeof(int));
    if (rc == KZ_OK) rc = fb.alloc(ctx, ((size_t)n_list + 1) * sizeof(int));
    if (rc == KZ_OK) rc = log_meta.alloc(ctx, (size_t)log_cap * sizeof(i32x2e) + 8);
    if (rc == KZ_OK) rc = log_key.alloc(ctx, (size_t)log_cap * sizeof(float) + 4);
    if (rc != KZ_OK) return rc;
    double *vg = dbuf.get(), *eps = dbuf.get() + n_list;
    unsigned long long* counters = (unsigned long long*)ibuf.get();
    int *flag = ibuf.get() + 16, *band_cnt = flag + n_pad;
    KZ_HIP(hipMemsetAsync(ibuf.get(), 0, (16 + 2 * (size_t)n_pad) * sizeof(int), ctx->stream));
    const kz_himage *qi = qsub->himg, *ii = index->himg;
    hipLaunchKernelGGL(kz_rank_band_kernel, dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, ctx->stream, (const int*)fl.get(), n_list, n_pad, q_begin, d_gold,
                       (const float*)query->raw, (const float*)index->raw, (const double*)query->sqn, (const double*)index->sqn, d, metric,
                       (const double*)qi->rowq, (const double*)ii->d_max, (const double*)ii->center->d_scale, (const double*)index->d_stats,
                       ctx->eps_scale, kz_gamma_acc_h(index->kg), lohi.get(), vg, eps, flag);
    KZ_HIP(hipGetLastError());
    // ---- the sweep: work items of kz_plan.h unchanged (query tile x index range, rounds in lockstep) ---------------------------
    const int n_slices = kz_h_nsr(index->kg);   // (the padded count the images are packed with)
    const KzCountKernel kern = kz_count_lookup(n_slices);
    if (!kern.fn) {
        kz_set_error("%s: internal: no count kernel for %d slices", who, n_slices);
        return KZ_ERR_UNSUPPORTED;
    }
    int per_cu = 1;
    rc = kz_count_occupancy(ctx, kern, &per_cu);
    if (rc != KZ_OK) return rc;
    const int slots = per_cu * ctx->n_cus;
    KzPlan pl;
    kz_plan_pass(n_qtiles, n_ytiles, slots, kz_max_pieces(16, 1), 16, 1, 1, 1, ctx->force_splits, 1, &pl);
    std::vector<KzWorkItem> hw((size_t)pl.W);   // (pageable: alive until the synchronisation behind the sweep)
    {
        const int per_xcd = (slots + 7) / 8;
        kz_plan_fill_work(pl, n_ytiles, 1, hw.data(), 4 * per_xcd > KZ_QGROUP ? 4 * per_xcd : KZ_QGROUP);
    }
    rc = d_work.alloc(ctx, (size_t)pl.W * sizeof(int4));
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemcpyAsync(d_work.get(), hw.data(), (size_t)pl.W * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    KnnCountParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.qpack = (const float*)qi->packed;
    cp.ypack = (const float*)ii->packed;
    cp.ybias = ii->bias;
    cp.work = d_work.get();
    cp.n_ytiles = n_ytiles;
    cp.lohi = lohi.get();
    cp.list = fl.get();
    cp.n_list = n_list;
    cp.rank = (long long*)d_rank;
    cp.band_cnt = band_cnt;
    cp.log_cnt = counters;
    cp.log_cap = log_cap;
    cp.log_meta = log_meta.get();
    cp.log_key = log_key.get();
    rc = kz_count_launch(ctx, kern, cp, pl.W);
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    unsigned long long n_band = 0;
    KZ_HIP(hipMemcpyAsync(&n_band, counters, 8, hipMemcpyDeviceToHost, ctx->stream));
    {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            kz_set_error("%s: the count sweep failed: %s", who, hipGetErrorString(e));
            return KZ_ERR_HIP;
        }
    }
    // ---- the band, the rows that are not trusted --------------------------------------------------------------------------------
    const bool over = n_band > (unsigned long long)log_cap;
    if (!over && n_band > 0) {
        const long long wgs = ((long long)n_band + 3) / 4;
        hipLaunchKernelGGL(kz_rank_resolve_kernel, dim3((unsigned)(wgs < 65536 ? wgs : 65536)), dim3(256), 0, ctx->stream, (const i32x2e*)log_meta.get(),
                           (const float*)log_key.get(), (long long)n_band, (const int*)fl.get(), q_begin, d_gold, (const float*)query->raw,
                           (const float*)index->raw, (const double*)query->sqn, (const double*)index->sqn, index->n, d, metric, (const double*)qi->rowq,
                           (const double*)ii->center->d_scale, (const double*)vg, (const double*)eps, (const int*)band_cnt, flag, counters + 1, d_rank);
    }
    hipLaunchKernelGGL(kz_rank_fallback_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)fl.get(), n_list, (const int*)flag, (const int*)band_cnt,
                       over ? 1 : 0, fb.get(), d_rank);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    int n_fb = 0;
    unsigned long long ratio_bits = 0;
    KZ_HIP(hipMemcpyAsync(&n_fb, fb.get() + n_list, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipMemcpyAsync(&ratio_bits, counters + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            kz_set_error("%s: resolving the band failed: %s", who, hipGetErrorString(e));
            return KZ_ERR_HIP;
        }
    }
    if (n_fb > 0) {
        rc = kz_gold_ranks_walk(who, ctx, query, q_begin, index, d_gold, nullptr, fb.get(), n_fb, d_rank);
        if (rc != KZ_OK) return rc;
    }
    KZ_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
    KZ_HIP(hipEventSynchronize(ctx->ev[6]));
    st.n_fallback_rows = n_fb;
    st.n_sweep_rows = n_list - n_fb;
    st.n_band_pairs = (int64_t)n_band;
    memcpy(&st.max_err_ratio, &ratio_bits, 8);
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
    st.sweep_ms = ms;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    st.band_ms = ms;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[6]));
    st.fallback_ms = ms;
    if (stats) *stats = st;
    return KZ_OK;
}
