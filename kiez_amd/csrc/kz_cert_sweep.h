// THE CERTIFIED fp16 SWEEP, HOST DRIVER AND SHARED DEVICE PIECES.  Four entry points run the same scheme (DESIGN.md sections 3.1c,
// 3.1d, 3.1j): an fp16 MFMA sweep over the packed images decides WHICH pairs need an exact value, a float64 pass resolves exactly
// those, the rounding bound is checked on every entry, and the exact route is the fallback:
//   kz_gold_ranks_sweep (kz_rank_sweep.h), kz_gold_ranks_reduced_sweep (kz_rank_r1_sweep.h), kz_radius_neighbors_sweep
//   (kz_radius_sweep.h), kz_knn_reduced_sweep (kz_knn_reduced_sweep.h).
// What they share lives here, once:
//   KzSweepQuery      -- the query-side image: the query's own, or the listed rows / the row range as a matrix of their own
//   KzSweepLog        -- the candidate log: capacity (kz_plan_log_capacity), entries, the 16-int counter block, the call's extras
//   kz_cert_lookup    -- a build by slice count, from the per-unit lookups
//   kz_cert_plan      -- occupancy, the work table of kz_plan_sweep_work, its upload
//   kz_cert_launch    -- the launch of any of the sweep kernels
//   kz_cert_sync, kz_cert_order_log, kz_cert_exact_route
//   device: kz_round_below / kz_round_above (an interval edge, outward), kz_run_lower (a row's run of the ordered log),
//           kz_bound_holds (the bound's own check of one entry)
#pragma once
#include "kz_knn_cntx16.h"   // (KzCountKernel, KnnCountParams, KnnEmitParams, KZ_EMIT_ABOVE)
#include "kz_plan.h"

// Log size, sizing choices, not tuned figures: 64 entries a row (kz_knn_reduced_sweep: 4 k where that is more), at least 2^20.
constexpr long long KZ_CERT_LOG_PER_ROW = 64;
constexpr long long KZ_CERT_LOG_MIN = 1ll << 20;

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// An interval edge in float: rounded outward and one float step further (the infinity of its own direction stays).
__device__ __forceinline__ float kz_round_below(double want) {
    float f = (float)want;
    if ((double)f > want) f = nextafterf(f, -INFINITY);
    return nextafterf(f, -INFINITY);
}
__device__ __forceinline__ float kz_round_above(double want) {
    float f = (float)want;
    if ((double)f < want) f = nextafterf(f, INFINITY);
    return nextafterf(f, INFINITY);
}

// The first place of row_key [n] (ascending) whose key is >= key: row q's run of an ordered log is [lower(q), lower(q + 1)).
__device__ __forceinline__ int kz_run_lower(const int* __restrict__ row_key, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (row_key[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The bound's own check of one entry: |approx - exact| / eps <= 1, approx the sweep's key in exact key units.  The largest ratio of
// the launch is kept as bits (non-negative: ordered as integers; a NaN ratio is left out and fails the check).
__device__ __forceinline__ bool kz_bound_holds(double approx, double exact, double eps, unsigned long long* __restrict__ max_ratio_bits) {
    const double ratio = fabs(approx - exact) / eps;
    if (ratio == ratio) atomicMax(max_ratio_bits, (unsigned long long)__double_as_longlong(ratio));
    return ratio <= 1.0;
}

// Keys of the first sort pass of kz_cert_order_log: the index row of every log entry, and the entry's place.
__global__ __launch_bounds__(256) void kz_radius_index_keys_kernel(const i32x2e* __restrict__ log_meta, int n, int* __restrict__ key, int* __restrict__ pos) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        key[e] = log_meta[e].y;
        pos[e] = (int)e;
    }
}
// Keys of the second pass: the query row of the entry the first pass put at place e.
__global__ __launch_bounds__(256) void kz_radius_row_keys_kernel(const i32x2e* __restrict__ log_meta, int n, const int* __restrict__ pos, int* __restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) key[e] = log_meta[pos[e]].x & ~KZ_EMIT_ABOVE;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// Where the sweeps exist.  The rank-one sweeps (kz_rank_r1_sweep.h, kz_knn_reduced_sweep.h) have builds of 2 .. 24 slices; the plain
// count and emit sweeps (kz_rank_sweep.h, kz_radius_sweep.h) of every slice count of the fp16 tier (kz_h_slices_ok: 2 .. 24 and
// 32 .. 128, d = 17 .. 384 and 497 .. 2048).
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

// Synchronise; an error names the stage that was running.
static int kz_cert_sync(kz_ctx* ctx, const char* who, const char* stage) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) return KZ_OK;
    kz_set_error("%s: %s failed: %s", who, stage, hipGetErrorString(e));
    return KZ_ERR_HIP;
}

// The whole call on the exact route: exact() runs it, its time -- read-backs included -- goes to *fallback_ms.
template <class F>
static int kz_cert_exact_route(kz_ctx* ctx, double* fallback_ms, F exact) {
    KZ_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    const int rc = exact();
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
    KZ_HIP(hipEventSynchronize(ctx->ev[6]));
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[5], ctx->ev[6]));
    *fallback_ms = ms;
    return KZ_OK;
}

// The query side of a sweep: n_rows rows of `query` from q_begin on -- rows q_begin + list[r] where the caller has a row list --
// as the matrix m whose fp16 image (beside the index's) the sweep reads.  A row list always gathers; a whole range uses the query's
// own image; any other range is gathered through the identity list.  Every buffer is released with the owner, stream-ordered.
struct KzSweepQuery {
    kz_matrix* m = nullptr;
    int n_rows = 0, n_qtiles = 0;
    int64_t n_pad = 0;   // rows of the image: whole tiles

    int init(kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int n, const int* list, kz_matrix* index) {
        ctx_ = ctx;
        n_rows = n;
        list_ = list;
        m = query;
        if (list || q_begin != 0 || n != query->n) {
            const size_t row_bytes = (size_t)index->d * 4;
            int rc = sub_raw_.alloc(ctx, (size_t)n * row_bytes);
            if (rc == KZ_OK) rc = identity(&list);
            if (rc != KZ_OK) return rc;
            hipLaunchKernelGGL(kz_gather_rows_kernel, dim3(n), dim3(256), 0, ctx->stream, (const char*)query->raw, list, q_begin, n, (int64_t)row_bytes,
                               (char*)sub_raw_.get(), (int64_t*)nullptr, (const int64_t*)nullptr);
            KZ_HIP(hipGetLastError());
            rc = kz_matrix_create(ctx, sub_raw_.get(), 2, n, (int)index->d, query->dtype, query->metric, &m);
            sub_.reset(m);
            if (rc != KZ_OK) return rc;
        }
        const int rc = kz_himage_ensure(m, index);
        if (rc != KZ_OK) return rc;
        n_qtiles = (int)m->n_tiles;
        n_pad = (int64_t)n_qtiles * KZ_TILE;
        return KZ_OK;
    }
    // *out = the row list: the caller's, else the identity 0 .. n_rows - 1, made when first asked for
    int identity(const int** out) {
        if (!list_) {
            const int rc = iota_.alloc(ctx_, (size_t)n_rows * sizeof(int));
            if (rc != KZ_OK) return rc;
            hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx_->stream, iota_.get(), n_rows);
            list_ = iota_.get();
        }
        *out = list_;
        return KZ_OK;
    }

private:
    kz_ctx* ctx_ = nullptr;
    const int* list_ = nullptr;
    KzPoolBuf<void> sub_raw_;
    KzPoolBuf<int> iota_;
    KzMatrixPtr sub_;
};

// The candidate log of a sweep: cap entries {meta, key} (the kernels write one vector past the count they reserve: + 8 / + 4 bytes)
// and words [16 + n_extra]: the counter block -- [0..1] log entries, [2..3] max ratio bits, from [4] on the call's own -- and behind
// it the call's per-row extras.  The caller clears the words (the kernel or memset it always used).
struct KzSweepCounters {
    unsigned long long n_log, ratio_bits;
    int flag, pad;
};
struct KzSweepLog {
    long long cap = 0;
    size_t n_words = 0;
    KzPoolBuf<int> words;
    KzPoolBuf<i32x2e> meta;
    KzPoolBuf<float> key;

    int alloc(kz_ctx* ctx, long long per_row, long long n_rows, bool fits_int, size_t n_extra) {
        size_t mem_free = 0, mem_total = 0;
        KZ_HIP(hipMemGetInfo(&mem_free, &mem_total));
        cap = kz_plan_log_capacity(per_row, n_rows, KZ_CERT_LOG_MIN, mem_free, fits_int);
        n_words = 16 + n_extra;
        int rc = words.alloc(ctx, n_words * sizeof(int));
        if (rc == KZ_OK) rc = meta.alloc(ctx, (size_t)cap * sizeof(i32x2e) + 8);
        if (rc == KZ_OK) rc = key.alloc(ctx, (size_t)cap * sizeof(float) + 4);
        return rc;
    }
    unsigned long long* counters() const { return (unsigned long long*)words.get(); }
    int* extra() const { return words.get() + 16; }
    // the head of the counter block as the emit sweeps lay it out, behind everything queued so far (`stage`: kz_cert_sync's)
    int read(kz_ctx* ctx, const char* who, const char* stage, KzSweepCounters* h) const {
        KZ_HIP(hipMemcpyAsync(h, words.get(), sizeof(*h), hipMemcpyDeviceToHost, ctx->stream));
        return kz_cert_sync(ctx, who, stage);
    }
};

// Behind the launch of an emit-style sweep (ev[3] was recorded where the call began): the counters, and into the call's statistics
// the sweep's time, the log's entries and whether it overflowed -- then nothing of the log is used.
template <class Stats>
static int kz_cert_sweep_done(kz_ctx* ctx, const char* who, const KzSweepLog& log, KzSweepCounters* h, Stats* st) {
    KZ_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    const int rc = log.read(ctx, who, "the sweep", h);
    if (rc != KZ_OK) return rc;
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
    st->sweep_ms = ms;
    st->n_candidates = (int64_t)h->n_log;
    st->overflowed = h->n_log > (unsigned long long)log.cap ? 1 : 0;
    return KZ_OK;
}

// A build by slice count (kz_h_nsr) from the lookups of its units: lo / hi (2 .. 24), the wide rows (32 .. 64), the parity-split
// builds (80 .. 128) where the family has them.  A count without a build gets the empty descriptor.
typedef KzCountKernel (*KzUnitLookup)(int n_slices);
static KzCountKernel kz_cert_lookup(int n_slices, KzUnitLookup lo, KzUnitLookup hi, KzUnitLookup wide = nullptr, KzUnitLookup split = nullptr) {
    KzUnitLookup unit = n_slices > 64 ? split : n_slices > 24 ? wide : n_slices <= KZ_CNT_WPS3_MAX ? lo : hi;
    return unit ? unit(n_slices) : KzCountKernel{};
}

// The sweep kernels are no entries of kz_sweep_kernel's table (whose contract is "lists of K'"): an occupancy query and a launcher
// of their own.  The builds of 2 .. 24 slices stay below 64 KiB of LDS; the parity-split builds take 97.5 KiB, and BOTH the query
// and the launch raise the function's limit first (kz_raise_lds: neither depends on the other).
static int kz_cert_occupancy(kz_ctx* ctx, const KzCountKernel& k, int* blocks_per_cu) {
    const int rc = kz_raise_lds(ctx, k.fn, k.lds_bytes);
    if (rc != KZ_OK) return rc;
    int nb = 0;
    KZ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, 256, k.lds_bytes));
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return KZ_OK;
}
// n_items work items of the plan: wg_per_item workgroups each.  P: the kernel's parameter struct.
template <class P>
static int kz_cert_launch(kz_ctx* ctx, const KzCountKernel& k, const P& p, int n_items) {
    const int rc = kz_raise_lds(ctx, k.fn, k.lds_bytes);
    if (rc != KZ_OK) return rc;
    P pc = p;
    void* args[] = {&pc};
    KZ_HIP(hipLaunchKernel(k.fn, dim3(k.wg_per_item * n_items), dim3(256), args, (size_t)k.lds_bytes, ctx->stream));
    return KZ_OK;
}

// The work items of a sweep (kz_plan.h unchanged: query tile x index range, rounds in lockstep), on the device.  `what` names the
// kernel family in the error for a slice count without a build.
struct KzSweepWork {
    KzPlan pl;
    std::vector<KzWorkItem> hw;   // (pageable: alive until the synchronisation behind the sweep)
    KzPoolBuf<int4> d_work;
};
static int kz_cert_plan(const char* who, kz_ctx* ctx, const KzCountKernel& kern, const char* what, int n_slices, int n_qtiles, int n_ytiles,
                        KzSweepWork* w) {
    if (!kern.fn) {
        kz_set_error("%s: internal: no %s kernel for %d slices", who, what, n_slices);
        return KZ_ERR_UNSUPPORTED;
    }
    int per_cu = 1;
    int rc = kz_cert_occupancy(ctx, kern, &per_cu);
    if (rc != KZ_OK) return rc;
    kz_plan_sweep_work(n_qtiles, n_ytiles, per_cu * ctx->n_cus, kz_max_pieces(16, 1), ctx->force_splits, &w->pl, &w->hw);
    rc = w->d_work.alloc(ctx, (size_t)w->pl.W * sizeof(int4));
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemcpyAsync(w->d_work.get(), w->hw.data(), (size_t)w->pl.W * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    return KZ_OK;
}

// An emit log of n > 0 entries ordered by (query row, index row): two stable passes of kz_sort_pairs_f32_i32 (kz_lists_combine's
// scheme; the sort moves the keys as bit patterns: non-negative ints come back as they went in, ordered as integers) -- by index
// row, then by query row.  Place e of the order is entry pos()[e], row_key()[e] its query row.
struct KzLogOrder {
    KzPoolBuf<int> ka, kb, pa, pb;
    const int* row_key() const { return kb.get(); }
    const int* pos() const { return pa.get(); }
};
static int kz_cert_order_log(kz_ctx* ctx, const i32x2e* log_meta, int n, KzLogOrder* o) {
    int rc = o->ka.alloc(ctx, (size_t)n * 4);
    if (rc == KZ_OK) rc = o->kb.alloc(ctx, (size_t)n * 4);
    if (rc == KZ_OK) rc = o->pa.alloc(ctx, (size_t)n * 4);
    if (rc == KZ_OK) rc = o->pb.alloc(ctx, (size_t)n * 4);
    if (rc != KZ_OK) return rc;
    const dim3 grid(kz_blocks(n, 4096)), wg(256);
    // ka = keys, pa = places -> kb, pb; then ka = the query rows of the places pb -> kb = row keys, pa = places
    hipLaunchKernelGGL(kz_radius_index_keys_kernel, grid, wg, 0, ctx->stream, log_meta, n, o->ka.get(), o->pa.get());
    KZ_HIP(hipGetLastError());
    rc = kz_sort_pairs_f32_i32(ctx, reinterpret_cast<const float*>(o->ka.get()), reinterpret_cast<float*>(o->kb.get()), o->pa.get(), o->pb.get(), n, 0);
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_radius_row_keys_kernel, grid, wg, 0, ctx->stream, log_meta, n, (const int*)o->pb.get(), o->ka.get());
    KZ_HIP(hipGetLastError());
    return kz_sort_pairs_f32_i32(ctx, reinterpret_cast<const float*>(o->ka.get()), reinterpret_cast<float*>(o->kb.get()), o->pb.get(), o->pa.get(), n, 0);
}
