// kz_fit / kz_kneighbors: one native call per HubnessReduction.fit and per .kneighbors (kiez/hubness_reduction/base.py:33-50,
// 89-105).  The decisions are kz_fit_plan.h (host-only, tested on the CPU); this file executes a plan with the library's own entry
// points -- kz_knn_dual / kz_knn / kz_split_self for the lists, kz_row_stats / kz_row_nanstats for the fit state, kz_rescale_select
// (or kz_mp_empiric + kz_select_topk + kz_cast_f64_f32) for the tail -- so every result is what a caller of those primitives gets.
#include <cstring>
#include <new>

#include "kz_common.h"
#include "kz_fit_plan.h"
#include "kz_precomputed.h"

static_assert(KZ_FP_OK == KZ_OK && KZ_FP_INVALID == KZ_ERR_INVALID && KZ_FP_UNSUPPORTED == KZ_ERR_UNSUPPORTED, "kz_fit_plan.h: status codes");
static_assert(KZ_FP_NONE == KZ_HUB_NONE && KZ_FP_CSLS == KZ_HUB_CSLS && KZ_FP_LS == KZ_HUB_LS && KZ_FP_NICDM == KZ_HUB_NICDM &&
                  KZ_FP_MP_NORMAL == KZ_HUB_MP_NORMAL && KZ_FP_MP_EMPIRIC == KZ_HUB_MP_EMPIRIC,
              "kz_fit_plan.h: hubness kinds");
static_assert(KZ_HUB_CSLS == KZ_RANK_CSLS && KZ_HUB_LS == KZ_RANK_LS && KZ_HUB_NICDM == KZ_RANK_NICDM && KZ_HUB_MP_NORMAL == KZ_RANK_MP_NORMAL,
              "the pointwise kinds share the numbering of KZ_RANK_*");

struct kz_fitted {
    kz_ctx* ctx;
    const kz_matrix* source;   // borrowed
    const kz_matrix* target;   // borrowed; == source for single source
    int kind, K, shared_sweep;
    KzFitPlan plan;
    KzPoolBuf<double> rev_d, fwd_d, t_a, t_b;
    KzPoolBuf<int64_t> rev_i, fwd_i;
    bool forward_ready;
    int n_searches;
    kz_knn_stats st_fwd, st_rev;
};

// the forward search, where the fit did not deliver the lists: kept until the object goes
static int kz_fitted_forward(kz_fitted* f) {
    if (f->forward_ready) return KZ_OK;
    const size_t half = f->plan.forward_bytes / 2;
    int rc = f->fwd_d.alloc(f->ctx, half);
    if (rc == KZ_OK) rc = f->fwd_i.alloc(f->ctx, half);
    if (rc == KZ_OK) {
        ++f->n_searches;
        rc = kz_knn(f->ctx, f->source, 0, f->plan.n_query, f->target, f->K, f->plan.forward_exclude_self, f->fwd_d.get(), f->fwd_i.get(), &f->st_fwd);
    }
    if (rc != KZ_OK) {
        f->fwd_d.reset();
        f->fwd_i.reset();
        return rc;
    }
    f->forward_ready = true;
    return KZ_OK;
}

static int kz_fit_run(kz_fitted* f) {
    kz_ctx* ctx = f->ctx;
    const KzFitPlan& p = f->plan;
    const int K = f->K;
    if (p.search == KZ_FIT_SEARCH_NONE) return KZ_OK;
    int rc = f->rev_d.alloc(ctx, p.reverse_bytes / 2);
    if (rc == KZ_OK) rc = f->rev_i.alloc(ctx, p.reverse_bytes / 2);
    if (rc != KZ_OK) return rc;
    if (p.forward_at_fit) {
        rc = f->fwd_d.alloc(ctx, p.forward_bytes / 2);
        if (rc == KZ_OK) rc = f->fwd_i.alloc(ctx, p.forward_bytes / 2);
        if (rc != KZ_OK) return rc;
    }
    if (p.search == KZ_FIT_SEARCH_DUAL) {
        ++f->n_searches;
        rc = p.larger_first ? kz_knn_dual(ctx, f->source, f->target, K, f->fwd_d.get(), f->fwd_i.get(), f->rev_d.get(), f->rev_i.get(), &f->st_fwd, &f->st_rev)
                            : kz_knn_dual(ctx, f->target, f->source, K, f->rev_d.get(), f->rev_i.get(), f->fwd_d.get(), f->fwd_i.get(), &f->st_rev, &f->st_fwd);
        if (rc != KZ_OK) return rc;
        f->forward_ready = true;
    } else if (p.search == KZ_FIT_SEARCH_SPLIT) {
        KzPoolBuf<double> all_d;
        KzPoolBuf<int64_t> all_i;
        rc = all_d.alloc(ctx, p.split_bytes / 2);
        if (rc == KZ_OK) rc = all_i.alloc(ctx, p.split_bytes / 2);
        if (rc != KZ_OK) return rc;
        ++f->n_searches;
        rc = kz_knn(ctx, f->source, 0, p.n_query, f->source, K + 1, 0, all_d.get(), all_i.get(), &f->st_fwd);
        if (rc == KZ_OK)
            rc = kz_split_self(ctx, all_d.get(), all_i.get(), p.n_query, K + 1, 0, f->rev_d.get(), f->rev_i.get(), f->fwd_d.get(), f->fwd_i.get());
        if (rc != KZ_OK) return rc;
        f->forward_ready = true;
    } else {
        ++f->n_searches;
        rc = kz_knn(ctx, f->target, 0, p.n_index, f->source, K, 0, f->rev_d.get(), f->rev_i.get(), &f->st_rev);
        if (rc != KZ_OK) return rc;
    }
    // the fit state of the reduction, from the reverse lists
    if (p.n_state >= 1) {
        rc = f->t_a.alloc(ctx, (size_t)p.n_index * 8);
        if (rc == KZ_OK && p.n_state == 2) rc = f->t_b.alloc(ctx, (size_t)p.n_index * 8);
        if (rc != KZ_OK) return rc;
        if (f->kind == KZ_HUB_MP_NORMAL)   // mutual_proximity.py:102-103
            rc = kz_row_nanstats(ctx, f->rev_d.get(), p.n_index, K, f->t_a.get(), f->t_b.get());
        else if (f->kind == KZ_HUB_LS)     // local_scaling.py:136
            rc = kz_row_stats(ctx, f->rev_d.get(), p.n_index, K, nullptr, nullptr, f->t_a.get());
        else                               // csls.py:90, local_scaling.py:143
            rc = kz_row_stats(ctx, f->rev_d.get(), p.n_index, K, f->t_a.get(), nullptr, nullptr);
    }
    return rc;
}

extern "C" {

int kz_fit(kz_ctx* ctx, const kz_matrix* source, const kz_matrix* target, int hubness, int n_candidates, int shared_sweep, kz_fitted** out) {
    KZ_REQUIRE(ctx && source && out, "kz_fit: null argument");
    *out = nullptr;
    const bool single = target == nullptr || target == source;
    const kz_matrix* t = single ? source : target;
    KZ_REQUIRE(!source->raw_only && !t->raw_only, "kz_fit: a rows-only matrix (kz_matrix_create rows_on_device = 3) cannot be searched");
    KzFitIn in{};
    in.n_source = source->n;
    in.n_target = t->n;
    in.single_source = single ? 1 : 0;
    in.K = n_candidates;
    in.kind = hubness;
    in.shared_sweep = shared_sweep ? 1 : 0;
    in.precomputed = (source->pre || t->pre) ? 1 : 0;
    in.agree = (source->ctx == ctx && t->ctx == ctx && source->d == t->d && source->dtype == t->dtype && source->metric == t->metric &&
                kz_metric_params_match(source, t))
                   ? 1
                   : 0;
    const KzFitPlan plan = kz_fit_plan(in);
    if (plan.status != KZ_FP_OK) {
        kz_set_error("kz_fit: %s (n_source=%lld, n_target=%lld, n_candidates=%d, hubness=%d)", plan.why, (long long)in.n_source,
                     (long long)in.n_target, n_candidates, hubness);
        return plan.status;
    }
    KZ_REQUIRE(source->ctx == ctx, "kz_fit: the matrix belongs to a different context");
    KZ_HIP(hipSetDevice(ctx->device));
    kz_fitted* f = new (std::nothrow) kz_fitted();
    if (!f) {
        kz_set_error("kz_fit: out of host memory");
        return KZ_ERR_NOMEM;
    }
    f->ctx = ctx;
    f->source = source;
    f->target = t;
    f->kind = hubness;
    f->K = n_candidates;
    f->shared_sweep = in.shared_sweep;
    f->plan = plan;
    f->forward_ready = false;
    f->n_searches = 0;
    memset(&f->st_fwd, 0, sizeof(f->st_fwd));
    memset(&f->st_rev, 0, sizeof(f->st_rev));
    const int rc = kz_fit_run(f);
    if (rc != KZ_OK) {
        delete f;   // (the owners hand their buffers back)
        return rc;
    }
    *out = f;
    return KZ_OK;
}

int kz_kneighbors(kz_fitted* f, int k, int out_dtype, void* d_dist, int64_t* d_ind) {
    KZ_REQUIRE(f && d_dist && d_ind, "kz_kneighbors: null argument");
    KZ_REQUIRE(k >= 1 && k <= f->K, "kz_kneighbors: k=%d must be in [1, n_candidates=%d]", k, f->K);
    KZ_REQUIRE(out_dtype == KZ_F64 || out_dtype == KZ_F32, "kz_kneighbors: out_dtype must be KZ_F64 or KZ_F32, got %d", out_dtype);
    kz_ctx* ctx = f->ctx;
    KZ_HIP(hipSetDevice(ctx->device));
    const KzFitPlan& p = f->plan;
    const int64_t n = p.n_query;
    if (p.tail == KZ_FIT_TAIL_KNN) {
        ++f->n_searches;
        if (out_dtype == KZ_F64)
            return kz_knn(ctx, f->source, 0, n, f->target, k, p.forward_exclude_self, (double*)d_dist, d_ind, &f->st_fwd);
        KzPoolBuf<double> od;
        int rc = od.alloc(ctx, (size_t)n * (size_t)k * 8);
        if (rc == KZ_OK) rc = kz_knn(ctx, f->source, 0, n, f->target, k, p.forward_exclude_self, od.get(), d_ind, &f->st_fwd);
        if (rc == KZ_OK) rc = kz_cast_f64_f32(ctx, od.get(), (float*)d_dist, n * (int64_t)k);
        return rc;
    }
    int rc = kz_fitted_forward(f);
    if (rc != KZ_OK) return rc;
    if (p.tail == KZ_FIT_TAIL_FUSED)
        return kz_rescale_select(ctx, f->fwd_d.get(), f->fwd_i.get(), n, f->K, k, f->kind, f->t_a.get(), f->t_b.get(), out_dtype, d_dist, d_ind);
    // MutualProximity 'empiric': its value depends on list membership -- the wave-per-row kernel, then the sort and the cast
    KzPoolBuf<double> w, od;
    rc = w.alloc(ctx, (size_t)n * (size_t)f->K * 8);
    if (rc == KZ_OK) rc = kz_mp_empiric(ctx, f->fwd_d.get(), f->fwd_i.get(), n, f->K, f->rev_d.get(), f->rev_i.get(), p.n_index, f->K, w.get());
    if (rc != KZ_OK) return rc;
    if (out_dtype == KZ_F64) return kz_select_topk(ctx, w.get(), f->fwd_i.get(), n, f->K, k, (double*)d_dist, d_ind);
    rc = od.alloc(ctx, (size_t)n * (size_t)k * 8);
    if (rc == KZ_OK) rc = kz_select_topk(ctx, w.get(), f->fwd_i.get(), n, f->K, k, od.get(), d_ind);
    if (rc == KZ_OK) rc = kz_cast_f64_f32(ctx, od.get(), (float*)d_dist, n * (int64_t)k);
    return rc;
}

int kz_fitted_info(const kz_fitted* f, kz_fit_info* out) {
    KZ_REQUIRE(f && out, "kz_fitted_info: null argument");
    memset(out, 0, sizeof(*out));
    out->n_source = f->plan.n_query;
    out->n_target = f->plan.n_index;
    out->n_candidates = f->K;
    out->hubness = f->kind;
    out->single_source = f->target == f->source ? 1 : 0;
    out->shared_sweep = f->shared_sweep;
    out->search = f->plan.search;
    out->larger_first = f->plan.larger_first;
    out->tail = f->plan.tail;
    out->fused = f->plan.fused;
    out->forward_ready = f->forward_ready ? 1 : 0;
    out->n_searches = f->n_searches;
    out->stats_forward = f->st_fwd;
    out->stats_reverse = f->st_rev;
    return KZ_OK;
}

int kz_fitted_state(const kz_fitted* f, int what, const void** d_ptr, int64_t* rows, int* cols) {
    KZ_REQUIRE(f && d_ptr, "kz_fitted_state: null argument");
    const void* ptr = nullptr;
    int64_t r = 0;
    int c = 0;
    switch (what) {
        case KZ_FIT_REVERSE_DIST: ptr = f->rev_d.get(); r = f->plan.n_index; c = f->K; break;
        case KZ_FIT_REVERSE_IND: ptr = f->rev_i.get(); r = f->plan.n_index; c = f->K; break;
        case KZ_FIT_FORWARD_DIST: ptr = f->forward_ready ? f->fwd_d.get() : nullptr; r = f->plan.n_query; c = f->K; break;
        case KZ_FIT_FORWARD_IND: ptr = f->forward_ready ? f->fwd_i.get() : nullptr; r = f->plan.n_query; c = f->K; break;
        case KZ_FIT_STATE_A: ptr = f->t_a.get(); r = f->plan.n_index; c = 1; break;
        case KZ_FIT_STATE_B: ptr = f->t_b.get(); r = f->plan.n_index; c = 1; break;
        default: kz_set_error("kz_fitted_state: unknown array %d", what); return KZ_ERR_INVALID;
    }
    *d_ptr = ptr;
    if (rows) *rows = ptr ? r : 0;
    if (cols) *cols = ptr ? c : 0;
    return KZ_OK;
}

int kz_fitted_destroy(kz_fitted* f) {
    if (!f) return KZ_OK;
    KZ_HIP(hipSetDevice(f->ctx->device));
    delete f;
    return KZ_OK;
}

}  // extern "C"
