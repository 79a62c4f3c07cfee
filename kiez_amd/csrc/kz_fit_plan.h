// Host-only PLAN of a whole fit / kneighbors (no HIP in this header, like kz_plan.h and kz_route.h: tests/host/fit_plan_sanitize.cpp
// compiles it with g++ -fsanitize=address,undefined on the CPU).  kz_fit.hip includes it for the product.
//
// What kz_fit / kz_kneighbors DECIDE is here -- a pure function from sizes, kind and flags to a plan record: which searches fit
// runs, whether the forward lists come out of fit, which tail kneighbors runs, the buffer sizes, and every refusal, before anything
// is allocated or launched.  What they EXECUTE (the searches, the state kernels, the tail) is kz_fit.hip.  The rules restate the
// pipeline of kiez_amd/hubness_reduction.py (HubnessReduction.fit / kneighbors_device) and SklearnNN.kneighbors_device_both.
#pragma once
#include <cstddef>
#include <cstdint>

// (the values of include/kiez_amd.h, repeated so that this header stands alone; kz_fit.hip asserts that they agree)
enum { KZ_FP_OK = 0, KZ_FP_INVALID = 1, KZ_FP_UNSUPPORTED = 3 };
enum { KZ_FP_NONE = 0, KZ_FP_CSLS = 1, KZ_FP_LS = 2, KZ_FP_NICDM = 3, KZ_FP_MP_NORMAL = 4, KZ_FP_MP_EMPIRIC = 5 };

// which searches kz_fit runs
enum {
    KZ_FIT_SEARCH_NONE = 0,      // no reduction: nothing is searched before kz_kneighbors
    KZ_FIT_SEARCH_DUAL = 1,      // two-sided, shared sweep: kz_knn_dual, the larger matrix first (it searches twice by itself where the sweep does not apply)
    KZ_FIT_SEARCH_REVERSE = 2,   // the reverse kz_knn only (target rows against the source, nothing stripped); the forward search runs at the first kz_kneighbors
    KZ_FIT_SEARCH_SPLIT = 3      // single source: ONE kz_knn(source, source, K + 1, exclude_self = 0) + kz_split_self
};
// which tail kz_kneighbors runs on the forward lists
enum {
    KZ_FIT_TAIL_KNN = 0,        // no reduction: one kz_knn for k neighbours (+ the cast)
    KZ_FIT_TAIL_FUSED = 1,      // kz_rescale_select (the fused kernel up to KZ_FIT_FUSED_MAX_K candidates, the kernel sequence inside the call beyond)
    KZ_FIT_TAIL_EMPIRIC = 2     // kz_mp_empiric + kz_select_topk + the cast
};

constexpr int KZ_FIT_MAX_K = 4095;          // neighbours per query a search returns beside the row itself (SklearnNN's limit)
constexpr int KZ_FIT_SPLIT_MAX_K1 = 110;    // K + 1 of the single-source split: what ONE fused list keeps
constexpr int KZ_FIT_FUSED_MAX_K = 128;     // candidates per row of the fused rescale + select kernel

struct KzFitIn {
    int64_t n_source;
    int64_t n_target;      // ignored for single-source
    int single_source;     // target == NULL
    int K;                 // n_candidates
    int kind;              // KZ_FP_*
    int shared_sweep;
    int precomputed;       // either matrix is a view of a precomputed distance matrix
    int agree;             // the two matrices have the same context, feature count, element type, metric and metric parameters
};

struct KzFitPlan {
    int status;            // KZ_FP_OK, or the refusal (then `why` says it and nothing else is set)
    const char* why;
    int search;            // KZ_FIT_SEARCH_*
    int larger_first;      // KZ_FIT_SEARCH_DUAL: 1 = the SOURCE is kz_knn_dual's a (n_source >= n_target), 0 = the target is
    int forward_at_fit;    // the forward lists exist when kz_fit returns
    int forward_exclude_self;   // exclude_self of a forward kz_knn (single source)
    int tail;              // KZ_FIT_TAIL_*
    int fused;             // KZ_FIT_TAIL_FUSED: 1 = the fused kernel serves K, 0 = the sequence inside kz_rescale_select
    int n_state;           // index-side state vectors of n_index doubles: 0 (none, MP empiric), 1, 2 (MP normal)
    int64_t n_query;       // rows of the forward lists (the source)
    int64_t n_index;       // rows of the reverse lists and of the state (the target; the source again for single-source)
    size_t reverse_bytes;  // of the reverse lists, distances + ids: 16 n_index K (0: no reduction)
    size_t forward_bytes;  // of the forward lists the fitted object keeps: 16 n_query K (0: no reduction)
    size_t state_bytes;    // 8 n_index n_state
    size_t split_bytes;    // KZ_FIT_SEARCH_SPLIT: the transient [n, K + 1] result, distances + ids
};

static inline KzFitPlan kz_fit_refuse(int status, const char* why) {
    KzFitPlan p{};
    p.status = status;
    p.why = why;
    return p;
}

static inline KzFitPlan kz_fit_plan(const KzFitIn& in) {
    if (in.kind < KZ_FP_NONE || in.kind > KZ_FP_MP_EMPIRIC) return kz_fit_refuse(KZ_FP_INVALID, "unknown hubness kind");
    if (in.n_source < 1 || (!in.single_source && in.n_target < 1)) return kz_fit_refuse(KZ_FP_INVALID, "an empty matrix");
    if (in.K < 1) return kz_fit_refuse(KZ_FP_INVALID, "n_candidates must be >= 1");
    if (in.kind != KZ_FP_NONE && in.K < 2)
        return kz_fit_refuse(KZ_FP_INVALID, "cannot perform hubness reduction with a single candidate per query");
    const int64_t k_max = in.single_source ? in.n_source - 1 : (in.n_source < in.n_target ? in.n_source : in.n_target);
    if ((int64_t)in.K > k_max)
        return kz_fit_refuse(KZ_FP_INVALID, in.single_source ? "n_candidates exceeds n - 1 (single source: the row itself is no neighbour)"
                                                             : "n_candidates exceeds the rows of a side (clamping is the caller's business)");
    if (in.K > KZ_FIT_MAX_K) return kz_fit_refuse(KZ_FP_UNSUPPORTED, "n_candidates above 4095");
    if (in.precomputed) return kz_fit_refuse(KZ_FP_UNSUPPORTED, "a precomputed distance matrix (search its two views with kz_knn)");
    if (!in.single_source && !in.agree)
        return kz_fit_refuse(KZ_FP_INVALID, "source and target disagree (context, feature count, element type, metric or its parameters)");

    KzFitPlan p{};
    p.status = KZ_FP_OK;
    p.why = "";
    p.n_query = in.n_source;
    p.n_index = in.single_source ? in.n_source : in.n_target;
    p.forward_exclude_self = in.single_source ? 1 : 0;
    if (in.kind == KZ_FP_NONE) {
        p.search = KZ_FIT_SEARCH_NONE;
        p.tail = KZ_FIT_TAIL_KNN;
        return p;
    }
    if (!in.shared_sweep) {
        p.search = KZ_FIT_SEARCH_REVERSE;
    } else if (!in.single_source) {
        p.search = KZ_FIT_SEARCH_DUAL;
        p.larger_first = in.n_source >= in.n_target ? 1 : 0;
    } else if ((int64_t)in.K + 1 <= in.n_source && in.K + 1 <= KZ_FIT_SPLIT_MAX_K1) {
        p.search = KZ_FIT_SEARCH_SPLIT;
        p.split_bytes = (size_t)16 * (size_t)in.n_source * (size_t)(in.K + 1);
    } else {
        p.search = KZ_FIT_SEARCH_REVERSE;   // (then the forward search with exclude_self = 1, at the first kz_kneighbors)
    }
    p.forward_at_fit = p.search == KZ_FIT_SEARCH_DUAL || p.search == KZ_FIT_SEARCH_SPLIT;
    if (in.kind == KZ_FP_MP_EMPIRIC) {
        p.tail = KZ_FIT_TAIL_EMPIRIC;
        p.n_state = 0;
    } else {
        p.tail = KZ_FIT_TAIL_FUSED;
        p.fused = in.K <= KZ_FIT_FUSED_MAX_K ? 1 : 0;
        p.n_state = in.kind == KZ_FP_MP_NORMAL ? 2 : 1;
    }
    p.reverse_bytes = (size_t)16 * (size_t)p.n_index * (size_t)in.K;
    p.forward_bytes = (size_t)16 * (size_t)p.n_query * (size_t)in.K;
    p.state_bytes = (size_t)8 * (size_t)p.n_index * (size_t)p.n_state;
    return p;
}
