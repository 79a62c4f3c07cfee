// KZ_PRECOMPUTED (kz_precomputed.hip): the caller's distance matrix as the value matrix of the exact stage.  Two kz_matrix handles --
// the rows view and the columns view -- share ONE kz_precomputed; a handle owns nothing else.  What the other translation units
// need: the pairing rule (kz_require_pair), the deferred verdict of the validation kernel, the value batch (kz_exact_distances)
// and the release (kz_matrix_destroy).
#pragma once
#include "kz_common.h"

struct kz_precomputed {
    void* values;        // [n_rows, n_cols] dtype, row-major: values[i, j] = distance from "source" row i to "target" row j
    bool borrowed;       // values is the caller's buffer (values_on_device = 2), not ours to free
    int64_t n_rows, n_cols;
    int dtype;
    int refs;            // handles alive (2 after creation): the last kz_matrix_destroy frees the storage
    int* d_flags;        // device [4] int, written by the validation kernel: [0] NaN or infinity seen, [1] a value < 0 seen
    bool checked;        // the flags have been read back and were clean (kz_precomputed_check)
};

// Waits for the validation kernel and reads its verdict: KZ_ERR_NONFINITE (NaN, +-inf), KZ_ERR_INVALID (a value < 0; -0.0 is fine),
// else KZ_OK -- remembered, so that only the first search of a matrix waits.  Called by kz_matrix_create_precomputed for host values
// and by kz_require_pair for device values.
int kz_precomputed_check(kz_ctx* ctx, kz_precomputed* p);
// vals [nb][index->n] of the listed rows q_begin + fl[b0 .. b0 + nb) of `query` (a precomputed pair, as kz_precomputed_require_pair
// admits it): the matrix entries widened to float64.  Launch errors are the caller's hipGetLastError, as for every value kernel.
void kz_precomputed_launch_values(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t q_begin, const kz_matrix* query, const kz_matrix* index,
                                  double* vals);
// kz_matrix_destroy's part: drops the handle's reference (nothing happens for an embedding matrix)
void kz_precomputed_release(kz_matrix* m);

// A precomputed handle pairs only with the OTHER view of the same storage.
static inline int kz_precomputed_require_pair(const char* who, const kz_matrix* query, const kz_matrix* index) {
    if (!query->pre && !index->pre) return KZ_OK;
    KZ_REQUIRE(query->pre && index->pre,
               "%s: a precomputed distance matrix pairs with its own other view (kz_matrix_create_precomputed), not with an embedding matrix", who);
    KZ_REQUIRE(query->pre == index->pre, "%s: the two handles are views of different precomputed matrices", who);
    KZ_REQUIRE(query->pre_cols != index->pre_cols,
               "%s: the same view of a precomputed matrix on both sides (query = one view, index = the other)", who);
    return KZ_OK;
}
// The entry points that read embeddings (kz_knn_dual, kz_pair_values, kz_dsl_fit, kz_dsl_transform, the metric parameters)
#define KZ_REFUSE_PRECOMPUTED(who, m)                                                                                                  \
    KZ_REQUIRE(!(m)->pre, "%s: not available for a precomputed distance matrix (metric='precomputed' holds no embeddings)", who)
