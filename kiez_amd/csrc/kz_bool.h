// scipy's boolean metrics (KZ_JACCARD .. KZ_YULE) on a bit-packed image of the rows (kz_bool.hip).
// scikit-learn sends these names through pairwise_distances: the rows cast to bool (x != 0: -0.0 is false), scipy's cdist, float64
// values whatever the input dtype.  A pair's value is a function of four integers -- ntt = popcount(x & y) and the rows' own counts
// nx, ny give them all -- and one float64 division; tests/boolean_restate.py restates the expressions and checks them against
// scikit-learn bit for bit.
#pragma once
#include "kz_common.h"

__host__ __device__ __forceinline__ bool kz_is_bool_metric(int metric) { return metric >= KZ_JACCARD && metric <= KZ_YULE; }

// The value the search ranks a pair by: n features, nx / ny true features of the two rows, ntt features true in both.  Every
// integer (and yule's products, below 2^32 for n <= 65536) is exact in float64, so each value is ONE rounded division -- scipy's bits.
// dice and sokalsneath are 0 / 0 between two all-false rows: that NaN is ranked as +inf (the selection kernels put (+inf, row) after
// every finite value, none of the seven metrics reaches +inf otherwise) and kz_output_distance turns it back into NaN.
__device__ __forceinline__ double kz_bool_finish(int metric, int n, int nx, int ny, int ntt) {
    const double tt = (double)ntt;
    const double df = (double)(nx + ny - 2 * ntt);   // ndf = ntf + nft
    double v;
    switch (metric) {
    case KZ_JACCARD:
        v = (tt + df == 0.0) ? 0.0 : df / (tt + df);
        break;
    case KZ_DICE:
        v = df / (2.0 * tt + df);
        break;
    case KZ_RUSSELLRAO:
        v = ((double)n - tt) / (double)n;
        break;
    case KZ_SOKALSNEATH:
        v = (2.0 * df) / (2.0 * df + tt);
        break;
    case KZ_YULE: {
        const double h = (double)(nx - ntt) * (double)(ny - ntt);   // ntf nft
        const double ff = (double)n - tt - df;
        v = (h == 0.0) ? 0.0 : (2.0 * h) / (tt * ff + h);
        break;
    }
    default:   // KZ_ROGERSTANIMOTO, KZ_SOKALMICHENER: the same expression in scipy
        v = (2.0 * df) / ((double)n + df);
        break;
    }
    return v == v ? v : INFINITY;
}

// A matrix searched against ITSELF: scikit-learn's pairwise_distances takes X is Y through pdist + squareform, whose diagonal is 0
// whatever the metric says of a row and itself (russellrao: (n - nx) / n; dice, sokalsneath of an all-false row: NaN) -- as long as
// the whole distance matrix is ONE chunk of its 1 GiB working memory (pairwise_distances_chunked hands the query on unsliced only
// then: floor(2^27 / n_index) >= n_query).  The single-source fit of a hubness reduction and a query that is the fitted array are
// such searches; the reference's results carry that 0, so the device writes it under the same condition.  Beyond one chunk
// scikit-learn slices the query, the pair goes through cdist and has the metric's own value -- here too.
static inline bool kz_bool_self_zero(const kz_matrix* query, const kz_matrix* index) {
    return query == index && ((int64_t)1 << 27) / index->n >= query->n;
}

// kz_matrix_create: the bit image and the row counts of a matrix created for a boolean metric (enqueued on the context's stream)
int kz_bool_image(kz_matrix* m);
void kz_bool_image_free(kz_matrix* m);
// the exact route's distance step: the [nb][n_i] float64 value matrix of the queries fail_list[b0 .. b0 + nb) (kz_exact.h: kz_exact_distances)
void kz_bool_launch_dist(kz_ctx* ctx, const int* fail_list, int b0, int nb, int64_t q_begin, const kz_matrix* query, const kz_matrix* index,
                         double* vals);
// kz_pair_values of the boolean metrics: one lane per pair over the packed rows
void kz_bool_launch_pair_values(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                                const int64_t* d_ind, int k, double* d_val);
