/*
 * kiez_amd.h — C ABI of the MI355X (gfx950) exact-kNN + hubness-reduction hot path.
 *
 * This is the drop-in boundary for the path
 *     kiez.Kiez.fit / kiez.Kiez.kneighbors                      (reference: kiez/kiez.py:160-223)
 *       -> HubnessReduction.fit / kneighbors / _sort            (kiez/hubness_reduction/base.py:33-105)
 *       -> SklearnNN._fit / _kneighbors                         (kiez/neighbors/exact/sklearn_nearest_neighbors.py:83-101)
 *       -> CSLS / MutualProximity / LocalScaling / DisSimLocal  (kiez/hubness_reduction/{csls,mutual_proximity,local_scaling,dis_sim}.py)
 * The reference has no native code (it is pure Python over scikit-learn), so there is no existing FFI to
 * mirror; the entry points below are what a `ctypes` binding inside the reference's plugin classes
 * (`NNAlgorithm._fit/_kneighbors`, `HubnessReduction._fit/transform`) binds.  INTEGRATION.md shows that stub.
 *
 * Conventions
 *   - plain C, `extern "C"`, no C++/torch types; every function returns 0 on success, non-zero on error and
 *     never throws across the boundary; `kz_last_error()` returns a thread-local message for the last failure.
 *   - all `d_*` pointers are DEVICE pointers (HBM) on the context's GPU; `h_*` are host pointers.
 *   - distances are float64, neighbour indices int64 (what the reference returns for the euclidean family,
 *     SURVEY.md §3.4); matrices are row-major [n, d], float32 or float64.
 *   - one kz_ctx per GPU; calls on one context are serialised by the caller (the reference is single-threaded).
 */
#ifndef KIEZ_AMD_H
#define KIEZ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZ_ABI_VERSION 7
/* candidates per query the rescaling / sort kernels take (kz_knn itself returns up to 4096 neighbours) */
#define KZ_MAX_CANDIDATES 4096
/* entries per row kz_merge_topk merges (segments x segment length) */
#define KZ_MERGE_MAX_ENTRIES 8192

/* status codes */
enum { KZ_OK = 0, KZ_ERR_INVALID = 1, KZ_ERR_HIP = 2, KZ_ERR_UNSUPPORTED = 3, KZ_ERR_NOMEM = 4, KZ_ERR_NONFINITE = 5 };
/* element types of an embedding matrix.  KZ_F16 (IEEE binary16) and KZ_BF16 (the upper half of a float32) are STORAGE types: rows of
 * 2 bytes per element, read in place, for the metrics of the fused MFMA kernels (0 .. 2) only.  Such a matrix behaves in every
 * call like the KZ_F64 matrix that holds the same values widened exactly: the same neighbours, the same distance bits, float64
 * outputs, the same errors.  (Additive: the ABI version stays 7.) */
enum { KZ_F32 = 0, KZ_F64 = 1, KZ_F16 = 2, KZ_BF16 = 3 };
/* metrics of the exact backend; minkowski(p=2) == euclidean (sklearn_nearest_neighbors.py:51-65).  0 .. 2 run the fused MFMA
 * kernels; 3 .. 5 (the rest of the Minkowski family: manhattan = cityblock = l1, chebyshev, minkowski with any p >= 1 set by
 * kz_matrix_set_minkowski_p) have no inner-product form: a register-tiled VALU kernel computes scikit-learn's generic
 * DistanceMetric expression (sklearn/metrics/_dist_metrics.pyx.tp: |x_j - y_j| in the input dtype, float64 accumulation in
 * feature order, result rounded to the input dtype), the exact float64 selection kernels pick the neighbours.
 * 6 .. 9 take the same VALU route with scikit-learn's expressions of the other per-feature metrics: braycurtis and seuclidean
 * (DistanceMetric: the difference in the input dtype, float64 sums in feature order, ranking value rounded to the input dtype;
 * seuclidean needs kz_matrix_set_seuclidean_v and returns sqrt of its ranking value), correlation and hamming (scipy's cdist:
 * float64 throughout; correlation = 1 - centred cosine, NaN for a constant row, ranked after every finite value).
 * 10 .. 16 are scipy's boolean metrics (scikit-learn casts the rows to bool, x != 0, and calls cdist): the matrix keeps a
 * bit-packed image of the rows, a popcount kernel counts popcount(x & y) per pair and one float64 division gives scipy's value;
 * dice and sokalsneath are NaN between two all-false rows, ranked after every finite value and returned as NaN.
 * 17 is scikit-learn's metric="precomputed": the caller's distance matrix IS the value matrix -- no distance arithmetic at all, the
 * exact float64 selection kernels pick the neighbours.  Such handles come from kz_matrix_create_precomputed only (kz_matrix_create
 * keeps refusing the id). */
enum { KZ_EUCLIDEAN = 0, KZ_SQEUCLIDEAN = 1, KZ_COSINE = 2, KZ_MANHATTAN = 3, KZ_CHEBYSHEV = 4, KZ_MINKOWSKI = 5,
       KZ_BRAYCURTIS = 6, KZ_SEUCLIDEAN = 7, KZ_CORRELATION = 8, KZ_HAMMING = 9,
       KZ_JACCARD = 10, KZ_DICE = 11, KZ_ROGERSTANIMOTO = 12, KZ_RUSSELLRAO = 13, KZ_SOKALMICHENER = 14, KZ_SOKALSNEATH = 15,
       KZ_YULE = 16, KZ_PRECOMPUTED = 17 };

typedef struct kz_ctx kz_ctx;       /* one GPU + one HIP stream + scratch                                   */
typedef struct kz_matrix kz_matrix; /* an embedding matrix resident in HBM: raw rows, MFMA-packed tiles, norms */

/* Statistics of one kz_knn call (all optional diagnostics; used by bench.py for the roofline line). */
typedef struct kz_knn_stats {
    double main_kernel_ms;   /* HIP-event time of the fused distance+top-k kernel (the dominant kernel)   */
    double finalize_ms;      /* merge + certify + float64 re-rank kernel                                   */
    double fallback_ms;      /* exact float64 brute-force for uncertified rows (0 if none)                 */
    int64_t n_fallback_rows; /* query rows answered by the exact float64 kernels: no approximate tier could certify their
                                candidate set (or, a handful left by a pass, sent there directly: n_spec_rows)         */
    int32_t list_len;        /* K' = per-list candidate count kept by the fused kernel                     */
    int32_t n_splits;        /* index range splits (grid.y)                                                */
    int32_t n_blocks;        /* workgroups launched                                                        */
    int32_t first_pass;      /* operand precision of the fused kernel the call started with: 0 = float32 MFMA,
                                1 = split-bf16 (bf16x2) MFMA, 2 = fp16 MFMA on centred operands               */
    int64_t n_escalated_rows; /* query rows whose candidate set the first pass could not certify and that were
                                searched again one tier down (longer lists -> float32 operands -> exact float64) */
    double max_err_ratio;    /* self-check: max over all re-ranked candidates of |approximate key - exact key| / eps,
                                eps = the rounding bound the certification uses; must stay below 1          */
    int32_t dual;            /* kz_knn_dual: 1 = this direction came out of the shared sweep, 0 = ordinary search */
    int32_t n_first_pass_fail; /* query rows the call's FIRST pass left uncertified, each counted once (n_escalated_rows is
                                cumulative over the levels below: a row that went two levels down counts twice there)  */
    int64_t n_events;        /* kz_knn_dual, reverse direction: events filed for the rows of b                */
    int64_t n_overflow_rows; /* kz_knn_dual, reverse direction: rows of b whose event buffer overflowed (searched again) */
    int64_t n_logged_groups; /* kz_knn_dual, reverse direction: groups of four keys the sweep logged (>= n_events / 4)   */
    int32_t wide_lists;      /* > 0: the call ran the fp16 tier's WIDE route -- that many lists of 16 per query (data whose keys
                                are dense around the k-th neighbour: margin in ranks instead of better operands)           */
    int32_t n_spec_rows;     /* of n_fallback_rows: a handful of rows the first pass left uncertified, answered by the exact kernels
                                launched speculatively behind the finalize kernel (no re-search, no extra synchronisation)        */
    double probe_ms;         /* tier / floor probe of a large search (a strided sample of the query rows searched first), incl. the
                                ladder's second rung; not part of fallback_ms                                                 */
    int64_t n_range_rows;    /* of n_fallback_rows: rows answered by the RANGE re-search -- the exact kernels on the index rows whose
                                approximate key lies within the rounding bound of the row's k-th candidate, not on the whole index */
    int64_t n_range_pairs;   /* (query row, index row) pairs the range re-search evaluated in float64                            */
    int64_t n_range_group_rows; /* of n_range_rows: rows answered as part of a GROUP -- rows of one tight cluster share the range of a
                                representative row: a dense block of pairs instead of one range per row                        */
    int32_t thresh_source;   /* kz_knn_dual: where the shared sweep's event thresholds came from -- 0 no shared sweep, 1 sample sweep,
                                2 nested sample sweep, 3 probe model (no sample sweep)                                           */
    int32_t model_max_events; /* ... probe model: the largest event count the model gives a probe row (0: the reverse probe did not run) */
    double model_mean_events; /* ... probe model: the mean of those counts                                                         */
    double floor_r2;         /* kz_knn_dual: share of the variance of the forward probe's k-th keys the floor's fit explains
                                (0: no floor probe); the model thresholds' pre-gate                                               */
} kz_knn_stats;

/* ---- library / context -------------------------------------------------------------------------------- */
int kz_abi_version(void);
const char* kz_last_error(void);
int kz_device_count(int* n);
/* stream: an existing hipStream_t to run on (e.g. torch's current stream), or NULL for a private stream. */
int kz_ctx_create(int device, void* stream, kz_ctx** out);
int kz_ctx_destroy(kz_ctx* ctx);
int kz_ctx_sync(kz_ctx* ctx);
/* Hands the context's cached device buffers back to the driver (buffers released by kz_free / kz_matrix_destroy / the
 * searches are kept for reuse -- up to 48 GiB -- so that a repeated fit() does not pay hipMalloc + hipFree; a process that
 * shares the GPU with another allocator, e.g. torch's, calls this after a large search).  Waits for the stream. */
int kz_ctx_trim(kz_ctx* ctx);
/* *h_free (host) = the bytes a kz_malloc can still get on the context's device -- what the driver reports free plus the released
 * buffers the context keeps for reuse; *h_total = the device's memory.  What a caller sizes a variable-length result against
 * (kz_radius_neighbors) before it allocates.  Additive, ABI v7. */
int kz_ctx_mem_info(kz_ctx* ctx, size_t* h_free, size_t* h_total);
/* Options (the public contract -- four names):
 *   "precision"    0 (default) = fp16 first pass on centred operands (16 <= d_pad <= 384), rows it cannot certify go down the
 *                  tiers (more / longer lists -> split-bf16 operands -> float32 operands -> exact float64); 2 = split-bf16 first
 *                  pass; 1 = float32 operands only.  The neighbour order is the float64 one either way.
 *   "dual_stride"  kz_knn_dual samples every n-th tile of a for its thresholds: 1 (default) = chosen from the shapes, 0 = always
 *                  two ordinary searches, 2 .. 64 = that stride.
 *   "dual_max_gb"  transient footprint kz_knn_dual may claim, GiB (0 = 32): beyond it, or beyond what is free, it searches twice.
 *   "eps_scale"    multiplies the certification bound (test knob: a huge value sends every row to the exact float64 kernels).
 * Every other name the call accepts is an internal tuning / diagnostic knob of this build (one table: kiez_amd/csrc/kz_options.h),
 * outside this contract.  Options decide how fast a result arrives, never what it is.  Unknown name or value: KZ_ERR_INVALID. */
int kz_ctx_set_option(kz_ctx* ctx, const char* name, double value);

int kz_malloc(kz_ctx* ctx, size_t bytes, void** d_ptr);
int kz_free(kz_ctx* ctx, void* d_ptr);
int kz_memcpy_h2d(kz_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int kz_memcpy_d2h(kz_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int kz_memcpy_d2d(kz_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* ---- index construction: replaces SklearnNN._fit (sklearn_nearest_neighbors.py:83-94) ------------------ */
/* rows [n, d]: rows_on_device = 0 host memory (copied into HBM), 1 device memory (copied), 2 device memory BORROWED
 * (read in place; the caller keeps the buffer alive and unchanged until kz_matrix_destroy), 3 device memory borrowed as a ROW
 * SOURCE only (no norms, no operand images: accepted by kz_dsl_fit as `source`, refused by every search entry point).  Computes the float64 row
 * norms; the MFMA operand images (fp16 / split-bf16 / float32 tiles) are built by the first kz_knn that needs them.
 * NaN/inf input is an error (KZ_ERR_NONFINITE; scikit-learn rejects those inputs too), and so is a row whose squared norm
 * |x|^2 exceeds 1e30 (|x| <= 1e15: the input limit of the float32 operand images and of the rounding bounds built on the row
 * norms; scikit-learn accepts such rows -- same error code, the message names the limit): reported here for host rows, by
 * the first kz_knn / kz_knn_dual that searches the matrix for device rows (this call then waits for nothing).
 * dtype KZ_F16 / KZ_BF16: metrics KZ_EUCLIDEAN, KZ_SQEUCLIDEAN and KZ_COSINE only (every rows_on_device mode); any other metric is
 * KZ_ERR_UNSUPPORTED before anything is allocated. */
int kz_matrix_create(kz_ctx* ctx, const void* rows, int rows_on_device, int64_t n, int64_t d, int dtype,
                     int metric, kz_matrix** out);
/* metric KZ_MINKOWSKI: the exponent p >= 1 (default 2; both matrices of a search must agree). */
int kz_matrix_set_minkowski_p(kz_matrix* m, double p);
/* metric KZ_SEUCLIDEAN: the per-feature variances V[0 .. d) (host memory, copied), every one finite and > 0 -- stricter than
 * scikit-learn, which divides by whatever V holds.  Refused for any other metric.  A search whose two matrices do not hold
 * bit-identical V (or no V) fails with KZ_ERR_INVALID. */
int kz_matrix_set_seuclidean_v(kz_matrix* m, const double* V, int64_t d);
int kz_matrix_destroy(kz_matrix* m);
int kz_matrix_shape(const kz_matrix* m, int64_t* n, int64_t* d, int* dtype, int* metric);

/* ---- a precomputed distance matrix (scikit-learn's metric="precomputed") -- ABI v7, additive ---------------------------------- */
/* values: row-major [n_rows, n_cols], dtype KZ_F32 or KZ_F64: values[i, j] = the distance from "source" row i to "target" row j
 * (a fused similarity of several views turned into a distance, the scores of a matching network, a cdist already in HBM).
 * values_on_device: 0 host memory (copied into HBM), 1 device memory (copied), 2 device memory BORROWED (read in place; the caller
 * keeps the buffer alive and unchanged until BOTH handles are destroyed).  Returns two handles over ONE storage: *rows_view has
 * n = n_rows (its "features" are the n_cols distances of a row), *cols_view has n = n_cols and is the transposed view.  The storage
 * is shared and reference counted: kz_matrix_destroy takes the handles in either order.  Nothing else is allocated or computed:
 * no operand image, no norms, no per-row state.  kz_matrix_shape reports (n, the other extent, dtype, KZ_PRECOMPUTED).
 * Both extents must be >= 1 and below 2^31 - 256 (element offsets are 64-bit: n_rows x n_cols may exceed 2^32).
 * A precomputed handle pairs ONLY with the other view of the same storage: kz_knn / kz_gold_ranks / kz_gold_ranks_reduced /
 * kz_knn_reduced / kz_softmin_rows with query = one view and index = the other answer "rows of D against its columns" or the reverse;
 * the same view on both sides, views of two different matrices, a precomputed handle beside an embedding matrix, and
 * exclude_self != 0 (the data is two-sided: a caller masks a diagonal themselves) are KZ_ERR_INVALID.  The value of a pair IS its
 * matrix entry, widened to float64: kz_knn orders by (value, index row) and returns the values as they are (the exact float64
 * selection kernels, any k <= min(index.n, 4096)); the whole-index calls reduce them as they reduce any distance.
 * Every value must be finite and >= 0 (-0.0 is fine): NaN or an infinity is KZ_ERR_NONFINITE, a negative value KZ_ERR_INVALID
 * ("Negative values in data passed to precomputed distance matrix", scikit-learn's words) -- scikit-learn raises ValueError for
 * both, and the selection kernels assume it.  Host values: the verdict comes from this call; device values: from the first of the
 * calls above on the pair (this call then waits for nothing).
 * kz_knn_dual, kz_pair_values, kz_dsl_fit, kz_dsl_transform, kz_matrix_set_minkowski_p and kz_matrix_set_seuclidean_v refuse a
 * precomputed handle with KZ_ERR_INVALID before anything is launched. */
int kz_matrix_create_precomputed(kz_ctx* ctx, const void* values, int values_on_device, int64_t n_rows, int64_t n_cols, int dtype,
                                 kz_matrix** rows_view, kz_matrix** cols_view);

/* ---- exact kNN: replaces SklearnNN._kneighbors (sklearn_nearest_neighbors.py:96-101) -------------------- */
/* For query rows [q_begin, q_begin+q_count) of `query` find the k nearest rows of `index`, ascending.
 * exclude_self != 0: query row r is index row r and is removed the way sklearn does for X=None
 * (sklearn/neighbors/_base.py:828-834, 937-965).  d_dist: [q_count, k] float64, d_ind: [q_count, k] int64.
 * Indices follow the float64 distance order (ties by smaller index); distances follow sklearn's dtype rule
 * (float32 inputs + euclidean: (double)sqrtf((float)d2)). */
int kz_knn(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
           int k, int exclude_self, double* d_dist, int64_t* d_ind, kz_knn_stats* stats);

/* Both directions between two matrices from ONE sweep of the distance matrix: what HubnessReduction.fit (target ->
 * source neighbours, kiez/hubness_reduction/base.py:48-58) and .kneighbors (source -> target, base.py:95-112) compute
 * with two brute-force searches.  d_dist_ab / d_ind_ab: [a.n, k] = for every row of a its k nearest rows of b;
 * d_dist_ba / d_ind_ba: [b.n, k] the reverse.  Results are identical to kz_knn(a, b) and kz_knn(b, a) (same float64
 * order, same tie rule); pass the LARGER matrix as a (fewer rows get event buffers).  Falls back to two ordinary
 * searches where the shared sweep does not apply (precision != 0, tiny inputs, k > 110).  stats_* may be NULL. */
int kz_knn_dual(kz_ctx* ctx, const kz_matrix* a, const kz_matrix* b, int k, double* d_dist_ab, int64_t* d_ind_ab,
                double* d_dist_ba, int64_t* d_ind_ba, kz_knn_stats* stats_ab, kz_knn_stats* stats_ba);

/* Host-only (no GPU needed): the work schedule kz_knn builds for a launch with `slots` resident workgroups
 * (DESIGN.md section 3.0 "host schedule": greedy rounds).  Round r covers round_qtiles[r] query tiles of 128 rows, each swept as
 * round_pieces[r] index ranges of round_piece_tiles[r] tiles of 128 rows (the last range may be shorter).  Arrays
 * hold up to 8 rounds.  k_eff = neighbours kept per query (k + 1 in single-source mode).
 * Diagnostic ABI: it plans the CLASSIC route -- one candidate list of K' in {16, 32, 64, 128} per query and index range, one
 * query tile per workgroup, k_eff <= 110 -- through the same kz_plan_rounds the product calls.  kz_knn itself also takes
 * routes this function does not describe: several lists of 16 over forced index ranges (13 <= k on a large index, the shared
 * sweep's forward lists, re-searches), the long-k route (111 .. ~540 neighbours) and work items of two or three query tiles
 * (wide and 64-query builds); their plans come out of the same kz_plan_pass with other arguments (tests/host/plan_sanitize.cpp
 * runs those argument ranges under the sanitizers). */
int kz_knn_plan(int64_t n_query_rows, int64_t n_index_rows, int k_eff, int slots, int force_splits, int min_splits,
                int* n_rounds, int* round_qtiles, int* round_pieces, int* round_piece_tiles);

/* ---- per-row statistics of a [n, K] distance array (numpy summation order) ----------------------------- */
/* mean: ndarray.mean(axis=1) (a NaN in the row gives NaN, as CSLS and NICDM have it); std: np.nanstd(axis=1) (ddof=0: NaN
 * entries are skipped, a row of NaN only gives NaN); last: column K-1.  Any output may be NULL.
 * Used for the fit state of CSLS (csls.py:90), NICDM (local_scaling.py:143), LS (:136). */
int kz_row_stats(kz_ctx* ctx, const double* d_dist, int64_t n, int K, double* d_mean, double* d_std, double* d_last);
/* mean: np.nanmean(axis=1); std: np.nanstd(axis=1) (ddof=0).  NaN entries (correlation against a constant row, dice /
 * sokalsneath between all-false rows) count as 0 in numpy's summation tree over the whole row and the sums are divided by the
 * number of entries that are not NaN; a row of NaN only gives NaN.  Either output may be NULL.  The fit state of MP normal
 * (mutual_proximity.py:102-103); kz_mp_normal computes the query side (:177-178) the same way. */
int kz_row_nanstats(kz_ctx* ctx, const double* d_dist, int64_t n, int K, double* d_mean, double* d_std);

/* ---- hubness rescaling: replace HubnessReduction.transform of each method ------------------------------ */
/* All take the forward candidates d_dist/d_ind [n, K] and write the UNSORTED rescaled distances d_out [n, K]. */
/* CSLS.transform, csls.py:85-96.  r_train[j] = mean_K dist_t2s[j,:] (length n_t). */
int kz_csls(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, const double* d_r_train,
            double* d_out);
/* Sinkhorn / inverted softmax (no counterpart in the reference) -- ABI v7, additive: d_out[i, c] = (d_dist[i, c] - d_f[i]) -
 * d_g[d_ind[i, c]], two float64 subtractions in that order: the candidate-list form of KZ_RANK_DUAL below, bit for bit what
 * kz_gold_ranks_reduced / kz_knn_reduced compute for the pair.  d_f: [n], d_g: [n_t], the potentials (kz_softmin_rows).  d_ind is
 * trusted as in kz_csls: every entry must be a row of d_g. */
int kz_dual_shift(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, const double* d_f,
                  const double* d_g, double* d_out);
/* LocalScaling.transform, local_scaling.py:129-151.  nicdm == 0: r_t = K-th reverse distance (:135-140);
 * nicdm != 0: r_t = mean reverse distance (:142-147). */
int kz_local_scaling(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, const double* d_r_t,
                     int nicdm, double* d_out);
/* MutualProximity 'normal', mutual_proximity.py:166-183. */
int kz_mp_normal(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, const double* d_mu_t,
                 const double* d_sd_t, double* d_out);
/* MutualProximity 'empiric', mutual_proximity.py:185-212 (target ids are looked up in the reverse lists of
 * source ids, as the reference does). */
int kz_mp_empiric(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K,
                  const double* d_dist_t2s, const int64_t* d_ind_t2s, int64_t n_t, int Kt, double* d_out);
/* DisSimLocal._fit, dis_sim.py:96-107: t2c[j] = |target[t_begin+j] - mean_K source[ind_t2s[j,:]]|^2 for
 * n_rows reverse-list rows. */
int kz_dsl_fit(kz_ctx* ctx, const int64_t* d_ind_t2s, int64_t n_rows, int Kt, const kz_matrix* source,
               const kz_matrix* target, int64_t t_begin, double* d_t2c);
/* DisSimLocal.transform, dis_sim.py:139-166 (before the global shift): writes d_out and the running
 * minimum into *d_min (caller initialises *d_min to +inf; multi-GPU callers all-reduce it with MIN). */
int kz_dsl_transform(kz_ctx* ctx, const int64_t* d_ind, int64_t n, int K, const kz_matrix* query, int64_t q_begin,
                     const kz_matrix* target, const double* d_t2c, double* d_out, double* d_min);
/* dis_sim.py:171-177: shift by -min if min < 0, then sqrt unless squared. */
int kz_dsl_finalize(kz_ctx* ctx, double* d_out, int64_t count, double min_value, int squared);

/* ---- final candidate sort: replaces HubnessReduction._sort (base.py:72-87, numpy branch) ---------------- */
/* Selection sort with swaps of the first k positions == np.argpartition(kth=arange(k)) + take_along_axis
 * (SURVEY.md §8 a-6).  d_odist/d_oind: [n, k]. */
int kz_select_topk(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, int k,
                   double* d_odist, int64_t* d_oind);

/* ---- the tail of kneighbors in one launch: rescale + final sort + output cast -- ABI v7, additive ------------------------------ */
/* The hubness kinds of kz_rescale_select and kz_fit.  1 .. 4 share the numbering of KZ_RANK_* below (the pointwise reductions);
 * KZ_HUB_NONE leaves the distances as they are, KZ_HUB_MP_EMPIRIC is a kind of kz_fit only. */
enum { KZ_HUB_NONE = 0, KZ_HUB_CSLS = 1, KZ_HUB_LS = 2, KZ_HUB_NICDM = 3, KZ_HUB_MP_NORMAL = 4, KZ_HUB_MP_EMPIRIC = 5 };
/* For the forward candidates d_dist / d_ind [n, K]: per row the query-side statistic (CSLS, NICDM: ndarray.mean in numpy's pairwise
 * order; LS: the last entry; MP normal: np.nanmean / np.nanstd), w of every candidate (kind KZ_HUB_NONE: w = d), the selection of
 * kz_select_topk (first minimum wins, swap history kept, NaN last) and the store of the first k values and ids -- bit for bit what
 * kz_csls / kz_local_scaling / kz_mp_normal -> kz_select_topk -> kz_cast_f64_f32 give, NaN payloads included, without the two [n, K]
 * intermediates.  d_t_a / d_t_b: the index-side state vectors as those calls take them (CSLS r_train; LS / NICDM r_t; MP normal
 * mu_t and sd_t; d_t_b is read by MP normal only, neither by KZ_HUB_NONE).  out_dtype KZ_F64 or KZ_F32: the type of d_odist [n, k]; for
 * KZ_F32 the cast comes LAST, after the selection.  d_oind: [n, k].  K <= 128 runs ONE kernel (64 rows per wave on a transposed image
 * in LDS); beyond that the call runs the kernels named above in sequence on transient buffers itself: same result.
 * k outside [1, K], an unknown kind (KZ_HUB_MP_EMPIRIC included: kz_mp_empiric reads the reverse lists), another out_dtype or a NULL
 * state the kind reads: KZ_ERR_INVALID before anything is written.  d_ind is trusted as in kz_csls. */
int kz_rescale_select(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K, int k, int kind,
                      const double* d_t_a, const double* d_t_b, int out_dtype, void* d_odist, int64_t* d_oind);

/* ---- one call per fit and per kneighbors: HubnessReduction.fit / .kneighbors (base.py:33-50, 89-105) -- ABI v7, additive -------- */
/* kz_fit decides which searches serve the two directions, runs those that belong to the fit and computes the fit state of the
 * reduction; kz_kneighbors runs the forward search where the fit did not, the rescaling, the final sort and the output cast, and
 * writes into the caller's buffers.  The decisions are a pure host function (kiez_amd/csrc/kz_fit_plan.h):
 *   two-sided, shared_sweep != 0   kz_knn_dual with the larger matrix first (it searches twice by itself where no sweep applies)
 *   shared_sweep == 0              the reverse kz_knn only (target rows against the source, nothing stripped); the forward search
 *                                  runs at the first kz_kneighbors
 *   single source (target NULL), shared_sweep != 0, n_candidates + 1 <= min(n, 110)
 *                                  ONE kz_knn(source, source, n_candidates + 1, exclude_self = 0) + kz_split_self
 *   any other single-source fit    the reverse search without stripping; the forward search (exclude_self = 1) at the first kz_kneighbors
 *   KZ_HUB_NONE                    no search at all: kz_kneighbors is one kz_knn for k neighbours (exclude_self for single source)
 * Refused before any launch: a reduction with n_candidates < 2, n_candidates above min(n_source, n_target) (above n - 1 for single
 * source: clamping with a warning is the caller's business) and matrices that disagree in context, feature count, element type or
 * metric: KZ_ERR_INVALID; n_candidates > 4095 and a precomputed matrix: KZ_ERR_UNSUPPORTED.
 * The fitted object BORROWS the two matrices (the caller keeps them alive until kz_fitted_destroy) and OWNS the reverse lists, the
 * fit state and -- once they exist, until kz_fitted_destroy -- the forward lists (16 n_source n_candidates bytes): a second
 * kz_kneighbors with another k runs no search (KZ_HUB_NONE searches for k neighbours each time).
 * Not here: ad-hoc query rows, the target -> source direction, DisSimLocal and the dual-potential reductions. */
typedef struct kz_fitted kz_fitted;
typedef struct kz_fit_info {
    int64_t n_source, n_target;  /* n_target = n_source for single source */
    int32_t n_candidates, hubness, single_source, shared_sweep;
    int32_t search;              /* the plan that ran: 0 none, 1 kz_knn_dual, 2 reverse search only, 3 single-source split */
    int32_t larger_first;        /* search 1: 1 = the source was kz_knn_dual's first matrix, 0 = the target */
    int32_t tail;                /* 0 kz_knn, 1 kz_rescale_select, 2 kz_mp_empiric + kz_select_topk + cast */
    int32_t fused;               /* tail 1: 1 = the fused kernel serves n_candidates, 0 = the kernel sequence */
    int32_t forward_ready;       /* the forward lists exist */
    int32_t n_searches;          /* search calls (kz_knn / kz_knn_dual) made for this object so far */
    kz_knn_stats stats_forward;  /* of the source -> target search (the one search of a single-source split); zero before it ran */
    kz_knn_stats stats_reverse;  /* of the target -> source search; zero where none ran (split, KZ_HUB_NONE) */
} kz_fit_info;
/* hubness: KZ_HUB_*; n_candidates: K; target NULL: single source.  *out: the fitted object. */
int kz_fit(kz_ctx* ctx, const kz_matrix* source, const kz_matrix* target, int hubness, int n_candidates, int shared_sweep,
           kz_fitted** out);
/* 1 <= k <= n_candidates; out_dtype KZ_F64 / KZ_F32: the type of d_dist [n_source, k] (the cast comes last); d_ind: [n_source, k]. */
int kz_kneighbors(kz_fitted* f, int k, int out_dtype, void* d_dist, int64_t* d_ind);
int kz_fitted_info(const kz_fitted* f, kz_fit_info* out);
/* Borrowed device pointers into the fitted object, valid until kz_fitted_destroy: *d_ptr (NULL where the object holds no such array:
 * the forward lists before they exist, a state the kind does not have), *rows and *cols (1 for a state vector). */
enum { KZ_FIT_REVERSE_DIST = 0, KZ_FIT_REVERSE_IND = 1, KZ_FIT_FORWARD_DIST = 2, KZ_FIT_FORWARD_IND = 3, KZ_FIT_STATE_A = 4,
       KZ_FIT_STATE_B = 5 };
int kz_fitted_state(const kz_fitted* f, int what, const void** d_ptr, int64_t* rows, int* cols);
/* Releases what the object owns (stream-ordered, as kz_free); NULL is fine. */
int kz_fitted_destroy(kz_fitted* f);

/* ---- multi-GPU exchange step (source row-sharded, SURVEY.md section 8e "alternative": per-shard partial top-K + merge) ----- */
/* The reverse search of HubnessReduction.fit (every target row against ALL source rows, base.py:37-42) over a row-sharded
 * source is the merge of the per-shard searches.  kz_knn orders neighbours by the exact float64 value (squared euclidean /
 * cosine distance), ties by smaller row, but RETURNS rounded distances (float32 + euclidean: (double)sqrtf((float)d2)), so
 * per-shard lists are merged by the exact values:
 * kz_pair_values: d_val[r, c] = the value kz_knn ranks index row d_ind[r, c] by for query row q_begin + r -- bit-identical to
 * what the search computed (one canonical dot product); entries with d_ind outside [0, index.n) get +inf. */
int kz_pair_values(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                   const int64_t* d_ind, int k, double* d_val);
/* kz_merge_topk: every row of d_key / d_ind / d_dist [n, segs * seg_len] holds `segs` segments (columns [s seg_len,
 * (s + 1) seg_len)), each sorted ascending by (key, ind) -- one per shard, ind = GLOBAL row ids.  Writes the k smallest
 * entries by (key, ind) in that order: d_odist[n, k] = their d_dist (or their key when d_dist is NULL), d_oind[n, k] = their ind
 * (0 when d_ind is NULL: kinds that only need the merged distances).  segs * seg_len <= KZ_MERGE_MAX_ENTRIES. */
int kz_merge_topk(kz_ctx* ctx, const double* d_key, const int64_t* d_ind, const double* d_dist, int64_t n, int segs, int seg_len,
                  int k, double* d_odist, int64_t* d_oind);

/* ---- multi-GPU: the collectives of the sharded path (kz_comm.hip), over RCCL -- ABI v6 ------------------------------------------
 * One process per GPU.  What the reference's only multi-device call hands to a library (kiez/neighbors/approximate/faiss.py:138,
 * faiss.index_cpu_to_all_gpus) a host in ANY language binds here, without torch: rank 0 draws a 128-byte id (kz_comm_unique_id)
 * and distributes it by whatever the host has (MPI, a file, a socket); every rank calls kz_comm_create with its context.  The
 * collectives are enqueued on the context's stream -- ordered with its kernels, no host synchronisation.  librccl.so is loaded by
 * the first of these calls (dlopen; a copy the process already holds is taken first) and is not a link-time dependency: without
 * RCCL they return KZ_ERR_UNSUPPORTED.  Buffers are device pointers, sizes are bytes.
 *   kz_comm_broadcast           d_buf of rank `root` to every rank, in place                  (the replicated target)
 *   kz_comm_all_gather          d_recv [world][bytes_per_rank] = every rank's d_send          (fit state, shard sizes, source shards)
 *   kz_comm_all_to_all          block r of d_send (send_offset[r], send_bytes[r]) to rank r; d_recv [world][recv_bytes] = the blocks
 *                               received, in rank order                                       (per-shard reverse lists -> kz_merge_topk)
 *   kz_comm_all_reduce_min_f64  element-wise minimum over the ranks, in place                 (DisSimLocal's global shift) */
#define KZ_COMM_ID_BYTES 128
typedef struct kz_comm kz_comm;
int kz_comm_unique_id(void* id128);
int kz_comm_create(kz_ctx* ctx, const void* id128, int rank, int world, kz_comm** out);
int kz_comm_destroy(kz_comm* comm);
int kz_comm_rank(const kz_comm* comm, int* rank, int* world);
int kz_comm_broadcast(kz_comm* comm, void* d_buf, size_t bytes, int root);
int kz_comm_all_gather(kz_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);
int kz_comm_all_to_all(kz_comm* comm, const void* d_send, const size_t* send_offset, const size_t* send_bytes, void* d_recv,
                       size_t recv_bytes);
int kz_comm_all_reduce_min_f64(kz_comm* comm, double* d_buf, size_t count);

/* Single-source mode (fit(source) only): d_dist / d_ind = [n, K1] result of ONE kz_knn of the matrix against itself for
 * K1 = K + 1 neighbours WITHOUT exclude_self, rows row0 .. row0 + n.  Writes both views the reference computes with two
 * searches: rev = the first K columns (HubnessReduction.fit's reverse pass keeps each row as its own first neighbour,
 * base.py:37-42) and fwd = the row minus itself, removed as sklearn does (neighbors/_base.py:937-965) = kz_knn(..., K,
 * exclude_self = 1).  All four outputs are [n, K]. */
int kz_split_self(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n, int K1, int64_t row0,
                  double* d_rev_dist, int64_t* d_rev_ind, double* d_fwd_dist, int64_t* d_fwd_ind);

/* ---- "next" row (f-1): kiez.analysis.hubness_score on the neighbour index matrix (kiez/analysis/estimation.py:197-351) */
/* min / max of an int64 device array (validation + bincount length). */
int kz_minmax_i64(kz_ctx* ctx, const int64_t* d_in, int64_t count, int64_t* h_min, int64_t* h_max);
/* the same over the first k columns of a row-major [rows, cols] matrix: the reference slices nn_ind[:, :k] BEFORE
 * np.bincount(minlength=n_train) (estimation.py:276-292), so ids in the dropped columns must not size the histogram. */
int kz_minmax_i64_2d(kz_ctx* ctx, const int64_t* d_in, int64_t rows, int cols, int k, int64_t* h_min, int64_t* h_max);
/* k-occurrence: np.bincount(nn_ind[:, :k].ravel(), minlength=n_bins) with negative ids dropped (estimation.py:283-292).
 * d_ind: [n_rows, cols] int64; d_kocc: [n_bins] int64. */
int kz_k_occurrence(kz_ctx* ctx, const int64_t* d_ind, int64_t n_rows, int cols, int k, int64_t n_bins, int64_t* d_kocc);
/* Reductions of the k-occurrence vector for skewness, Robin Hood, Atkinson, hub/antihub statistics and (optionally, O(n^2))
 * the Gini numerator.  h_out[10] (host): sum, sum|x-mean|, sum(x-mean)^2, sum(x-mean)^3, sum sqrt(x), max, #zeros,
 * sum over hubs (x >= hub_threshold), #hubs, gini numerator. */
int kz_kocc_stats(kz_ctx* ctx, const int64_t* d_kocc, int64_t n, double hub_threshold, int with_gini, double* h_out);
/* np.argwhere(kocc == 0) (mode 0) / np.argwhere(kocc >= thr) (mode 1), ascending; d_out must hold n entries. */
int kz_kocc_select(kz_ctx* ctx, const int64_t* d_kocc, int64_t n, int mode, double thr, int64_t* d_out, int64_t* h_count);

/* "next" row (f-2): kiez.evaluate.hits (kiez/evaluate/eval_metrics.py:23-61).  d_gold[i] = gold target of source row i or
 * INT64_MIN when the row has no gold entry; d_hist[c] (c < cols) = rows whose gold id sits at position c, d_hist[cols] =
 * rows whose gold id is absent.  hits@k = sum(d_hist[:k]) / len(gold). */
int kz_hit_positions(kz_ctx* ctx, const int64_t* d_ind, const int64_t* d_gold, int64_t n, int cols, int64_t* d_hist);

/* Exact ranks of gold targets against the WHOLE index: mean rank, mean reciprocal rank and hits@k beyond any neighbour list (a list
 * ends at 4096 neighbours).  d_gold[r] = the index row that is the gold answer of query row q_begin + r, INT64_MIN = no gold row
 * (kz_hit_positions' convention); d_gold and d_rank: [q_count] on the device.
 * d_rank[r] = the number of index rows kz_knn orders BEFORE the gold row -- by the exact float64 ranking value ascending, ties by
 * smaller index row, NaN values (correlation against a constant row, dice / sokalsneath between all-false rows) ranked as +inf by
 * row, as the selection kernels have it -- i.e. the 0-based position of the gold row in kz_knn(query, index, k = index.n,
 * exclude_self = 0), for any index.n; d_rank[r] = -1 where d_gold[r] is INT64_MIN or outside [0, index.n).
 * The matrices must agree as for a search (dtype, metric, exponent, seuclidean V: KZ_ERR_INVALID otherwise).  No self-exclusion:
 * the call is for two-sided data.  Runs the exact float64 value kernels of kz_knn for the rows that have a gold id (every metric)
 * and a counting kernel in place of the selection; rows without gold cost no distance work.  Synchronises the context's stream. */
int kz_gold_ranks(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                  const int64_t* d_gold, int64_t* d_rank);
/* The same ranks under a POINTWISE hubness reduction -- ABI v7, additive: CSLS, LocalScaling 'standard', NICDM and MutualProximity
 * 'normal' rescale a pair's distance d with one state of the query row and one of the index row (two each for MP), so the reduced
 * distance w exists for EVERY index row, not for the K candidates alone.  d_rank[r] = #{ j : w_j < w_g or (w_j == w_g and j < g) }
 * with g = d_gold[r], d = the distance kz_knn returns for the pair (the exact ranking value converted as kz_knn converts it) and
 *   KZ_RANK_CSLS       w = 2 d - q_a[r] - t_a[j]                              (the means of the K forward / reverse distances)
 *   KZ_RANK_LS         w = 1 - exp(-d^2 / (q_a[r] t_a[j]))                    (the K-th forward / reverse distance)
 *   KZ_RANK_NICDM      w = d / sqrt(q_a[r] t_a[j])                            (the means)
 *   KZ_RANK_MP_NORMAL  w = 1 - sf(d; q_a[r], q_b[r]) sf(d; t_a[j], t_b[j])    (nanmean and nanstd; sf: the normal survival function)
 *   KZ_RANK_DUAL       w = (d - q_a[r]) - t_a[j]                              (the dual potentials f, g of Sinkhorn / the inverted
 *                                                                              softmax: kz_softmin_rows; kz_dual_shift's expression)
 * in float64, the expressions of kz_csls / kz_local_scaling / kz_mp_normal: w of a pair is bit for bit what those write for it, so
 * with lists over the whole index (K = index.n) the rank is the count over the transform's output row by (value, index row).  A NaN w
 * ranks as +inf by row.  MP normal is exactly 1.0 for pairs far beyond both lists: they tie and go by row.
 * d_q_a / d_q_b: [q_count] on the device, entry r for query row q_begin + r (kz_row_stats / kz_row_nanstats of the forward lists);
 * d_t_a / d_t_b: [index.n] (the same of the reverse lists: the fit state).  d_q_b and d_t_b are for KZ_RANK_MP_NORMAL and must be
 * NULL otherwise (KZ_RANK_DUAL too: one potential per side); an unknown kind, a missing or a surplus vector: KZ_ERR_INVALID.  Everything else as kz_gold_ranks. */
#define KZ_RANK_CSLS 1
#define KZ_RANK_LS 2
#define KZ_RANK_NICDM 3
#define KZ_RANK_MP_NORMAL 4
#define KZ_RANK_DUAL 8 /* (not 5: 5 .. 7 and 0 stay unknown kinds) */
int kz_gold_ranks_reduced(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                          const int64_t* d_gold, int kind, const double* d_q_a, const double* d_q_b,
                          const double* d_t_a, const double* d_t_b, int64_t* d_rank);
/* The list those ranks are positions in -- ABI v7, additive: the k nearest index rows of every query row by the REDUCED distance w
 * over the WHOLE index, not over a candidate list (kz_csls / kz_local_scaling / kz_mp_normal rescale K candidates; an index row
 * outside them can have a smaller w).  Row r of d_w / d_ind ([q_count, k] on the device) holds the k index rows with the smallest w
 * to query row q_begin + r and their w, ascending by (w, index row).  kind, the four state vectors, d and the expression for w are
 * kz_gold_ranks_reduced's: w of a pair has the bits kz_csls / kz_local_scaling / kz_mp_normal write for it.  The order is that
 * call's: a NaN w ranks as +inf and ties with it by index row (and is RETURNED as NaN), -inf is an ordinary smallest value, -0.0
 * equals +0.0.  So for every r and c < k, kz_gold_ranks_reduced with d_gold[r] = d_ind[r, c] and the same inputs gives rank c.
 * k < 1 or k > index.n: KZ_ERR_INVALID; k > KZ_KNN_REDUCED_MAX_K: KZ_ERR_UNSUPPORTED -- beyond it kz_gold_ranks_reduced is the
 * tool: it ranks any row against the whole index without a list.  An unknown kind, a missing or a surplus vector, matrices that
 * disagree (dtype, metric, exponent, seuclidean V): KZ_ERR_INVALID, as kz_gold_ranks_reduced.  No self-exclusion: the call is for
 * two-sided data.  Runs the exact float64 value kernels of kz_knn for every query row and a two-level selection on integer keys;
 * the result does not depend on the order anything runs in.  Synchronises the context's stream. */
#define KZ_KNN_REDUCED_MAX_K 512
int kz_knn_reduced(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                   int k, int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a, const double* d_t_b,
                   double* d_w, int64_t* d_ind);
/* RADIUS NEIGHBOURS over the whole index -- ABI v7, additive: every pair within a threshold, as a CSR.  Pair (r, j) of query row
 * q_begin + r and index row j is in the result exactly when w_rj <= radius, where w is what the list calls return for the pair:
 * kz_radius_neighbors: the distance kz_knn returns (the exact float64 ranking value converted as kz_knn converts it);
 * kz_radius_neighbors_reduced: the hubness-reduced distance of kz_gold_ranks_reduced / kz_knn_reduced (kind, the four state vectors
 * and their validation as there) -- the same expressions and therefore the same bits.  A NaN w is never in the result, not even
 * for radius = +inf.  radius NaN: KZ_ERR_INVALID; +-inf and negative radii are legal (CSLS values are routinely negative).
 * d_indptr: [q_count + 1] int64 on the device: d_indptr[0] = 0, d_indptr[r + 1] - d_indptr[r] = the count of row q_begin + r;
 * *h_total (host) = the number of pairs.  Both are ALWAYS complete and exact, whatever `capacity` is; capacity = 0 is the count-only
 * call (d_ind / d_dist may be NULL).  d_ind / d_dist: [capacity] int64 / float64 on the device: the entries (index row, w) of every
 * row whose end offset d_indptr[r + 1] is <= capacity, at d_indptr[r] ..; for any other row NOTHING is written, and the call
 * returns KZ_OK all the same: the caller compares *h_total with capacity and calls again with an exact allocation.
 * sorted == 0: a row's entries ascend by index row.  sorted != 0: they ascend by (w, index row) in the order of kz_knn_reduced
 * (-0.0 equals +0.0; w is NaN-free by construction), a row of any length -- a row can hold the whole index; rows beyond 4096
 * entries are sorted through a transient second copy of the output in device memory (KZ_ERR_NOMEM when it does not fit).
 * Runs the exact float64 value kernels of kz_knn for every query row and, per batch of them, a count, an integer scan and a fill
 * (the predicate again; places from integer prefix sums): no atomics on the output, nothing depends on the order anything runs
 * in, and the result has the same bits however the call is cut into batches or row ranges (d_indptr relative to the range).
 * Matrices that disagree (dtype, metric, exponent, seuclidean V), a negative capacity: KZ_ERR_INVALID.  No self-exclusion: the call
 * is for two-sided data.  Synchronises the context's stream. */
int kz_radius_neighbors(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                        double radius, int sorted, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                        int64_t* h_total);
int kz_radius_neighbors_reduced(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                                double radius, int sorted, int64_t capacity, int kind, const double* d_q_a, const double* d_q_b,
                                const double* d_t_a, const double* d_t_b, int64_t* d_indptr, int64_t* d_ind, double* d_dist,
                                int64_t* h_total);
/* Row-wise SOFT-MIN over the whole index -- ABI v7, additive: the primitive of the Sinkhorn potentials and the inverted softmax.
 *   d_out[r] = softmin_eps over every index row j of (d_rj - d_off[j])  +  shift,   softmin_eps(x) = m - eps log sum exp(-(x - m) / eps),
 * m = min x, in float64; d_rj = the distance kz_knn returns for query row q_begin + r and index row j (the exact ranking value
 * converted as kz_knn converts it: what KZ_RANK_* reduce).  d_off: [index.n] on the device or NULL (no offset); d_out: [q_count] on
 * the device.  eps > 0 is the temperature, in the units of d.  A Sinkhorn row step is this call with d_off = g; the column step is
 * the same call with target as query, source as index, d_off = f and shift = eps log(n_s / n_t).
 * A NaN entry (a NaN distance, a NaN offset) counts as +inf and contributes nothing; a row with no entry below +inf gives +inf + shift,
 * a row whose minimum is -inf gives -inf.  The minimum is taken out before the sum: no term overflows, and the sum is >= 1 however
 * small eps is.  The order in which a row's terms are added is a function of j, index.n and KZ_SOFTMIN_CHUNK_ROWS only (no atomics,
 * fixed trees): a row's result has the same bits wherever it stands in the call, however the call is split into row ranges, and
 * from run to run.  eps not finite or <= 0, a shift that is not finite, matrices that disagree (dtype, metric, exponent, seuclidean V): KZ_ERR_INVALID;
 * q_count == 0: KZ_OK.  No self-exclusion.  Runs the exact float64 value kernels of kz_knn for every query row and a two-level
 * reduction; synchronises the context's stream. */
#define KZ_SOFTMIN_CHUNK_ROWS 4096 /* index rows per first-level workgroup: part of the summation order */
int kz_softmin_rows(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index, double eps,
                    const double* d_off, double shift, double* d_out);
/* *h_out (host) = max over i < n of |d_a[i] - d_b[i]| (float64 vectors on the device), entries whose difference is NaN ignored (0 when
 * none is left, n == 0 included): a maximum, so the result does not depend on the order anything runs in.  The convergence read-out
 * of the Sinkhorn iteration.  Synchronises the context's stream. */
int kz_max_abs_diff(kz_ctx* ctx, const double* d_a, const double* d_b, int64_t n, double* h_out);
/* ---- the same potentials on the CANDIDATE LISTS (kz_softmin_lists.hip) -- additive, ABI v7 ------------------------------------- */
/* kz_softmin_rows evaluates every pair of the two sides in every step.  These four calls restrict the transport plan to the pairs of
 * neighbour lists d_dist / d_ind [n_q, k] (float64 / int64, on the device): entry (i, c) is a PAIR of source row i and target row
 * d_ind[i, c] when 0 <= d_ind[i, c] < n_index, kz_match_lists' rule; any other id (-1, kz_knn_reduced's INT_MAX padding, an id >=
 * n_index) is no pair.  A pair outside a row's list would carry exp(-(d - m) / eps) of mass; it is DROPPED, so the potentials depend
 * on k.  1 <= k <= KZ_MAX_CANDIDATES, 1 <= n_index <= 2^31 - 2, n_q k <= 2^31 - 2, eps finite and > 0, shift finite, no null
 * pointer: KZ_ERR_INVALID otherwise.  A NaN value (a NaN distance, a NaN offset) counts as +inf; a set with no entry below +inf
 * gives +inf + shift, one with a -inf gives -inf, all as kz_softmin_rows.  New: a row or a column with NO PAIR AT ALL gives NaN,
 * "no value" -- a target row nobody lists has no potential, and under KZ_RANK_DUAL its w is NaN and ranks last, by row.
 *
 * kz_lists_transpose: the column-major view of the pairs.  d_colptr [n_index + 1] (int64), d_col_row [n_q k] (int32: the source row)
 * and d_col_val [n_q k] (float64: the pair's d_dist); the entries of column j are the places d_colptr[j] .. d_colptr[j + 1] - 1, in
 * ascending flat position i k + c (ascending source row); d_colptr[n_index] = nnz, the places behind it are not written.  *h_nnz
 * (host, may be NULL: then nothing is read back and the call does not synchronise) = nnz.  A stable sort places the entries, no
 * atomic does: the arrays are the same in every run.  n_q == 0: all of d_colptr is 0. */
int kz_lists_transpose(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                       int64_t* d_colptr, int32_t* d_col_row, double* d_col_val, int64_t* h_nnz);
/* d_out[i] = softmin_eps over the pairs c of row i of (d_dist[i, c] - d_off[d_ind[i, c]])  +  shift; d_off: [n_index] or NULL,
 * d_out: [n_q].  The order a row's terms are added in is a fixed tree that depends on k only (k <= 64: the next power of two >= k
 * lanes hold a row; k > 64: one wave per row): the same bits whichever other rows are in the call, and from run to run.
 * n_q == 0: KZ_OK.  Synchronises the context's stream. */
int kz_softmin_list_rows(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, double eps,
                         const double* d_off, double shift, double* d_out);
/* d_out[j] = softmin_eps over the entries p of column j of (d_col_val[p] - d_off[d_col_row[p]])  +  shift, on the view
 * kz_lists_transpose wrote; nnz: what it returned (or the capacity n_q k of the arrays); d_off: [n_q] or NULL, d_out: [n_index].
 * A column is cut into chunks of KZ_SOFTMIN_LIST_CHUNK entries counted from its own first entry; one wave reduces a chunk to
 * (minimum, sum), the parts of a column of more than one chunk are folded by one wave, lane l taking the chunks l, l + 64, ...
 * in ascending order.  The tree is a function of the column's entry count and KZ_SOFTMIN_LIST_CHUNK only (no float atomics): the
 * same bits wherever the column lies in the view, whatever other columns and rows are in the call, and from run to run.
 * Synchronises the context's stream. */
#define KZ_SOFTMIN_LIST_CHUNK 512 /* entries of a column per first-level wave: part of the summation order */
/* (Also THE ROW TREE OF A CSR ROW: kz_softmin_csr_rows reduces a row of n entries by the tree this call gives a column of n entries.) */
int kz_softmin_list_cols(kz_ctx* ctx, const int64_t* d_colptr, const int32_t* d_col_row, const double* d_col_val, int64_t n_index,
                         int64_t nnz, double eps, const double* d_off, double shift, double* d_out);
/* The Sinkhorn iteration over the lists: from f = 0, n_iter >= 1 times the column step g = kz_softmin_list_cols(d_off = f, shift =
 * eps log(n_q / n_index)) (the first one without offset) and the row step f = kz_softmin_list_rows(d_off = g), bit for bit what the
 * two calls return.  tol >= 0: the loop stops after the column step that moves g by at most tol -- the largest |g_new - g_old|, NaN
 * differences ignored as kz_max_abs_diff ignores them; the row step behind that column step is still taken.  tol < 0: no
 * tolerance.  Writes d_f [n_q] and d_g [n_index] (device), *h_n_iter = the iterations done, *h_change = the last measured change
 * of g and *h_measured = 1 -- or 0, with *h_change = 0, when none was measured (a single iteration); the three host pointers may
 * be NULL.  The transposition and every step are queued at once and the stopping rule is decided on the device (the steps behind
 * the stop return at once); the host reads once, at the end.  n_iter < 1, a NaN tol: KZ_ERR_INVALID; n_q == 0: KZ_OK, nothing is
 * written (*h_n_iter = 0).  Synchronises the context's stream. */
int kz_sinkhorn_lists(kz_ctx* ctx, const double* d_dist, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, double eps,
                      int n_iter, double tol, double* d_f, double* d_g, int* h_n_iter, double* h_change, int* h_measured);
/* Reductions of a rank vector d_rank [n] (entries < 0: no rank).  h_hits[j] (host, j < n_k <= 64) = #(0 <= rank < h_ks[j]);
 * h_out[3] (host) = #(rank >= 0), sum(rank + 1), sum 1 / (rank + 1) -- the float64 sum in a fixed order. */
int kz_rank_stats(kz_ctx* ctx, const int64_t* d_rank, int64_t n, const int64_t* h_ks, int n_k, int64_t* h_hits, double* h_out);

/* ---- one-to-one alignment: stable matching over neighbour lists (kz_match.hip) -- additive, ABI v7 --------------------------- */
/* d_dist [n_q, k] (dist_dtype: KZ_F32 or KZ_F64) and d_ind [n_q, k] on the device: the lists kz_knn, kz_select_topk or kz_knn_reduced
 * return.  Entry (i, c) with 0 <= d_ind[i, c] < n_index is a PAIR of source row i and target row d_ind[i, c] with value
 * w = d_dist[i, c]; any other entry (kz_knn_reduced's INT_MAX padding, a -1) is no pair.  Writes the source-proposing
 * deferred-acceptance (Gale-Shapley) matching: a source row prefers its pairs by column, smaller first; a target row prefers the
 * sources that list it by (key(w), source row), smaller first, key = kz_knn_reduced's order of w widened to double -- NaN counts as
 * +inf, -0.0 equals +0.0, -inf is an ordinary smallest value.  The source-optimal stable matching is unique for fixed preferences,
 * so the result is that of a sequential Gale-Shapley in any order, bit for bit and from run to run; where every row is
 * non-decreasing in key order it equals the greedy assignment over all pairs sorted by (key, source row, column), taking a pair
 * when both ends are free.  A row may list a target twice: each entry is a proposal of its own.
 * d_match[i] = the target row of source row i or -1, d_col[i] = the column of that pair or -1 (both [n_q] on the device).
 * *h_rounds (host, may be NULL) = the number of proposal rounds that had a proposer (at most n_q k + n_index).
 * 1 <= k <= KZ_MAX_CANDIDATES, 1 <= n_index <= 2^31 - 2, n_q <= 2^31 - 2, a known dist_dtype: KZ_ERR_INVALID otherwise, before
 * anything is written; n_q == 0 returns at once.  Rounds are separate launches on the context's stream (integer atomics only, no
 * launch waits for another workgroup); synchronises the stream. */
int kz_match_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                   int64_t* d_match, int64_t* d_col, int64_t* h_rounds);
/* The values of the matched pairs: d_out[i] = d_dist[i, d_col[i]] in d_dist's dtype, NaN where d_col[i] < 0 (d_out: [n_q] on the
 * device).  Enqueued on the context's stream; n_q and k as above. */
int kz_match_values(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_col, int64_t n_q, int k, void* d_out);

/* ---- one-to-one alignment: minimum-cost assignment over neighbour lists (kz_assign.hip) -- additive, ABI v7 ------------------ */
/* The lists of kz_match_lists.  Entry (i, c) is a PAIR when 0 <= d_ind[i, c] < n_index, w = d_dist[i, c] widened to double is finite
 * and w <= unmatched_cost; any other entry (padding, -1, NaN, +-inf) is no pair.  A matching uses every source and every target row
 * at most once; its cost is the sum of w over the matched pairs plus unmatched_cost per unmatched source row.  Writes a matching
 * with cost <= optimum + n_q eps, found by the forward auction in Jacobi form: prices start at 0.0 and all rows FREE; in a round
 * every FREE row computes v_c = (-w_c) - price[t_c] over its pair columns, best = the first column with the largest v (v1), v2 = the
 * largest v of its other pair columns taken together with -unmatched_cost; not v1 > -unmatched_cost: the row is unmatched for good;
 * otherwise it bids (price[t] + (v1 - v2)) + eps on its best target.  A target takes the largest bid, among equal bids the smallest
 * row; the bid becomes the price, the winner the owner, the previous owner FREE.  The rule is synchronous per round and float64
 * add / subtract / compare only: the same arrays from every run, whatever the split into launches.
 * d_match[i] = the target row of source row i or -1, d_col[i] = the column of that pair or -1 (rows still FREE at max_rounds: -1);
 * d_price (device, [n_index], may be NULL) = the final prices; *h_rounds (host, may be NULL) = the rounds that began with a FREE
 * row; *h_converged (host, may be NULL) = 1 when no row is FREE, 0 when max_rounds ended the run -- still KZ_OK and a valid matching.
 * tail_rows: rounds with at most that many FREE rows run inside one single-workgroup launch (0: the default 1024; 1 .. 1024;
 * negative: never), the others as three grid-wide launches each; the result does not depend on it.
 * Limits as kz_match_lists; unmatched_cost finite, eps > 0 finite, max_rounds >= 0: KZ_ERR_INVALID otherwise.  Synchronises. */
int kz_assign_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                    double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col,
                    double* d_price, int64_t* h_rounds, int* h_converged);
/* The smallest and the largest value, widened to double, over the entries with 0 <= d_ind < n_index and a finite value (what the
 * defaults of unmatched_cost and eps are made of): *h_min, *h_max (host); *h_any = 0 and both 0.0 when there is no such entry. */
int kz_assign_range(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                    double* h_min, double* h_max, int* h_any);

/* ---- the same three steps on RAGGED (CSR) pair lists (kz_match.hip, kz_assign.hip, kz_softmin_lists.hip) -- additive, ABI v7 -- */
/* The second list layout: what kz_radius_neighbors returns, or a blocking step's candidate pairs.  d_indptr [n_q + 1] (int64),
 * d_ind [nnz] (int64) and d_dist [nnz] (dist_dtype: KZ_F32 or KZ_F64; the soft-min calls take float64 only) on the device.  Entry
 * p of row i (d_indptr[i] <= p < d_indptr[i + 1]) is a PAIR under exactly the rule of the fixed-width call of the same name: 0 <=
 * d_ind[p] < n_index, and for kz_assign_csr additionally a finite value <= unmatched_cost.  A target may repeat inside a row, a
 * row may be empty, and there is NO LIMIT on the length of a row (the fixed-width calls stop at KZ_MAX_CANDIDATES columns).
 * n_q <= 2^31 - 2, 1 <= n_index <= 2^31 - 2, 0 <= nnz <= 2^31 - 2: KZ_ERR_INVALID otherwise.
 * VALIDATION: every call first runs one small kernel that checks d_indptr[0] == 0, d_indptr non-decreasing and d_indptr[n_q] ==
 * nnz, and reads its flag back BEFORE anything that depends on d_indptr is queued: a bad d_indptr is KZ_ERR_INVALID and never an
 * address.  Each call therefore synchronises the context's stream at least once.
 *
 * kz_match_csr: kz_match_lists' matching, a row walked from d_indptr[i]; d_col[i] = the position of the matched entry INSIDE its
 * row (p - d_indptr[i]) or -1; *h_rounds <= nnz + n_index.  One rule, one kernel body: the propose / tie / resolve kernels are
 * instantiated per row layout.  kz_match_values_csr: d_out[i] = d_dist[d_indptr[i] + d_col[i]], NaN where d_col[i] is outside the
 * row. */
int kz_match_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                 int64_t nnz, int64_t n_index, int64_t* d_match, int64_t* d_col, int64_t* h_rounds);
int kz_match_values_csr(kz_ctx* ctx, const int64_t* d_indptr, const void* d_dist, int dist_dtype, const int64_t* d_col, int64_t n_q,
                        int64_t nnz, void* d_out);
/* kz_assign_csr: kz_assign_lists' auction -- the same synchronous rule, arguments, defaults and outputs, d_col as kz_match_csr.
 * A FREE row reads its whole row in every round it bids, so a row of more than KZ_CSR_LONG_ROW entries bids with ONE WAVE: lane l
 * takes the entries l, l + 64, ... in ascending order, and a 64-lane butterfly merges (v1, first position with v1, v2) by compares
 * only -- ties in v1 go to the smaller position, v2 is the largest of everything else, the losing v1 included -- so the bid is bit
 * for bit the one a single lane computes.  The long rows are found once per call by an ordered compaction of the row ids (no
 * atomics); the wave kernel is indexed by rank.  While a long row is FREE the call stays in grid-wide rounds: the single-workgroup
 * tail starts only when at most tail_rows rows are FREE and none of them is long.  The arrays that come out depend neither on
 * that nor on tail_rows.  kz_assign_range_csr: kz_assign_range over the nnz entries. */
#ifndef KZ_CSR_LONG_ROW
#define KZ_CSR_LONG_ROW 256 /* a row with more entries bids with one wave (profiles/csr_lists.md) */
#endif
int kz_assign_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                  int64_t nnz, int64_t n_index, double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match,
                  int64_t* d_col, double* d_price, int64_t* h_rounds, int* h_converged);
int kz_assign_range_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                        int64_t nnz, int64_t n_index, double* h_min, double* h_max, int* h_any);
/* kz_csr_transpose: kz_lists_transpose's view (d_colptr [n_index + 1], d_col_row int32 [nnz], d_col_val [nnz]) of a CSR: the
 * stable sort of (target id, flat position p), the source row of an entry recovered by binary search in d_indptr.
 * kz_softmin_csr_rows: d_out[i] = softmin_eps over the pairs p of row i of (d_dist[p] - d_off[d_ind[p]]) + shift.  THE ROW TREE OF
 * A CSR ROW IS, BY DEFINITION, THE COLUMN TREE OF ITS ENTRY COUNT: the row step is kz_softmin_list_cols' kernel pair applied to
 * (d_indptr, d_ind, d_dist) with a 64-bit index type -- chunks of KZ_SOFTMIN_LIST_CHUNK entries from the row's own first entry,
 * one wave per chunk, the parts folded by one wave -- so its bits are those of kz_softmin_list_cols on the view (colptr = indptr,
 * col_row = ind, col_val = dist).  An entry that is no pair is +inf and adds an exact zero; a row without a pair gives NaN.
 * kz_sinkhorn_csr: kz_sinkhorn_lists' loop over the two -- every step queued at once (behind the validation), the stopping rule on
 * the device, no float atomics, the same bits from every run; arguments and outputs as kz_sinkhorn_lists. */
int kz_csr_transpose(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                     int64_t n_index, int64_t* d_colptr, int32_t* d_col_row, double* d_col_val, int64_t* h_nnz);
int kz_softmin_csr_rows(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                        int64_t n_index, double eps, const double* d_off, double shift, double* d_out);
int kz_sinkhorn_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const double* d_dist, int64_t n_q, int64_t nnz,
                    int64_t n_index, double eps, int n_iter, double tol, double* d_f, double* d_g, int* h_n_iter, double* h_change,
                    int* h_measured);

/* ---- NEIGHBOUR PAIRS OF BOTH DIRECTIONS AS A CSR (kz_pairs.hip, kz_pairs.h) -- additive, ABI v7 -------------------------------- */
/* The producer in front of the three CSR calls above.  F = the pairs (i, j) with target row j in the forward list of source row i,
 * R = the pairs (i, j) with source row i in the reverse list of target row j.  MEMBERSHIP IS BY THE LISTS the caller brings (the raw
 * lists of two kz_knn searches: ties are the search's business), never by a value.
 *
 * kz_lists_combine: the set step.  d_fwd_ind [n_q, k_f]: target ids per source row; d_rev_ind [n_index, k_r]: source ids per target
 * row (int64, on the device; k_f != k_r is fine).  An entry whose id is outside its range -- a target id outside [0, n_index) in a
 * forward list, a source id outside [0, n_q) in a reverse list: kz_match_lists' rule, so -1, kz_knn_reduced's INT_MAX padding and an
 * id >= n -- is no pair; an id repeated inside a row counts once.  mode: KZ_PAIRS_FORWARD = F, KZ_PAIRS_REVERSE = R grouped by source
 * row (the transposed reverse lists), KZ_PAIRS_UNION = F u R, KZ_PAIRS_MUTUAL = F n R; every pair once.  FORWARD does not read
 * d_rev_ind and REVERSE does not read d_fwd_ind (they may be NULL).
 * Output and CAPACITY CONTRACT: kz_radius_neighbors'.  d_indptr [n_q + 1] (int64, device) and *h_total (host) = the number of pairs
 * are ALWAYS complete and exact; capacity = 0 is the count-only call (d_ind may be NULL); d_ind [capacity] (int64, device) receives
 * the target ids of every row whose end offset d_indptr[i + 1] is <= capacity, at d_indptr[i] .., ascending by target id; for any
 * other row NOTHING is written, and the call returns KZ_OK all the same.
 * How: the entries the mode reads are ordered by (source row, target row) with two passes of the stable radix sort (kz_sort.hip); the
 * first entry of every run of equal pairs decides by the sides present in its run; places are an integer prefix sum of those flags.
 * Integer keys, counts and scans; no atomics on the output; nothing depends on the order anything runs in: two calls give identical
 * bytes.  One thread per ENTRY: a row of any length (a hub source can be listed by every target) costs what its entries cost.
 * 1 <= k_f, k_r <= KZ_MAX_CANDIDATES, 0 <= n_q <= 2^31 - 2, 1 <= n_index <= 2^31 - 2, capacity >= 0, a known mode: KZ_ERR_INVALID
 * otherwise; more than 2^31 - 2 list entries read (n_q k_f + n_index k_r for UNION / MUTUAL; the total is at most that):
 * KZ_ERR_UNSUPPORTED; n_q == 0: KZ_OK with d_indptr[0] = 0.  Transient device memory: about 32 bytes per list entry read (the sort's included).  Synchronises the
 * context's stream. */
#define KZ_PAIRS_FORWARD 0
#define KZ_PAIRS_REVERSE 1
#define KZ_PAIRS_UNION 2
#define KZ_PAIRS_MUTUAL 3
int kz_lists_combine(kz_ctx* ctx, const int64_t* d_fwd_ind, int64_t n_q, int k_f, const int64_t* d_rev_ind, int64_t n_index, int k_r,
                     int mode, int64_t capacity, int64_t* d_indptr, int64_t* d_ind, int64_t* h_total);
/* kz_pairs_values: d_out[p] (float64 [nnz], device) = the value of entry p of the CSR (d_indptr [n_q + 1], d_ind [nnz]) between the
 * query row i that holds p (rows 0 .. n_q - 1 of `query`, n_q <= query.n) and index row d_ind[p]:
 *   kind 0               the distance kz_knn returns for query row i and index row d_ind[p] -- kz_output_distance of the exact ranking
 *                        value, kz_pair_values' canonical dot product; ALWAYS this direction's value, whichever list named the pair;
 *   a KZ_RANK_* kind     w of kz_gold_ranks_reduced / kz_knn_reduced (kind, the four state vectors and their validation as there;
 *                        kind 0: all four NULL), d_q_a / d_q_b indexed by i, d_t_a / d_t_b by d_ind[p].
 * The same expressions as kz_radius_neighbors[_reduced], so a pair has the bits that call returns for it with radius = +inf -- and,
 * for a pair of a forward list, the bits of kz_knn's distance (kind 0) or of kz_csls / kz_local_scaling / kz_mp_normal / kz_dual_shift.
 * Every metric and row dtype kz_pair_values serves (float16 / bfloat16 rows included), and a precomputed pair of views: the matrix
 * entry, widened.  A NaN value is written as it is (the caller decides what it means); an entry whose id is outside [0, index.n):
 * NaN.  The indptr validation of the CSR calls runs first; limits as there (kz_csr_require); matrices that disagree: KZ_ERR_INVALID.
 * One wave per entry (one lane for the Minkowski family, the boolean metrics and precomputed values), the row of an entry by binary
 * search in d_indptr; then one pointwise kernel in place.  Synchronises the context's stream. */
int kz_pairs_values(kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index, const int64_t* d_indptr, const int64_t* d_ind,
                    int64_t n_q, int64_t nnz, int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a,
                    const double* d_t_b, double* d_out);
/* kz_csr_sort_rows: every row of a float64 CSR (d_ind / d_dist [nnz], permuted together, in place) ascending by (value, index row) in
 * the order of kz_knn_reduced -- kz_radius_neighbors' sort with both of its branches (a row of up to 4096 entries in LDS, a longer
 * one by a stable radix sort through a transient second copy of the CSR: KZ_ERR_NOMEM when it does not fit).  A NaN value orders as
 * +inf: last, by index row.  Ids must be below 2^31 - 1.  The indptr validation runs first.  Synchronises the context's stream. */
int kz_csr_sort_rows(kz_ctx* ctx, const int64_t* d_indptr, int64_t n_q, int64_t nnz, int64_t n_index, int64_t* d_ind, double* d_dist);

/* ---- ENTITY CLUSTERS: the connected components of a pair list (kz_components.hip) -- additive, ABI v7 ------------------------- */
/* The third way to resolve a many-to-many pair list, beside the one-to-one calls and Sinkhorn: its transitive closure.  The graph is
 * bipartite: source row i is node i, target row j is node n_q + j, and every stored entry (i, d_ind[p]) with 0 <= d_ind[p] < n_index
 * is an edge (any other entry -- a -1, kz_knn_reduced's INT_MAX padding, an id >= n_index -- is no pair: kz_match_lists' rule; a pair
 * stored twice is one edge; values are not read).  EVERY node belongs to a component: a source row without a pair and a target row
 * nobody lists are components of one node.  Components are numbered 0 .. C - 1 IN THE ORDER OF THEIR SMALLEST NODE, source rows before
 * target rows (so d_label_q[0] == 0 whenever n_q > 0): one answer, the same bytes in every run, whatever order anything ran in.
 *   d_label_q [n_q], d_label_t [n_index]   (int64, device) the component of every source row and of every target row;
 *   d_size_q, d_size_t                     (int64, device; BOTH NULL or both given, each with room for n_q + n_index entries) the
 *                                          number of source rows and of target rows of component c, c < *h_n_components; entries
 *                                          behind that are not written.  A source singleton has (1, 0), a target singleton (0, 1);
 *   *h_n_components                        (host) C.
 * kz_components_csr reads the CSR (d_indptr [n_q + 1], d_ind [nnz]) after the indptr validation of every CSR call;
 * kz_components_lists reads fixed-width lists d_ind [n_q, k] (any k >= 1: k is no candidate count here).
 * How: union-find on int32 parent words with parent[v] <= v ALWAYS.  One thread per ENTRY (a hub row of 10^5 entries costs what 10^5
 * entries of short rows cost) finds the two roots with path halving and links the larger root under the smaller with one
 * compare-and-swap, continuing from the value it read when it loses.  The root of a finished tree is the smallest node of the
 * component.  Then: every node stores its root, an exclusive integer prefix sum of the root flags numbers the roots, and (when asked)
 * the sizes are integer adds, pre-aggregated per wave.  Integer arithmetic and integer atomics only; no kernel waits for another
 * workgroup; every loop is bounded by decreasing node ids.
 * Limits, all decided BEFORE anything is launched: kz_csr_require's (0 <= n_q, nnz <= 2^31 - 2, 1 <= n_index <= 2^31 - 2), k >= 1,
 * one size array without the other: KZ_ERR_INVALID; n_q + n_index >= 2^31 - 1 (node ids are int32) or, for lists, n_q k > 2^31 - 2:
 * KZ_ERR_UNSUPPORTED.  n_q == 0 and nnz == 0 are legal (every node a singleton).  Transient device memory: 12 bytes per node.
 * Synchronises the context's stream. */
int kz_components_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, int64_t n_q, int64_t nnz, int64_t n_index,
                      int64_t* d_label_q, int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components);
int kz_components_lists(kz_ctx* ctx, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, int64_t* d_label_q,
                        int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components);

/* kz_components_edges: the same answer for an EDGE ARRAY -- edge e joins source row d_source[e] and target row d_target[e], e < count
 * (int64 [count], device; any order, an edge may repeat; an edge with an id outside [0, n_q) / [0, n_index) is no pair).  Outputs,
 * numbering and limits as kz_components_csr (count in the place of nnz); the same stage kernels behind a hook with one thread per edge.
 * This is what labels a cut of kz_forest_*'s forest: its first `searchsorted(value, t)` edges.  Synchronises the context's stream. */
int kz_components_edges(kz_ctx* ctx, const int64_t* d_source, const int64_t* d_target, int64_t count, int64_t n_q, int64_t n_index,
                        int64_t* d_label_q, int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components);

/* ---- THE SINGLE-LINKAGE HIERARCHY of a pair list: its minimum spanning forest (kz_forest.hip) -- additive, ABI v7 ------------------ */
/* The components of the pairs with value <= t, for EVERY threshold t, from one call: the minimum spanning forest (MSF) of the weighted
 * pair graph.  The graph is kz_components_*'s (source row i is node i, target row j node n_q + j) with one more rule: entry p is an
 * EDGE when 0 <= d_ind[p] < n_index AND its value is not NaN (NaN is <= no threshold); -inf, +inf, -0.0 and negative values are
 * legal; a pair stored twice is two edges.  p is the entry's flat position: the CSR position, or i k + c for lists [n_q, k].
 * ORDER: edge p comes before p' when (key(w_p), p) < (key(w_p'), p'), key the order-preserving 64-bit pattern of the value widened
 * to float64 with -0.0 == +0.0 and -inf first (kz_order_key.h).  A strict total order: the MSF under it is unique -- the forest
 * Kruskal's algorithm builds taking the edges in that order -- and the result has the same bytes in every run.
 *   d_source, d_target, d_entry (int64), d_value (float64)   (device, each with room for max(n_q + n_index - 1, 1) entries) the
 *                                          m = n_q + n_index - C forest edges ascending in the order above: the two rows, the value
 *                                          widened, the position p; entries behind m are not written;
 *   *h_n_edges, *h_n_components            (host) m and C, the number of components of all edges;
 *   *h_rounds                              (host, may be NULL) the Boruvka rounds that joined something (<= 31).
 * The components at threshold t are those of the first `number of d_value <= t` edges (the values are non-decreasing under the
 * IEEE comparison): kz_components_edges on that prefix equals kz_components_csr on the entries with value <= t, bit for bit.
 * How: Boruvka in rounds, one thread per ENTRY.  Per round every entry between two components offers its key to both with an
 * unsigned 64-bit atomicMin (behind a relaxed load that skips the atomic when the key is not smaller), a second pass breaks ties by
 * position with an int atomicMin, every component marks its pick and hooks under the other end's component (of a mutual pick the
 * smaller root stays), and the component array is flattened by pointer jumping.  One flag word is read back per round; the loop
 * stops at the first round that joined nothing.  The marked entries are compacted by an integer scan and sorted by (key, p) with
 * kz_csr_sort_rows' kernel.  Integer atomics only; no kernel waits for another workgroup; every loop is bounded.
 * Limits, decided BEFORE anything is launched: kz_csr_require's (CSR), k >= 1 and the n_q / n_index ranges (lists), a dist_dtype that
 * is not KZ_F32 / KZ_F64, a null output: KZ_ERR_INVALID; n_q + n_index >= 2^31 - 1 or n_q k > 2^31 - 2: KZ_ERR_UNSUPPORTED.  The CSR
 * call runs the indptr validation of every CSR call first.  n_q == 0 and nnz == 0 are legal: m = 0, C = n_q + n_index.
 * Transient device memory: 20 bytes per node and 12 bytes per entry, plus 16 bytes per forest edge for the sort when m > 4096.
 * Synchronises the context's stream (once per round). */
int kz_forest_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q, int64_t nnz,
                  int64_t n_index, int64_t* d_source, int64_t* d_target, double* d_value, int64_t* d_entry, int64_t* h_n_edges,
                  int64_t* h_n_components, int* h_rounds);
int kz_forest_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                    int64_t* d_source, int64_t* d_target, double* d_value, int64_t* d_entry, int64_t* h_n_edges, int64_t* h_n_components,
                    int* h_rounds);

/* float64 -> float32 cast of an [count] array (cosine + float32 inputs keep the reference's output dtype). */
int kz_cast_f64_f32(kz_ctx* ctx, const double* d_in, float* d_out, int64_t count);

/* Self-test hook (tests/test_gpu_fast_div.py): the shared-reciprocal division of the cosine re-rank (kz_div_shared, kz_common.h)
 * against the plain float64 division on `count` pseudo-random pairs (numerator a float32 value, divisor a norm >= |a|; `mode`
 * 1: numerators and divisors with all-ones / single-bit significands mixed in); *h_mismatch = pairs whose bits differ. */
int kz_selftest_div(kz_ctx* ctx, int64_t count, uint64_t seed, int mode, int64_t* h_mismatch);

/* Self-test hook (tests/test_gpu_images.py): the raw device bytes of one of the per-matrix buffers every MFMA search starts from
 * -- norms, bias, maxima, the float32 / split-bf16 / fp16 operand images, the fp16 centre and row statistics -- built (where it
 * is lazy) by the functions kz_knn calls, copied to h_dst as they lie in HBM: no un-layouting, no arithmetic.  *h_bytes = the
 * buffer's size; capacity 0 asks for the size only, a smaller capacity than the size is KZ_ERR_INVALID.  `partner` (may be NULL):
 * the matrix the fp16 image shares its centre with (the index of a search whose query is m).  `arg`: the number of index ranges
 * (KZ_IMG_DEALT_*) or of rows in the host list h_rows (KZ_IMG_ROWS_*: packed into the next multiple of 128 image rows).
 * KZ_ERR_NONFINITE for a matrix whose rows were flagged; KZ_ERR_INVALID for rows-only, precomputed and boolean matrices and, for
 * the fp16 buffers, widths without an fp16 tier.  Synchronises. */
enum {
    KZ_IMG_SQN = 0,      /* double [n] */
    KZ_IMG_BIAS,         /* float [n_pad] */
    KZ_IMG_STATS,        /* 40 bytes: double max norm, double max |operand|, 16 bytes unused, int non-finite flag, int unused */
    KZ_IMG_F32,          /* float [n_tiles][d_pad / 4][128][4] */
    KZ_IMG_BF,           /* uint16 [n_tiles][d_pad / 16][hi0, hi1, lo0, lo1][128][8] */
    KZ_IMG_NORM64,       /* double [n][d], 0 bytes when the matrix gets none */
    KZ_IMG_CORR,         /* double [n][2], 0 bytes unless the metric is KZ_CORRELATION */
    KZ_IMG_MU,           /* float [16 nsr] */
    KZ_IMG_SCALE,        /* double {S, 1 / S^2} */
    KZ_IMG_H,            /* fp16 [n_tiles][nsr][2][128][8] (without the padding behind the image) */
    KZ_IMG_H_BIAS,       /* float [n_pad] */
    KZ_IMG_ROWQ,         /* double [n][3] */
    KZ_IMG_DMAX,         /* double [3] */
    KZ_IMG_DEALT_PERM,   /* int [n_pad] */
    KZ_IMG_DEALT_H,
    KZ_IMG_DEALT_BIAS,
    KZ_IMG_ROWS_H,
    KZ_IMG_ROWS_BIAS
};
int kz_selftest_image(kz_ctx* ctx, kz_matrix* m, kz_matrix* partner, int what, int64_t arg, const int* h_rows, void* h_dst,
                      size_t capacity, size_t* h_bytes);

/* Self-test hook (tests/test_gpu_finalize_direct.py): the finalize kernels of kz_knn (merge a query's candidate lists, select, re-rank
 * in float64, certify) on candidate lists the CALLER supplies, through the launcher and the parameter fill every search uses.  Nothing
 * of the kernels is restated: the hook validates the geometry, copies the host arrays to the device, launches and copies back.
 *   tier      0: the float32 / split-bf16 bound with the caller's `gamma`;  2: the fp16 bound (the images are built as kz_knn builds
 *             them, the context's eps_scale applies; needs contig = 1 and a width that has an fp16 image)
 *   layout    n_regions regions of query tiles [qt_end[r-1], qt_end[r]) with pieces[r] index ranges each; `halves` lists per (query,
 *             range); contig 1: every list is KP contiguous entries, 0: the wave-interleaved layout.  The region bases follow as the
 *             planner lays them out; h_key / h_idx hold n_list = sum over regions of tiles x 128 x pieces x (contig ? KP : 2 KP) entries.
 *   rows      local query q = 0 .. q_count - 1 is list row list_row0 + q and query row q_begin + q (image row, with h_row_map)
 *   optional  (NULL: absent) h_self_ids [q_count]; h_list_floor, h_excl_floor, h_row_map [query rows]; h_idx_map [n_idx_map]
 *   outputs   h_out_dist / h_out_ind [rows][k] (rows = q_count, with h_row_map: the query's rows), NaN / -1 where nothing was written;
 *             h_fail_list / h_fail_tau [q_count], *n_fail entries of them set; *err_ratio; *build = KZ_FIN_BUILD_* of the launches
 * KZ_ERR_INVALID, before anything is launched, for: an id outside [-1, n_i) (after h_idx_map), a map entry that is no row, KP outside
 * {16, 32, 64, 128}, more than 4096 entries per query, lists that do not fit the kernel's LDS, 0 < KSEL < k_eff (KSEL = 0: KP < k_eff),
 * tier 2 on an interleaved layout or a width without fp16 image, h_idx_map on an interleaved layout (only the contiguous gather applies
 * it), h_excl_floor with anything but one list of KP entries per query, all selected, and no h_list_floor (the reverse direction of a
 * shared sweep, whose bound counts nothing else), metrics other than the euclidean family and cosine.  Synchronises. */
enum { KZ_FIN_BUILD_ORDINARY = 0, KZ_FIN_BUILD_TWO_LOADS, KZ_FIN_BUILD_MANY, KZ_FIN_BUILD_WIDE };
typedef struct kz_selftest_fin {
    int32_t k, exclude_self, tier, KP, KSEL;
    int32_t n_regions, halves, contig, dual_col, n_idx_map;
    int32_t qt_end[8], pieces[8];
    double gamma;
    int64_t q_begin, q_count, list_row0, n_list;
    const float* h_key;
    const int32_t* h_idx;
    const int64_t* h_self_ids;
    const float* h_list_floor;
    const float* h_excl_floor;
    const int32_t* h_idx_map;
    const int32_t* h_row_map;
    double* h_out_dist;
    int64_t* h_out_ind;
    int32_t* h_fail_list;
    double* h_fail_tau;
    int32_t n_fail, build;
    double err_ratio;
} kz_selftest_fin;
int kz_selftest_finalize(kz_ctx* ctx, kz_matrix* query, kz_matrix* index, kz_selftest_fin* t);

/* Self-test hook (tests/test_gpu_sweep_direct.py): ONE launch of one entry of the sweep-kernel table over query rows [q_begin, q_begin
 * + q_count) against the whole index, through the stages every search runs -- the tier's operand images, the resolver, the chunk's
 * plan, scratch carve-up and work table, the sweep launch -- and nothing behind them: the candidate lists (and, dual builds, the event
 * log) come back as they lie on the device.  Nothing of the kernels is restated.  The plain images are swept (not the row-dealt or the
 * sorted ones).
 *   entry     tier 0 float32 / 1 split-bf16 / 2 fp16; KP 16 / 32 / 64 / 128; q64: the 64-queries-per-wave build; dual: the dual-pass
 *             build (fp16 only, as q64); n_ranges >= 1: index ranges per query tile (what option "force_splits" sets)
 *   optional  h_qfloor [query rows padded to 128] (fp16 only): the lists start full of (qfloor, no row) entries
 *   dual      h_theta [index tiles x 128], h_qnbias [query rows padded to 128], log_cap >= 1; h_log_keys [4 log_cap] / h_log_meta
 *             [2 log_cap] receive the first min(log_count, log_cap) entries, log_count the device counter
 *   outputs   n_list = entries of the launch's lists; the layout (n_regions, qt_end, pieces, base, halves, contig), KP, qt0 (first query
 *             tile of the launch: list row = query row - 128 qt0) and the entry that ran (wg_per_item, tiles_per_item, n_slices).
 *             With h_out_key == NULL nothing is launched and these are all the call returns (the caller sizes its arrays by n_list);
 *             else list_capacity >= n_list entries of h_out_key / h_out_idx receive the raw arrays (bytes the kernel did not write
 *             read as NaN / -1).
 * KZ_ERR_UNSUPPORTED for a combination without a build (q64 or dual off the fp16 tier, a width the tier has no kernel for);
 * KZ_ERR_INVALID, before anything is launched, for: q_count < 1, rows a single launch does not take, precomputed / boolean / rows-only
 * matrices, metrics other than the euclidean family and cosine, matrices of another context, a floor off the fp16 tier, a dual build
 * without its three inputs.  Synchronises. */
typedef struct kz_selftest_swp {
    int32_t tier, KP, q64, dual, n_ranges;
    int64_t q_begin, q_count;
    const float* h_qfloor;
    const float* h_theta;
    const float* h_qnbias;
    int64_t log_cap;
    int64_t list_capacity;
    float* h_out_key;
    int32_t* h_out_idx;
    float* h_log_keys;
    int32_t* h_log_meta;
    int64_t n_list;
    uint64_t log_count;
    int32_t n_regions, halves, contig, qt0;
    int32_t qt_end[8], pieces[8];
    int64_t base[8];
    int32_t wg_per_item, tiles_per_item, n_slices, entry_KP, n_items, reserved;
} kz_selftest_swp;
int kz_selftest_sweep(kz_ctx* ctx, kz_matrix* query, kz_matrix* index, kz_selftest_swp* t);

#ifdef __cplusplus
}
#endif
#endif /* KIEZ_AMD_H */
