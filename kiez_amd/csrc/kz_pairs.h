// NEIGHBOUR PAIRS AS A CSR, the half that lives in kz_knn.hip's translation unit (the other half: kz_pairs.hip): the VALUE of every
// entry of a CSR as the list calls return it, and the ROW SORT of a CSR.
//   kz_pairs_values    kz_pairs_raw_values (kz_pairs.hip: the exact ranking value of every entry, kz_pair_values' bits), then ONE
//                      pointwise kernel that converts it in place -- kind 0: kz_output_distance<T> (the distance kz_knn returns), a
//                      KZ_RANK_* kind: kz_rank_reduce<T, KIND, METRIC> with the state of the entry's query row and index row --
//                      instantiated by THE dispatch of kz_gold_ranks.h.  These are the expressions kz_radius_w evaluates on the exact
//                      stage's value matrix, so a pair has the bits kz_radius_neighbors[_reduced](+inf) returns for it, whether or not
//                      it lies in a neighbour list.  An entry whose id is no index row: NaN.
//   kz_csr_sort_rows   kz_radius_sort_kernel (kz_radius.h) on any float64 CSR: rows ascending by (kz_knnr_key(value), index row), the
//                      bitonic network in LDS up to KZ_RADIUS_SORT_LDS entries and the stable radix sort through a second copy
//                      beyond; NaN orders as +inf and therefore last, by index row.  No second sort exists.
#pragma once
#include "kz_rows.h"   // kz_csr_row_of, kz_csr_require, kz_csr_validate

int kz_pairs_raw_values(kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index, const int64_t* d_indptr, const int64_t* d_ind, int64_t n_q,
                        int64_t nnz, double* d_out);   // kz_pairs.hip

// One lane per entry, in place.  KZ_RANK_NONE reads no state (and no indptr).
template <typename T, int KIND, int METRIC>
__global__ __launch_bounds__(256) void kz_pairs_convert_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ ind, int64_t n_q,
                                                               int64_t nnz, int64_t n_i, double mp, const double* __restrict__ q_a,
                                                               const double* __restrict__ q_b, const double* __restrict__ t_a,
                                                               const double* __restrict__ t_b, double* __restrict__ vals) {
    constexpr bool ONE = KIND != KZ_RANK_NONE, TWO = KIND == KZ_RANK_MP_NORMAL;   // state vectors per side
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t j = ind[e];
        if (j < 0 || j >= n_i) {
            vals[e] = NAN;
            continue;
        }
        const int64_t row = ONE ? kz_csr_row_of(indptr, n_q, e) : 0;
        vals[e] = kz_radius_w<T, KIND, METRIC>(vals[e], mp, ONE ? q_a[row] : 0.0, TWO ? q_b[row] : 0.0, ONE ? t_a[j] : 0.0, TWO ? t_b[j] : 0.0);
    }
}

extern "C" int kz_pairs_values(kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index, const int64_t* d_indptr, const int64_t* d_ind,
                               int64_t n_q, int64_t nnz, int kind, const double* d_q_a, const double* d_q_b, const double* d_t_a,
                               const double* d_t_b, double* d_out) {
    const int rcp = kz_require_pair("kz_pairs_values", ctx, query, 0, n_q, index, d_indptr, d_indptr);
    if (rcp != KZ_OK) return rcp;
    KZ_REQUIRE(nnz <= 0 || (d_ind && d_out), "kz_pairs_values: null argument");   // (nnz == 0: there is no entry to read or write)
    const int rcq = kz_csr_require("kz_pairs_values", ctx, n_q, nnz, index->n);
    if (rcq != KZ_OK) return rcq;
    if (kind != KZ_RANK_NONE) {
        const int rcr = kz_rank_require_reduction("kz_pairs_values", kind, d_q_a, d_q_b, d_t_a, d_t_b);
        if (rcr != KZ_OK) return rcr;
    } else {
        KZ_REQUIRE(!d_q_a && !d_q_b && !d_t_a && !d_t_b, "kz_pairs_values: the state vectors belong to a KZ_RANK_* kind and must be NULL for kind 0");
    }
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_pairs_values", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    if (nnz == 0) return KZ_OK;
    const int rc = kz_pairs_raw_values(ctx, query, index, d_indptr, d_ind, n_q, nnz, d_out);
    if (rc != KZ_OK) return rc;
    const int64_t b = (nnz + 255) / 256;
    const dim3 grid((unsigned)(b < 4096 ? b : 4096));
    auto go = [&](auto t, auto kd, auto metric) {
        hipLaunchKernelGGL((kz_pairs_convert_kernel<typename decltype(t)::type, decltype(kd)::value, decltype(metric)::value>), grid, dim3(256), 0,
                           ctx->stream, d_indptr, d_ind, n_q, nnz, index->n, index->mink_p, d_q_a, d_q_b, d_t_a, d_t_b, d_out);
    };
    if (kind == KZ_RANK_NONE)
        kz_rank_dispatch_distance(index, [&](auto t, auto metric) { go(t, KzRankC<KZ_RANK_NONE>(), metric); });
    else
        kz_rank_dispatch(kind, index, go);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

extern "C" int kz_csr_sort_rows(kz_ctx* ctx, const int64_t* d_indptr, int64_t n_q, int64_t nnz, int64_t n_index, int64_t* d_ind, double* d_dist) {
    const int rcq = kz_csr_require("kz_csr_sort_rows", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(nnz == 0 || (d_ind && d_dist), "kz_csr_sort_rows: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_csr_sort_rows", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    if (nnz < 2) return KZ_OK;
    // (released when the function returns, stream-ordered)
    KzPoolBuf<double> tmp_w;   // the radix path's second copy: only a CSR of more than KZ_RADIUS_SORT_LDS entries can hold a row that long
    KzPoolBuf<int64_t> tmp_i;
    if (nnz > KZ_RADIUS_SORT_LDS) {
        int rc = tmp_w.alloc(ctx, (size_t)nnz * sizeof(double));
        if (rc == KZ_OK) rc = tmp_i.alloc(ctx, (size_t)nnz * sizeof(int64_t));
        if (rc != KZ_OK) return rc;
    }
    hipLaunchKernelGGL(kz_radius_sort_kernel, dim3((unsigned)n_q), dim3(256), 0, ctx->stream, d_indptr, nnz, d_dist, d_ind, tmp_w.get(), tmp_i.get());
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}
