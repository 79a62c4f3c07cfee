// THE HOST SIDE OF THE ROW LAYOUT (kz_rows.h): the argument limits of the fixed-width and of the CSR calls, and the check of a CSR's
// indptr that runs before anything reads through it.  Shared by kz_match.hip, kz_assign.hip, kz_softmin_lists.hip, kz_components.hip
// and the pair calls of kz_pairs.h.
#include "kz_rows.h"
#include "kz_pool_buf.h"

// the fixed-width lists of float32 or float64 values
int kz_match_require(const char* who, kz_ctx* ctx, const void* d_dist, int dist_dtype, int64_t n_q, int k) {
    KZ_REQUIRE(ctx != nullptr, "%s: null context", who);
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "%s: dist_dtype must be KZ_F32 or KZ_F64, got %d", who, dist_dtype);
    KZ_REQUIRE(k >= 1 && k <= KZ_MAX_CANDIDATES, "%s: lists of 1 .. %d columns, got k = %d", who, KZ_MAX_CANDIDATES, k);
    KZ_REQUIRE(n_q >= 0 && n_q < 0x7fffffffLL, "%s: n_q = %lld is outside [0, 2^31 - 1)", who, (long long)n_q);
    KZ_REQUIRE(n_q == 0 || d_dist != nullptr, "%s: null list", who);
    return KZ_OK;
}

// the fixed-width lists of the soft-min calls: float64 values, the entries counted as a CSR's are
int kz_sl_require(const char* who, kz_ctx* ctx, int64_t n_q, int k, int64_t n_index) {
    KZ_REQUIRE(ctx != nullptr, "%s: null context", who);
    KZ_REQUIRE(k >= 1 && k <= KZ_MAX_CANDIDATES, "%s: lists of 1 .. %d columns, got k = %d", who, KZ_MAX_CANDIDATES, k);
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "%s: n_index = %lld is outside [1, 2^31 - 1)", who, (long long)n_index);
    KZ_REQUIRE(n_q >= 0 && n_q * (int64_t)k < 0x7fffffffLL, "%s: n_q k = %lld entries, the limit is 2^31 - 2", who, (long long)(n_q * (int64_t)k));
    return KZ_OK;
}

// the limits every CSR call shares
int kz_csr_require(const char* who, kz_ctx* ctx, int64_t n_q, int64_t nnz, int64_t n_index) {
    KZ_REQUIRE(ctx != nullptr, "%s: null context", who);
    KZ_REQUIRE(n_q >= 0 && n_q < 0x7fffffffLL, "%s: n_q = %lld is outside [0, 2^31 - 1)", who, (long long)n_q);
    KZ_REQUIRE(nnz >= 0 && nnz < 0x7fffffffLL, "%s: nnz = %lld entries, the limit is 2^31 - 2", who, (long long)nnz);
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "%s: n_index = %lld is outside [1, 2^31 - 1)", who, (long long)n_index);
    return KZ_OK;
}

// flag |= 1 unless indptr[0] == 0, indptr[i - 1] <= indptr[i] for every i and indptr[n_q] == nnz: together, every row lies in [0, nnz)
__global__ __launch_bounds__(256) void kz_csr_validate_kernel(const int64_t* __restrict__ indptr, int64_t n_q, int64_t nnz, int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_q; i += stride) {
        const int64_t v = indptr[i];
        const bool bad = (i == 0 && v != 0) || (i == n_q && v != nnz) || (i > 0 && indptr[i - 1] > v);
        if (bad) atomicOr(flag, 1);
    }
}

// Runs the check kernel and READS ITS FLAG: nothing that reads through d_indptr is queued before this returns KZ_OK.
int kz_csr_validate(const char* who, kz_ctx* ctx, const int64_t* d_indptr, int64_t n_q, int64_t nnz) {
    KZ_REQUIRE(d_indptr != nullptr, "%s: null indptr", who);
    KzPoolBuf<int> flag;
    const int rc = flag.alloc(ctx, 16);
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemsetAsync(flag.get(), 0, 16, ctx->stream));
    hipLaunchKernelGGL(kz_csr_validate_kernel, dim3(kz_blocks(n_q + 1, 256)), dim3(256), 0, ctx->stream, d_indptr, n_q, nnz, flag.get());
    KZ_HIP(hipGetLastError());
    int h_flag = 0;
    KZ_HIP(hipMemcpyAsync(&h_flag, flag.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    KZ_REQUIRE(h_flag == 0, "%s: indptr must start at 0, never decrease and end at nnz = %lld", who, (long long)nnz);
    return KZ_OK;
}
