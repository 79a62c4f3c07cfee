// THE ROW LAYOUT of a pair list: where row i starts in dist / ind and how many entries it has.  Every kernel of kz_match.hip,
// kz_assign.hip and kz_components.hip that walks a row is instantiated once per layout -- one rule, one body: KzRowsFixed the
// [n_q, k] neighbour lists, KzRowsCsr a CSR's indptr.  A CSR's indptr is checked by kz_csr_validate BEFORE any kernel that reads
// through it is queued.  This header and kz_rows.hip are the one place of the native code that knows the two layouts apart.
#pragma once
#include "kz_common.h"

struct KzRowsFixed {
    int k;
    __device__ __forceinline__ int64_t start(int64_t i) const { return i * k; }
    __device__ __forceinline__ int len(int64_t) const { return k; }
    __device__ __forceinline__ bool is_long(int64_t) const { return false; }   // (kz_assign.hip: no wave bid, whatever k is)
};

// a row with more entries than this bids with one wave in kz_assign_csr (include/kiez_amd.h; -DKZ_CSR_LONG_ROW=2147483647 builds
// the library without the wave path, the variant profiles/csr_lists.md measures it against)
struct KzRowsCsr {
    const int64_t* __restrict__ indptr;
    __device__ __forceinline__ int64_t start(int64_t i) const { return indptr[i]; }
    __device__ __forceinline__ int len(int64_t i) const { return (int)(indptr[i + 1] - indptr[i]); }   // (nnz < 2^31)
    __device__ __forceinline__ bool is_long(int64_t i) const { return indptr[i + 1] - indptr[i] > (int64_t)KZ_CSR_LONG_ROW; }
};

// The row of a validated CSR that holds entry p (0 <= p < nnz = indptr[n_q]): the largest i with indptr[i] <= p.  Empty rows hold
// nothing: the search steps over them.  (kz_pairs.hip, kz_pairs.h: the kernels that take one thread or one wave per ENTRY.)
__device__ __forceinline__ int64_t kz_csr_row_of(const int64_t* __restrict__ indptr, int64_t n_q, int64_t p) {
    int64_t lo = 0, hi = n_q;   // (indptr[lo] <= p < indptr[hi])
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (indptr[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// THE HOST SIDE of the layout (kz_rows.hip): the limits every CSR call shares and the check kernel over indptr with its flag read
// back (synchronises the stream); the limits of the fixed-width calls -- kz_match_require those that take float32 or float64 values
// (kz_match.hip, kz_assign.hip), kz_sl_require those that take float64 ones and an entry count (kz_softmin_lists.hip)
int kz_csr_require(const char* who, kz_ctx* ctx, int64_t n_q, int64_t nnz, int64_t n_index);
int kz_csr_validate(const char* who, kz_ctx* ctx, const int64_t* d_indptr, int64_t n_q, int64_t nnz);
int kz_match_require(const char* who, kz_ctx* ctx, const void* d_dist, int dist_dtype, int64_t n_q, int k);
int kz_sl_require(const char* who, kz_ctx* ctx, int64_t n_q, int k, int64_t n_index);

// The exclusive prefix sum of `total` >= 1 int flags (kz_pairs.hip: tile sums, one workgroup over the tile totals, the tile again),
// queued on the context's stream: d_place[p] = the flags in front of place p, d_place[total] = their sum; d_tile: scratch of
// ceil(total / 256) ints.  Integer adds: the same bytes from every run.
void kz_scan_flags(kz_ctx* ctx, const int* d_keep, int total, int* d_tile, int* d_place);

// THE dispatch on a pair list's value type: f(the typed pointer) for a dist_dtype a *_require has checked (KZ_F32 or KZ_F64)
template <typename F>
static inline auto kz_with_values(int dist_dtype, const void* d_dist, F&& f) {
    return dist_dtype == KZ_F32 ? f((const float*)d_dist) : f((const double*)d_dist);
}
