// metric = 'precomputed' (KZ_PRECOMPUTED): the caller's distance matrix D [n_rows, n_cols] IS the value matrix of the exact stage
// (kz_exact.h).  No arithmetic touches a value: the two kernels below widen the entries of the listed rows to float64 and write the
// batch vals [nb][index.n] that the selection, the counts and the soft-min consume -- bit for bit the input.
//   rows direction    (query = rows view, index = columns view):  vals[b][j] = (double)D[row_b, j]     a streaming widen-copy
//   columns direction (query = columns view, index = rows view):  vals[b][i] = (double)D[i, col_b]     a 64 x 64 transpose through LDS
// Both move the same bytes per value: the element in, 8 bytes out.  A validation kernel reduces the whole matrix to two integer
// flags once, at creation (NaN / infinity, negative): the selection kernels assume values >= 0 and never NaN.
#include "kz_precomputed.h"

#include <type_traits>

// ---- validation ------------------------------------------------------------------------------------------------------------------
// flags[0] |= a NaN or an infinity was seen, flags[1] |= a value < 0 was seen (-0.0 is not: it compares equal to 0).  Integer
// atomics only; a thread touches the flags once, and only if it saw something.
template <typename T>
__global__ __launch_bounds__(256) void kz_precomputed_check_kernel(const T* __restrict__ D, int64_t count, int* __restrict__ flags) {
    bool nonfinite = false, negative = false;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += stride) {
        const T v = D[e];
        bool fin;
        if (sizeof(T) == 4)
            fin = ((__float_as_uint((float)v) >> 23) & 0xffu) != 0xffu;
        else
            fin = (((unsigned long long)__double_as_longlong((double)v) >> 52) & 0x7ffull) != 0x7ffull;
        nonfinite |= !fin;
        negative |= fin && v < (T)0;
    }
    if (nonfinite) atomicOr(flags, 1);
    if (negative) atomicOr(flags + 1, 1);
}

// ---- rows direction ------------------------------------------------------------------------------------------------------------
// Workgroup (c, b) copies chunk c of row_b = q_begin + fl[batch0 + b]: 256 threads x KZ_PRE_U 16-byte loads in flight.  A row of D
// starts at ANY element (n_cols odd: the starts alternate in alignment), so the chunk is cut as KzRankChunk cuts a value row: up to
// V - 1 scalar elements in front of the first 16-byte aligned one, the vectors, up to V - 1 scalar elements behind them (V = 4
// float32 / 2 float64 elements per load).  The float64 destination is 16-byte aligned at every other element, and which ones is
// uniform over the workgroup (a vector starts an even number of elements behind the first): aligned pairs go out as 16-byte stores.
constexpr int KZ_PRE_U = 4;
__device__ __forceinline__ void kz_pre_store(double* __restrict__ dst, bool pair_aligned, const float4& x) {
    if (pair_aligned) {
        *reinterpret_cast<double2*>(dst) = double2{(double)x.x, (double)x.y};
        *reinterpret_cast<double2*>(dst + 2) = double2{(double)x.z, (double)x.w};
    } else {
        dst[0] = (double)x.x;
        *reinterpret_cast<double2*>(dst + 1) = double2{(double)x.y, (double)x.z};
        dst[3] = (double)x.w;
    }
}
__device__ __forceinline__ void kz_pre_store(double* __restrict__ dst, bool pair_aligned, const double2& x) {
    if (pair_aligned) {
        *reinterpret_cast<double2*>(dst) = x;
    } else {
        dst[0] = x.x;
        dst[1] = x.y;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void kz_precomputed_rows_kernel(const int* __restrict__ fl, int batch0, int64_t q_begin, const T* __restrict__ D,
                                                                  int64_t n_cols, double* __restrict__ vals) {
    using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
    constexpr int V = 16 / sizeof(T);
    constexpr int CHUNK = 256 * KZ_PRE_U * V;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t row = q_begin + fl[batch0 + b];
    const T* __restrict__ src = D + row * n_cols;       // (64-bit element offsets: n_rows x n_cols may pass 2^32)
    double* __restrict__ dst = vals + (int64_t)b * n_cols;
    const int64_t j0 = (int64_t)blockIdx.x * CHUNK;
    const int64_t j1 = j0 + CHUNK < n_cols ? j0 + CHUNK : n_cols;
    // a = the first element at or behind j0 whose address is 16-byte aligned (the matrix itself is aligned to its element size)
    const int mis = (int)((reinterpret_cast<uintptr_t>(src + j0) / sizeof(T)) & (uintptr_t)(V - 1));
    int64_t a = j0 + ((V - mis) & (V - 1));
    if (a > j1) a = j1;
    const int n_vec = (int)((j1 - a) / V);
    const int64_t t0 = a + (int64_t)n_vec * V;   // the scalar elements behind the vectors: [t0, j1)
    const Vec* __restrict__ vecs = reinterpret_cast<const Vec*>(src + a);
    Vec x[KZ_PRE_U];
#pragma unroll
    for (int u = 0; u < KZ_PRE_U; ++u) {
        const int p = tid + 256 * u;
        x[u] = p < n_vec ? vecs[p] : Vec{};
    }
    // the scalar ends: wave 0 the elements in front, wave 1 those behind (at most V - 1 each)
    if (tid < (int)(a - j0))
        dst[j0 + tid] = (double)src[j0 + tid];
    else if (tid >= 64 && tid - 64 < (int)(j1 - t0))
        dst[t0 + tid - 64] = (double)src[t0 + tid - 64];
    const bool pair_aligned = ((reinterpret_cast<uintptr_t>(dst + a) >> 3) & 1u) == 0;
#pragma unroll
    for (int u = 0; u < KZ_PRE_U; ++u) {
        const int p = tid + 256 * u;
        if (p < n_vec) kz_pre_store(dst + a + (int64_t)p * V, pair_aligned, x[u]);
    }
}

// ---- columns direction ---------------------------------------------------------------------------------------------------------
// Workgroup (ti, tb) moves the tile of 64 rows i of D x 64 listed columns b through LDS.  Loads: lanes along b -- wave w, step r
// reads D[i0 + w + 4 r, col_(b0 + lane)]; the listed rows are a run in every caller but kz_gold_ranks' compacted list, so a wave
// reads 64 consecutive elements of a row of D, and a list with holes is still correct (every lane looks its own column up).  Stores:
// lanes along i -- wave w, step r writes vals[b0 + w + 4 r][i0 + lane], 512 consecutive bytes.
// LDS image: float64 s[b][i] with a PITCH OF 65 doubles (64 x 65 x 8 = 33 280 bytes, four workgroups per CU).
//   writes: lane l stores the double at dword 2 (65 l + c), c = w + 4 r.  ds_write_b64 is served in groups of 16 consecutive lanes,
//           bank = dword % 32: the 16 lanes start at banks (130 l + 2 c) % 32 = (2 l + 2 c) % 32 -- 16 distinct even banks, each
//           with its odd neighbour: all 32 banks once.  0 conflicts.  (Pitch 64: 128 l % 32 = 0, every lane of a group on the same
//           two banks -- 16-way.)  The compiler pairs two steps into one ds_write2_b64: two accesses of this same pattern.
//   reads:  lane l loads the double at dword 2 (65 (w + 4 r)) + 2 l.  ds_read_b64 is served per 32-lane half, bank = dword % 64: 32
//           lanes read 64 consecutive dwords -- all 64 banks once, whatever the pitch.  0 conflicts.
// Derived conflict count of the tile: 0 on both sides.
constexpr int KZ_PRE_TILE = 64, KZ_PRE_PITCH = 65;
template <typename T>
__global__ __launch_bounds__(256) void kz_precomputed_cols_kernel(const int* __restrict__ fl, int batch0, int nb, int64_t q_begin,
                                                                  const T* __restrict__ D, int64_t n_rows, int64_t n_cols,
                                                                  double* __restrict__ vals) {
    __shared__ double s[KZ_PRE_TILE * KZ_PRE_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * KZ_PRE_TILE;
    const int b0 = blockIdx.y * KZ_PRE_TILE;
    // (columns past the end of the batch, rows past the end of D: the last one again, nothing is written for them)
    const int bl = b0 + lane < nb ? b0 + lane : nb - 1;
    const int64_t col = q_begin + fl[batch0 + bl];
    T x[KZ_PRE_TILE / 4];
#pragma unroll
    for (int r = 0; r < KZ_PRE_TILE / 4; ++r) {
        const int64_t i = i0 + wave + 4 * r;
        x[r] = D[(i < n_rows ? i : n_rows - 1) * n_cols + col];
    }
#pragma unroll
    for (int r = 0; r < KZ_PRE_TILE / 4; ++r) s[lane * KZ_PRE_PITCH + wave + 4 * r] = (double)x[r];
    __syncthreads();
    const int64_t i = i0 + lane;
#pragma unroll
    for (int r = 0; r < KZ_PRE_TILE / 4; ++r) {
        const int b = b0 + wave + 4 * r;
        if (b < nb && i < n_rows) vals[(int64_t)b * n_rows + i] = s[(wave + 4 * r) * KZ_PRE_PITCH + lane];
    }
}

void kz_precomputed_launch_values(kz_ctx* ctx, const int* fl, int b0, int nb, int64_t q_begin, const kz_matrix* query, const kz_matrix* index,
                                  double* vals) {
    const kz_precomputed* p = query->pre;
    const bool f32 = p->dtype == KZ_F32;
    if (!query->pre_cols) {
        const int chunk = 256 * KZ_PRE_U * (f32 ? 4 : 2);
        const dim3 grid((unsigned)((p->n_cols + chunk - 1) / chunk), (unsigned)nb);
        if (f32)
            hipLaunchKernelGGL(kz_precomputed_rows_kernel<float>, grid, dim3(256), 0, ctx->stream, fl, b0, q_begin, (const float*)p->values, p->n_cols,
                               vals);
        else
            hipLaunchKernelGGL(kz_precomputed_rows_kernel<double>, grid, dim3(256), 0, ctx->stream, fl, b0, q_begin, (const double*)p->values,
                               p->n_cols, vals);
    } else {
        const dim3 grid((unsigned)((p->n_rows + KZ_PRE_TILE - 1) / KZ_PRE_TILE), (unsigned)((nb + KZ_PRE_TILE - 1) / KZ_PRE_TILE));
        if (f32)
            hipLaunchKernelGGL(kz_precomputed_cols_kernel<float>, grid, dim3(256), 0, ctx->stream, fl, b0, nb, q_begin, (const float*)p->values,
                               p->n_rows, p->n_cols, vals);
        else
            hipLaunchKernelGGL(kz_precomputed_cols_kernel<double>, grid, dim3(256), 0, ctx->stream, fl, b0, nb, q_begin, (const double*)p->values,
                               p->n_rows, p->n_cols, vals);
    }
}

int kz_precomputed_check(kz_ctx* ctx, kz_precomputed* p) {
    if (p->checked) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    KZ_HIP(hipMemcpyAsync(ctx->h_counters, p->d_flags, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_counters[0] != 0) {
        kz_set_error("kz_matrix_create_precomputed: the distance matrix contains NaN or infinity");
        return KZ_ERR_NONFINITE;
    }
    if (ctx->h_counters[1] != 0) {
        kz_set_error("Negative values in data passed to precomputed distance matrix.");
        return KZ_ERR_INVALID;
    }
    p->checked = true;
    return KZ_OK;
}

void kz_precomputed_release(kz_matrix* m) {
    kz_precomputed* p = m->pre;
    if (!p) return;
    m->pre = nullptr;
    if (--p->refs > 0) return;
    if (!p->borrowed) kz_pool_free(m->ctx, p->values, 0);
    kz_pool_free(m->ctx, p->d_flags, 0);
    delete p;
}

extern "C" int kz_matrix_create_precomputed(kz_ctx* ctx, const void* values, int values_on_device, int64_t n_rows, int64_t n_cols, int dtype,
                                            kz_matrix** rows_view, kz_matrix** cols_view) {
    KZ_REQUIRE(ctx && values && rows_view && cols_view, "kz_matrix_create_precomputed: null argument");
    KZ_REQUIRE(n_rows > 0 && n_cols > 0, "kz_matrix_create_precomputed: empty matrix (n_rows=%lld, n_cols=%lld)", (long long)n_rows,
               (long long)n_cols);
    const int64_t n_max = ((int64_t)1 << 31) - 256;
    KZ_REQUIRE(n_rows < n_max && n_cols < n_max, "kz_matrix_create_precomputed: n_rows=%lld / n_cols=%lld exceeds the int32 row-id range",
               (long long)n_rows, (long long)n_cols);
    KZ_REQUIRE(dtype == KZ_F32 || dtype == KZ_F64, "kz_matrix_create_precomputed: dtype must be KZ_F32 or KZ_F64");
    KZ_REQUIRE(values_on_device >= 0 && values_on_device <= 2, "kz_matrix_create_precomputed: values_on_device must be 0, 1 or 2");
    const size_t esz = dtype == KZ_F32 ? 4 : 8;
    KZ_REQUIRE((reinterpret_cast<uintptr_t>(values) & (esz - 1)) == 0, "kz_matrix_create_precomputed: values must be aligned to the element size");
    KZ_HIP(hipSetDevice(ctx->device));
    const int64_t count = n_rows * n_cols;
    const size_t bytes = (size_t)count * esz;

    kz_precomputed* p = new kz_precomputed();
    memset(p, 0, sizeof(*p));
    p->n_rows = n_rows;
    p->n_cols = n_cols;
    p->dtype = dtype;
    p->borrowed = values_on_device == 2;
    auto fail = [&](int code) {
        if (!p->borrowed) kz_pool_free(ctx, p->values, 0);
        kz_pool_free(ctx, p->d_flags, 0);
        delete p;
        return code;
    };
    if (p->borrowed) p->values = const_cast<void*>(values);
    if ((!p->borrowed && kz_pool_alloc(ctx, bytes, &p->values) != KZ_OK) || kz_pool_alloc(ctx, 4 * sizeof(int), (void**)&p->d_flags) != KZ_OK) {
        kz_set_error("kz_matrix_create_precomputed: out of device memory (%zu B of values)", bytes);
        return fail(KZ_ERR_NOMEM);
    }
    hipError_t e = hipSuccess;
    if (!p->borrowed)
        e = hipMemcpyAsync(p->values, values, bytes, values_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_flags, 0, 4 * sizeof(int), ctx->stream);
    if (e != hipSuccess) {
        kz_set_error("kz_matrix_create_precomputed: copy failed: %s", hipGetErrorString(e));
        return fail(KZ_ERR_HIP);
    }
    // (a grid-stride reduction: enough workgroups to fill the device, at least 1 024 values each where the matrix has them)
    int64_t blocks = (count + 1023) / 1024;
    const int64_t blocks_max = (int64_t)(ctx->n_cus > 0 ? ctx->n_cus : 256) * 16;
    if (blocks > blocks_max) blocks = blocks_max;
    if (dtype == KZ_F32)
        hipLaunchKernelGGL(kz_precomputed_check_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const float*)p->values, count,
                           p->d_flags);
    else
        hipLaunchKernelGGL(kz_precomputed_check_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const double*)p->values, count,
                           p->d_flags);
    e = hipGetLastError();
    if (e != hipSuccess) {
        kz_set_error("kz_matrix_create_precomputed: validation kernel failed: %s", hipGetErrorString(e));
        return fail(KZ_ERR_HIP);
    }
    // Host values: the copy above was synchronous anyway, the verdict comes from this call (scikit-learn rejects such input in fit).
    // Device values: nothing is waited for; the first search of the pair reads the flags (kz_require_pair).
    if (values_on_device == 0) {
        const int rc = kz_precomputed_check(ctx, p);
        if (rc != KZ_OK) return fail(rc);
    }
    kz_matrix* view[2];
    for (int c = 0; c < 2; ++c) {
        kz_matrix* m = new kz_matrix();
        memset(m, 0, sizeof(*m));
        m->ctx = ctx;
        m->n = c ? n_cols : n_rows;
        m->d = c ? n_rows : n_cols;
        m->dtype = dtype;
        m->metric = KZ_PRECOMPUTED;
        m->mink_p = 2.0;
        m->n_tiles = (m->n + KZ_TILE - 1) / KZ_TILE;
        m->raw = p->values;       // (never read as rows: every entry point that reads embeddings refuses the handle)
        m->raw_borrowed = true;   // (the storage is the shared struct's)
        m->checked = true;        // (no norm kernel ran: the matrix' own verdict is kz_precomputed_check's)
        m->pre = p;
        m->pre_cols = c != 0;
        view[c] = m;
    }
    p->refs = 2;
    *rows_view = view[0];
    *cols_view = view[1];
    return KZ_OK;
}
