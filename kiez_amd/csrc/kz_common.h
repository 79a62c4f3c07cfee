// Internal definitions shared by the HIP translation units of libkiez_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <type_traits>

#include "../../include/kiez_amd.h"
#include "kz_pool_buf.h"
#include "kz_route.h"

#define KZ_TILE 128   // rows per packed tile (= MFMA block tile edge)
#define KZ_KSLICE 16  // k elements staged per LDS slice (4 k-groups of 4)
#define KZ_LIVE_MAX 1024
#define KZ_POOL_SLOTS 256   // cached released buffers (a shared-sweep fit + kneighbors releases ~90: 64 slots evicted ~28 a step -- hipFree, a device-wide sync each)

// Former context options that no tool or test set (round 6: one table of <= 30 options): the values every build ran with.
// (The on / off switches among them are gone with the branches they guarded; what is left are values.)
constexpr double KZ_K_NESTED_MIN_MS = 2.0;   // the nested sample of the shared sweep is taken when it saves at least this many model-ms (sweep / stride)
constexpr int KZ_K_DUAL_SHORT_KP = 16;   // short-list routes: lists of this length, one per KZ_K_DUAL_SHORT_DIV neighbours (kz_route.h)
constexpr double KZ_K_SPEC_ELEMS = 1.6e9;   // speculative rescue: at most this / (index rows x d) rows (and at most "spec_rows")
constexpr int KZ_K_FLOOR_PROBE = 1024;   // seeded lists: rows of the probe in kz_knn_dual
constexpr double KZ_K_MODEL_MIN_R2 = 0.45;  // model thresholds of the shared sweep: the forward floor fit must explain at least this share of the k-th key's variance, or the reverse probe is not run (kz_knn_dual.h "MODEL THRESHOLDS")

struct kz_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    hipEvent_t ev[12];   // [0..7] work on `stream`, [8..11] the reverse direction of kz_knn_dual on `stream2`
    int stream2_busy;    // kz_knn_dual: the reverse chain is (or is about to be) on stream2 -- nobody else may queue behind it
    hipStream_t stream2; // second stream: kz_knn_dual runs the reverse direction's event chain beside the forward direction's finalize
    double eps_scale;
    int force_splits;
    int chunk_rows;   // test knob: query rows per chunk (0 = default 524288)
    int precision;    // 0: fp16 first pass where eligible (default), 2: split-bf16 first pass, 1: float32 operands only
    int dual_stride;  // kz_knn_dual: every dual_stride-th tile of the query side is in the threshold sample (0: no dual pass, 1: automatic)
    int esc_bf;            // 1 (default): rows the fp16 tier cannot certify with its longest lists go to the split-bf16 operands before the float32 ones
    int short_ord_min_tiles;   // ... when an index range has at least this many tiles (default 48)
    int short_ord;         // 1 (default): the ordinary fp16 kernel takes the short-list route too (a dealt second image of the index)
    int dual_short_main;   // 1 (default): the main sweep of kz_knn_dual keeps k / dual_short_div lists of 16 per query instead of one of 32 / 64; 0: one list of K'
    int dual_rev_long;     // 1 (default): the reverse direction of kz_knn_dual keeps lists of 2 K'
    int dual_short_extra;  // ... of whose entries the finalize kernel selects k + this many (default 48)
    int dual_short_min_tiles;   // ... taken when an index range has at least this many tiles (default 128; test knob)
    int dual_sample_short; // 1 (default): the sample sweep of kz_knn_dual uses lists of 16 (32) over several index ranges whatever K' is; 0: lists of K'
    int dual_overlap; // 1 (default): kz_knn_dual runs the reverse direction's chain on the second stream beside the forward finalize; 0: behind it
    double dual_max_gb; // kz_knn_dual: transient footprint budget in GiB (0 = the built-in 32)
    int dual_force;   // test knob: run the dual pass also where it does not pay (few query rows)
    int h_q64;        // 64-queries-per-wave kernel (kz_knn_h64.h) for K' = 16 sweeps of 4 .. 13 slices: 2 (default) = where it pays (kz_knn_impl), 1 = always, 0 = never
    int fin_fast_div; // finalize kernel, cosine: shared-reciprocal division (kz_div_shared)
    double probe_min_pairs;  // ordinary searches below this many distance pairs take neither the tier probe nor a floor (5e10)
    int list_floor;   // kz_knn_dual: 1 = the forward lists of the shared sweep start at a population floor (kz_knn_dual.h "POPULATION FLOOR")
    int tier_probe;   // rows of the strided sample a large ordinary search sends through the fp16 pass first (0 = off; default 1024): more than half uncertified -> the call starts at split-bf16
    int dual_nested;  // kz_knn_dual: 1 (default) = the sample is the first tiles of the dealt image and is swept ONLY by the sample sweep (kz_knn_dual.h "NESTED")
    int esc_ladder;   // 1 (default): kz_knn.hip "LADDER AFTER THE FACT"
    int exact_rows;   // 1 (default): the exact distance kernel that keeps four query rows in registers and takes 64 / LPR index rows per step
    int abl;          // diagnostics (bit mask): 1 = kz_knn.hip "abl_refloor", 2 = "abl_stamp", 4 / 8 = kz_range.h (overflow / hand-back paths)
    double floor_margin;  // seeded lists: the largest shortfall of the probe below the model, times this (default 1.3; 0 = the model itself: a test knob)
    int dual_rank;    // kz_knn_dual: rank of the sample key that becomes a row's event threshold (0 = automatic, -1 = k + 1, > 0 = that rank; kz_knn_dual.h)
    int spec_rows;    // exact kernels launched speculatively behind every finalize kernel for up to this many uncertified rows (default 64; kz_knn.hip "SPECULATIVE RESCUE")
    int wide_lists;   // fp16 tier's WIDE route (kz_knn_impl): lists of 16 per query when the tier probe finds the keys dense around the k-th neighbour (default 32; 0 = off)
    int wide_sel;     // ... entries of those lists the finalize kernel selects (default 256)
    int dual_model;   // kz_knn_dual: event thresholds from a probe model instead of a sample sweep -- 0 never, 1 (default) where the gate allows, 2 forced (tests; kz_knn_dual.h "MODEL THRESHOLDS")
    double dual_model_shift;   // ... added to the model's thresholds, in the fit's key units (default 0; test knob: a huge value leaves no events at all)
    // scratch (grown on demand, reused across calls)
    void* scratch;
    size_t scratch_bytes;
    float* floor_buf;      // seeded lists of an ordinary search: one float per padded query row (kz_knn.hip "POPULATION FLOOR")
    size_t floor_bytes;
    int* d_counters;  // small device int array (fail counter, flags)
    int* h_counters;  // pinned host mirror
    int n_cus;        // compute units of the device
    void* h_stage;    // pinned host staging for the per-call work table
    size_t h_stage_bytes;
    int h_stage_flip; // which half of h_stage the last pass used (kz_prepare_pass)
    const void* lds_raised[16];   // sweep kernels whose dynamic-LDS limit this context has raised on its device (kz_knn_kernels.h)
    unsigned lds_raised_next;
    // stream-ordered free list: buffers released by kz_free / kz_matrix_destroy are reused by later allocations of a
    // similar size instead of going through hipFree (device-wide sync) + hipMalloc on every fit()
    struct { void* ptr; size_t bytes; } pool[KZ_POOL_SLOTS];
    int pool_n;
    size_t pool_bytes;
    void* live_ptr[KZ_LIVE_MAX];   // capacity of every buffer handed out (so kz_free needs no size)
    size_t live_bytes[KZ_LIVE_MAX];
};

// kz_pool_alloc / kz_pool_free are declared in kz_pool_buf.h (with KzPoolBuf, the scoped owner of a transient buffer)

// Shift and scale shared by the fp16 images of the matrices that are searched against each other (kz_pack.hip):
// distances are translation invariant, so both sides are centred with ONE vector mu (the column mean of the first index
// of the pair) and scaled by ONE power of two S into the fp16 range.  Reference counted: images keep it alive.
// (kz_h_nsr, kz_h_slices_ok -- the slices of the fp16 image and where the fp16 tier exists: kz_route.h)
// Work items the planner may put into one round of an fp16 launch: the resident workgroups -- half of them where two workgroups
// sweep one item (wg_per_item of the kernel's descriptor, kz_knn_kernels.h: the parity-split builds own 64 queries each).
__host__ __forceinline__ int kz_h_slots(int wg_per_item, int blocks_per_cu, int n_cus) {
    const int resident = blocks_per_cu * n_cus;
    return wg_per_item > 1 ? (resident + 1) / 2 : resident;
}

struct kz_center {
    float* d_mu;      // [16 kz_h_nsr(kg)] float32 shift (zero padded)
    double* d_scale;  // device {S, 1 / S^2}
    int refs;
};

// fp16 operand image of a matrix (first pass of the fused kernel, kz_knn_h16.h), built lazily by kz_knn
// Rows dealt over P parts: position r' of a sequence of N rows <- row j, with j running through the parts one after the other,
// part p = rows p, p + P, p + 2 P, ... (the first N % P parts hold one row more).  P = 1: j = r'.
__host__ __device__ __forceinline__ int64_t kz_dealt_row(int64_t rp, int64_t N, int P) {
    const int64_t q = N / P, r = N - q * P;
    int64_t part, i;
    if (rp < r * (q + 1)) {
        part = rp / (q + 1);
        i = rp - part * (q + 1);
    } else {
        const int64_t j2 = rp - r * (q + 1);
        part = r + j2 / q;
        i = j2 - (part - r) * q;
    }
    return part + P * i;
}

struct kz_himage {
    kz_center* center;
    unsigned short* packed;  // [n_tiles][nsr][2 planes][128 rows][8] fp16: plane p = k 8p..8p+7 of the 16-k slice
    float* bias;             // [n_tiles*128] accumulator init -S^2 |x_c|^2 / 2 (pad rows: -inf)
    double* rowq;            // [n][3] unscaled: |x_c|^2, |x_h|, |x_c - x_h|  (x_c = float32(x - mu), x_h = fp16 operand / S)
    double* d_max;           // device [3]: max |x_h|, max |x_c - x_h|, max |x_c|^2 over the rows
    // a second image with the rows DEALT over dealt_P index ranges (kz_himage_dealt; short-list route of the ordinary kernel).
    // dealt_* = the image kz_himage_dealt selected last; TWO are kept (slot): a search and the re-search of its uncertified rows
    // deal the index over different numbers of ranges, and with one buffer every step re-packed the whole index twice (500 k x
    // 200: 0.68 ms each)
    int dealt_P;
    unsigned short* dealt_packed;
    float* dealt_bias;
    int* dealt_perm;         // [n_tiles*128] matrix row of image row r (-1 behind the end)
    struct { int P; unsigned short* packed; float* bias; int* perm; } slot[2];
    int slot_cur;
};

struct kz_matrix {
    kz_ctx* ctx;
    int64_t n, d;
    int dtype, metric;
    double mink_p;    // KZ_MINKOWSKI: the exponent (kz_matrix_set_minkowski_p; 2 by default)
    double* seu_v;    // KZ_SEUCLIDEAN: device [d] per-feature variances (kz_matrix_set_seuclidean_v; NULL until set)
    double* seu_v_host;  // ... and their host copy (the bit-identical check between the two matrices of a search)
    double* corr;     // KZ_CORRELATION: device [n][2] float64 row mean and norm of the centred row (kz_pack.hip: kz_corr_rows_kernel)
    uint32_t* bits;   // the boolean metrics (KZ_JACCARD .. KZ_YULE): device [n][bits_words] uint32, bit j of word w = x[32 w + j] != 0, rows
                      // zero-padded to a multiple of four words (kz_bool.hip: kz_bool_pack_kernel)
    int32_t* bits_cnt;   // ... and device [n] int32: the row's number of true features
    int bits_words;      // ... words per image row (a multiple of 4)
    int64_t n_tiles;  // ceil(n / 128)
    int kg;       // d_pad / 4 (number of 4-wide k-groups), d_pad = round_up(d, 16)
    int kg_bf;        // same for the split-bf16 image (currently equal to kg)
    void* raw;        // [n, d] dtype, row-major (exact data, used by the float64 re-rank)
    bool raw_borrowed;  // raw is the caller's buffer (kz_matrix_create rows_on_device = 2 / 3), not ours to free
    bool raw_only;      // rows_on_device = 3: rows only -- no norms, no operand images: a row SOURCE (kz_dsl_fit), not searchable
    float* packed;    // [n_tiles][kg][128][4] float32 MFMA operand image (NULL until kz_matrix_image_f32)
    unsigned short* packed_bf;  // [n_tiles][kg/4][4 planes][128][8] bf16 split image: planes hi(k 0-7), hi(k 8-15), lo, lo
                                // (NULL until kz_matrix_image_bf)
    float* bias;      // [n_tiles*128] accumulator init: -|y|^2/2 (euclidean family), 0 (cosine), -inf (pad rows)
    double* sqn;      // [n] float64: squared norms (euclidean family) or norms with 0 -> 1 (cosine)
    double max_norm;  // max_j |y_j|  (host copy, valid once `checked`)
    bool checked;     // the norm kernel's verdict (finite input, max_norm) has been read back (kz_matrix_check)
    double* d_stats;  // device [4]: max |y_j| (as max_norm), max |operand element| (normalised rows for cosine)
    kz_himage* himg;  // fp16 image (NULL until a kz_knn call builds it)
    double* norm64;   // cosine, float32 rows: [n][d] float64 rows x / |x| -- the values the re-rank's per-element divisions produce
                      // (NULL until kz_matrix_norm64: built for finalize launches with many candidates per query, kz_knn_fin_wide.h)
    size_t raw_bytes, packed_bytes, bias_bytes, sqn_bytes;
    struct kz_precomputed* pre;   // KZ_PRECOMPUTED: the storage the two views share (kz_precomputed.h); NULL for every embedding matrix.  Such a
                                  // handle owns nothing else: raw points at the shared values (never freed through the handle), no sqn / bias / images
    bool pre_cols;                // ... this handle is the COLUMNS view (n = n_cols, d = n_rows)
};

// operand images are built on first use (kz_pack.hip); all enqueue on the context's stream
int kz_matrix_image_f32(kz_matrix* m);
int kz_matrix_image_bf(kz_matrix* m);
int kz_matrix_norm64(kz_matrix* m);   // KZ_OK also when the image is not built (wrong metric / dtype / shape, or too large): m->norm64 stays NULL
int kz_himage_ensure(kz_matrix* query, kz_matrix* index);
int kz_himage_pack_permuted(kz_matrix* m, const int* d_perm, unsigned short* packed, float* bias);
int kz_himage_pack_rows(kz_matrix* m, const int* d_rows, int64_t n_rows, int64_t n_pad, unsigned short* packed, float* bias);
int kz_himage_dealt(kz_matrix* m, int P);
// stable sort of (float key, int value) pairs on the context's stream (kz_sort.hip)
int kz_sort_pairs_f32_i32(kz_ctx* ctx, const float* keys_in, float* keys_out, const int* vals_in, int* vals_out, int n, int descending);
int kz_matrix_check(kz_matrix* m);
void kz_himage_free(kz_matrix* m);

void kz_set_error(const char* fmt, ...);

// scoped owner of a scratch matrix (the rows of a re-search, kz_matrix_create with rows borrowed on the device)
struct KzMatrixDestroy {
    void operator()(kz_matrix* m) const { kz_matrix_destroy(m); }
};
using KzMatrixPtr = std::unique_ptr<kz_matrix, KzMatrixDestroy>;

#define KZ_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            kz_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return KZ_ERR_HIP;                                                                   \
        }                                                                                        \
    } while (0)

#define KZ_REQUIRE(cond, ...)          \
    do {                               \
        if (!(cond)) {                 \
            kz_set_error(__VA_ARGS__); \
            return KZ_ERR_INVALID;     \
        }                              \
    } while (0)

// what kz_norms_kernel's flag means (KZ_ERR_NONFINITE): a NaN, an infinity, or a row whose squared norm exceeds the input limit
#define KZ_MSG_NONFINITE "kz_matrix_create: input contains NaN, infinity or a row with |x|^2 > 1e30 (the input limit: squared row norms up to 1e30)"

// ---------------------------------------------------------------------------------------------------
// Element types of the raw rows.  float and double are themselves; the two 2-byte STORAGE types (KZ_F16, KZ_BF16) are a bit
// pattern that widens exactly to double wherever a kernel reads `(double)row[k]`: a half matrix behaves like the KZ_F64 matrix
// of the widened values, bit for bit.  They have no arithmetic of their own.
// ---------------------------------------------------------------------------------------------------
struct kz_f16 {
    unsigned short bits;
    __device__ __forceinline__ operator double() const { return (double)__builtin_bit_cast(_Float16, bits); }
};
struct kz_bf16 {
    unsigned short bits;
    __device__ __forceinline__ operator double() const { return (double)__uint_as_float((unsigned)bits << 16); }
};
// scikit-learn's float32 conventions (ArgKmin32, the float32 DistanceMetric) apply to float32 rows ONLY; every other element type
// is on the float64 side.  (Asked by type, never by sizeof: "not 4 bytes" no longer means "8 bytes".)
template <typename T>
constexpr bool kz_f32_rows = std::is_same<T, float>::value;
template <typename T>
constexpr bool kz_half_rows = std::is_same<T, kz_f16>::value || std::is_same<T, kz_bf16>::value;

// bytes per element of a dtype code (0: not an element type)
static inline size_t kz_elem_size(int dtype) {
    switch (dtype) {
        case KZ_F32: return 4;
        case KZ_F64: return 8;
        case KZ_F16:
        case KZ_BF16: return 2;
        default: return 0;
    }
}
static inline bool kz_dtype_is_half(int dtype) { return dtype == KZ_F16 || dtype == KZ_BF16; }
static inline const char* kz_dtype_name(int dtype) {
    switch (dtype) {
        case KZ_F32: return "KZ_F32";
        case KZ_F64: return "KZ_F64";
        case KZ_F16: return "KZ_F16";
        case KZ_BF16: return "KZ_BF16";
        default: return "an unknown element type";
    }
}

// THE dispatch on a matrix' element type: f(KzElem<T>()) with the row type T of `dtype`, KZ_ERR_UNSUPPORTED for a code that is none
// of the four (nothing is launched: no unknown type is ever read as doubles).  f returns an int status (launch errors stay the
// caller's hipGetLastError).
template <typename T>
struct KzElem {
    using type = T;
};
template <typename F>
static inline int kz_dispatch_rows(int dtype, const char* who, F&& f) {
    switch (dtype) {
        case KZ_F32: return f(KzElem<float>());
        case KZ_F64: return f(KzElem<double>());
        case KZ_F16: return f(KzElem<kz_f16>());
        case KZ_BF16: return f(KzElem<kz_bf16>());
        default: kz_set_error("%s: unsupported element type %d", who, dtype); return KZ_ERR_UNSUPPORTED;
    }
}
// The same for kernels that never read raw rows and take T only for the OUTPUT convention (or work on the float64 value matrix):
// float for float32 rows, double -- the float64 semantics -- for float64 and both half types.
template <typename F>
static inline int kz_dispatch_values(int dtype, const char* who, F&& f) {
    switch (dtype) {
        case KZ_F32: return f(KzElem<float>());
        case KZ_F64:
        case KZ_F16:
        case KZ_BF16: return f(KzElem<double>());
        default: kz_set_error("%s: unsupported element type %d", who, dtype); return KZ_ERR_UNSUPPORTED;
    }
}

int kz_scratch(kz_ctx* ctx, size_t bytes, void** out);
int kz_floor_buf(kz_ctx* ctx, size_t bytes, float** out);

// workgroups of 256 threads for a grid-stride kernel over n items: ceil(n / 256) in [1, cap]
static inline int kz_blocks(int64_t n, int cap) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : b < cap ? b : cap);
}

// ---------------------------------------------------------------------------------------------------
// Canonical wave-cooperative float64 dot product.  Every exact distance in the library (row norms, the
// re-rank, the exact fallback) goes through this routine so that |x|^2 + |y|^2 - 2 x.y is EXACTLY 0 for
// x == y and the same pair gives bit-identical values in the forward and the reverse pass.
// All 64 lanes must be active; every lane returns the same value.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double kz_wave_sum(double acc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}

// Order of the canonical dot product: the row is cut into chunks of 256 elements; inside a chunk lane l owns elements
// 4l .. 4l+3 (one 16-byte load for float32 rows), accumulated in increasing k by an fma chain per lane; then the butterfly
// sum.  kz_row4 fetches a lane's four elements of a chunk (vector load when the row allows it, scalar loads with zero fill
// at the tail: the fma of a zero leaves the chain unchanged, so both paths give identical bits).
// The four elements one vector load of a lane brought in (KzRowFrag<T>: 16 bytes of float32, 8 bytes of a 2-byte type), in float64
template <typename T>
using KzRowFrag = typename std::conditional<kz_half_rows<T>, uint2, float4>::type;
template <typename T, typename F>
__device__ __forceinline__ void kz_frag4(const F& v, double (&out)[4]) {
    if constexpr (kz_half_rows<T>) {
        const T e0 = {(unsigned short)(v.x & 0xffffu)}, e1 = {(unsigned short)(v.x >> 16)};
        const T e2 = {(unsigned short)(v.y & 0xffffu)}, e3 = {(unsigned short)(v.y >> 16)};
        out[0] = (double)e0; out[1] = (double)e1; out[2] = (double)e2; out[3] = (double)e3;
    } else {
        out[0] = (double)v.x; out[1] = (double)v.y; out[2] = (double)v.z; out[3] = (double)v.w;
    }
}
template <typename T>
__device__ __forceinline__ void kz_row4(const T* __restrict__ row, int k0, int d, bool vec, double (&out)[4]) {
    if (vec && k0 + 3 < d) {
        if constexpr (kz_f32_rows<T>) {
            const float4 v = *reinterpret_cast<const float4*>(row + k0);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        } else if constexpr (kz_half_rows<T>) {
            // 2-byte elements: ONE 8-byte load of the lane's four elements, widened exactly as the scalar path widens them
            kz_frag4<T>(*reinterpret_cast<const uint2*>(row + k0), out);
        } else {
            static_assert(std::is_same<T, double>::value, "kz_row4: float, double, kz_f16 or kz_bf16 rows");
            const double2 v0 = *reinterpret_cast<const double2*>(row + k0), v1 = *reinterpret_cast<const double2*>(row + k0 + 2);
            out[0] = v0.x; out[1] = v0.y; out[2] = v1.x; out[3] = v1.y;
        }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) out[u] = k0 + u < d ? (double)row[k0 + u] : 0.0;
    }
}
// a row may be read with kz_row4's vector loads when its start and its pitch are aligned to them: 16 bytes (float32, float64), 8 bytes
// for the 2-byte types, whose four elements are one 8-byte load
template <typename T>
__device__ __forceinline__ bool kz_row_vec_ok(const T* base, int d) {
    constexpr uintptr_t mask = kz_half_rows<T> ? 7u : 15u;
    return ((reinterpret_cast<uintptr_t>(base) | ((uintptr_t)d * sizeof(T))) & mask) == 0;
}

template <typename T>
__device__ __forceinline__ double kz_wave_dot(const T* __restrict__ a, const T* __restrict__ b, int d, int lane) {
    const bool vec = kz_row_vec_ok(a, d) && kz_row_vec_ok(b, d);
    double acc = 0.0;
    for (int k0 = 4 * lane; k0 < d; k0 += 256) {
        double x[4], y[4];
        kz_row4(a, k0, d, vec, x);
        kz_row4(b, k0, d, vec, y);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma(x[u], y[u], acc);
    }
    return kz_wave_sum(acc);
}

// a / b for MANY numerators over one divisor, bit for bit the IEEE quotient: rcp = 1.0 / b (correctly rounded, computed once),
// q0 = RN(a rcp) is within 2 ulp of a / b; one residual step makes it faithful (q1 = RN(q0 + (a - b q0) rcp): the value before
// the rounding is within 2^-51 ulp of a / b); for a faithful q1 the residual a - b q1 is exact and RN(q1 + (a - b q1) rcp) is
// the correctly rounded quotient (Markstein, "Computation of elementary functions on the IBM RISC System/6000 processor", 1990,
// theorem on the final step of a division with a correctly rounded reciprocal).  Five multiply-adds against the eleven
// instructions (one of them a quarter-rate reciprocal) of the compiler's division.  Valid while nothing under- or overflows: here
// a is a float32 value or 0 and b the row's norm >= |a| (or 1.0 for a zero row), so |a / b| <= 1 and the residuals stay far
// above the subnormal range; the caller takes the plain division when rcp is not finite (b = 0).  tests/test_gpu_fast_div.py compares the two on
// 2^30 pairs.
__device__ __forceinline__ double kz_div_shared(double a, double b, double rcp) {
    const double q0 = a * rcp;
    const double q1 = fma(fma(-q0, b, a), rcp, q0);
    const double q2 = fma(fma(-q1, b, a), rcp, q1);
    return q2;
}

// cosine: sum_k (a_k / na) * (b_k / nb) with the per-element divisions scikit-learn's normalize() performs
template <typename T>
__device__ __forceinline__ double kz_wave_dot_normalized(const T* __restrict__ a, double na, const T* __restrict__ b,
                                                         double nb, int d, int lane) {
    const bool vec = kz_row_vec_ok(a, d) && kz_row_vec_ok(b, d);
    double acc = 0.0;
    for (int k0 = 4 * lane; k0 < d; k0 += 256) {
        double x[4], y[4];
        kz_row4(a, k0, d, vec, x);
        kz_row4(b, k0, d, vec, y);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma(x[u] / na, y[u] / nb, acc);
    }
    return kz_wave_sum(acc);
}

// numpy's pairwise summation of a contiguous run converted to float64 (numpy/_core/src/umath/loops_utils.h.src,
// DOUBLE_pairwise_sum): < 8 elements sequential, <= 128 eight interleaved accumulators, else split.
template <typename T>
__device__ double kz_np_pairwise_sum(const T* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += (double)a[i];
        return res;
    }
    if (n <= 128) {
        double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
        int i;
        for (i = 8; i < n - (n % 8); i += 8) {
            r0 += (double)a[i + 0];
            r1 += (double)a[i + 1];
            r2 += (double)a[i + 2];
            r3 += (double)a[i + 3];
            r4 += (double)a[i + 4];
            r5 += (double)a[i + 5];
            r6 += (double)a[i + 6];
            r7 += (double)a[i + 7];
        }
        double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += (double)a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return kz_np_pairwise_sum(a, n2) + kz_np_pairwise_sum(a + n2, n - n2);
}

// The exact float64 value the search ranks an index row by (squared euclidean distance / cosine distance): the re-rank of
// kz_knn_finalize_kernel, the exact fallback and kz_pair_values all evaluate THIS expression on the canonical dot product.
// Minkowski family beyond p = 2 (KZ_MANHATTAN, KZ_CHEBYSHEV, KZ_MINKOWSKI): scikit-learn's generic DistanceMetric
// (sklearn/metrics/_dist_metrics.pyx.tp: ManhattanDistance / ChebyshevDistance / MinkowskiDistance): the difference x_j - y_j in
// the INPUT dtype, |.| (to the power p) accumulated in float64 IN FEATURE ORDER, the result -- the ranking value: sum |.|, max |.|,
// sum |.|^p -- rounded to the input dtype.  Every kernel that evaluates the family (the tiled distance kernel of kz_exact.h,
// kz_pair_values) adds the terms of a pair in this order, one thread per pair: manhattan and chebyshev values are scikit-learn's
// bit for bit, minkowski's to the last bit of pow().
// One term.  p_int = 3 or 4 (float32 inputs only, kz_family_p_int): the power as a product with ONE rounding -- a is a float32
// value, so a a is exact in float64 (48 bits) and (a a) a, (a a)(a a) round the exact product once: the correctly rounded a^p, what
// a correctly rounded pow() returns.  Anything else -- float64 inputs, p >= 5, fractional p -- calls pow() as scikit-learn's
// MinkowskiDistance does (a longer chain, or a chain on float64 values, rounds more than once: 1 ulp off in a quarter of the terms).
// CHAIN: -1 = decide at run time from p_int; 3 / 4 = that product, unrolled
template <typename T, int METRIC, int CHAIN = -1>
__device__ __forceinline__ double kz_family_term(T x, T y, double p, int p_int) {
    const T df = x - y;
    const double a = fabs((double)df);
    if (METRIC != KZ_MINKOWSKI) return a;
    if (CHAIN == 3 || (CHAIN < 0 && p_int == 3)) return (a * a) * a;
    if (CHAIN == 4 || (CHAIN < 0 && p_int == 4)) return (a * a) * (a * a);
    return pow(a, p);
}
template <int METRIC>
__device__ __forceinline__ double kz_family_add(double acc, double term) {
    return METRIC == KZ_CHEBYSHEV ? fmax(acc, term) : acc + term;
}
__host__ __device__ __forceinline__ int kz_family_p_int(int metric, double p, bool f32_inputs) {
    return (metric == KZ_MINKOWSKI && f32_inputs && (p == 3.0 || p == 4.0)) ? (int)p : 0;
}

// The per-feature metrics beyond the Minkowski family (KZ_BRAYCURTIS .. KZ_HAMMING) take the same route and the same tiles.  A
// pair's state is two float64 accumulators (a, b); kz_family_step adds feature j of a pair, kz_family_finish turns (a, b) into the
// ranking value.  Every expression is scikit-learn's (tests/metric_restate.py restates them and checks them bit for bit):
//   Minkowski family  a = kz_family_add(a, kz_family_term(x, y))                                          value a (rounded to T)
//   braycurtis        a += |x - y| (difference in T), b += |x| + |y| (float64)   (DistanceMetric)       value a / b, 0 if b == 0 (rounded to T)
//   seuclidean        a += t t / V_j with t = x - y in T (a correctly rounded division; no reciprocal)   value a (rounded to T);
//                     the distance returned is sqrt(a) (kz_output_distance)
//   correlation       x, y are the CENTRED float64 values (x - mean(x), one float64 subtraction, scipy's cdist); even features
//                     into a, odd ones into b: scipy's dot product in two interleaved partial sums, the odd tail term added after
//                     a + b by the caller (kz_family_finish's `tail`); value 1 - clip(dot / (|u| |v|)), NaN (constant row) ranked as
//                     +inf -- the selection kernels order (+inf, row) after every finite value, kz_output_distance turns it back
//   hamming           a += x != y                                                   (scipy's cdist)     value a / d
// kz_family_step's x / y: the input dtype T, except for correlation (the centred float64 values).
template <typename T, int METRIC, int CHAIN = -1, typename S>
__device__ __forceinline__ void kz_family_step(double& a, double& b, S x, S y, double p, int p_int, double v_j, bool odd) {
    if constexpr (METRIC <= KZ_MINKOWSKI) {
        a = kz_family_add<METRIC>(a, kz_family_term<T, METRIC, CHAIN>(x, y, p, p_int));
    } else if constexpr (METRIC == KZ_BRAYCURTIS) {
        const T df = x - y;
        a += fabs((double)df);
        b += fabs((double)x) + fabs((double)y);
    } else if constexpr (METRIC == KZ_SEUCLIDEAN) {
        const T df = x - y;
        const double t = (double)df;
        a += t * t / v_j;
    } else if constexpr (METRIC == KZ_CORRELATION) {
        if (odd)
            b += x * y;
        else
            a += x * y;
    } else {
        a += x != y ? 1.0 : 0.0;
    }
}
// (tail: correlation, odd d -- the product of the centred last features; nx, ny: correlation, the norms of the centred rows)
template <typename T, int METRIC>
__device__ __forceinline__ double kz_family_finish(double a, double b, int d, double tail, double nx, double ny) {
    if constexpr (METRIC == KZ_BRAYCURTIS) {
        const double v = b != 0.0 ? a / b : 0.0;
        return kz_f32_rows<T> ? (double)(float)v : v;
    } else if constexpr (METRIC == KZ_CORRELATION) {
        double s = a + b;
        if (d & 1) s += tail;
        double c = s / (nx * ny);
        if (fabs(c) > 1.0) c = copysign(1.0, c);
        const double v = 1.0 - c;
        return v == v ? v : INFINITY;
    } else if constexpr (METRIC == KZ_HAMMING) {
        return a / (double)d;
    } else {
        return kz_f32_rows<T> ? (double)(float)a : a;
    }
}
// per-search state of the metrics beyond the Minkowski family, for one pair: V (seuclidean), the (mean, centred norm) of both rows
// (correlation)
struct kz_family_pair_args {
    const double* V;
    const double* xc;
    const double* yc;
};
template <typename T, int METRIC>
__device__ __forceinline__ double kz_family_value_seq_m(const T* __restrict__ a, const T* __restrict__ b, int d, double p, int p_int,
                                                        const kz_family_pair_args& ex) {
    double acc = 0.0, acc2 = 0.0;
    if constexpr (METRIC == KZ_CORRELATION) {
        const int de = d & ~1;
        for (int j = 0; j < de; ++j)
            kz_family_step<T, METRIC>(acc, acc2, (double)a[j] - ex.xc[0], (double)b[j] - ex.yc[0], p, p_int, 1.0, (j & 1) != 0);
        const double tail = (d & 1) ? ((double)a[d - 1] - ex.xc[0]) * ((double)b[d - 1] - ex.yc[0]) : 0.0;
        return kz_family_finish<T, METRIC>(acc, acc2, d, tail, ex.xc[1], ex.yc[1]);
    } else {
        for (int j = 0; j < d; ++j)
            kz_family_step<T, METRIC>(acc, acc2, a[j], b[j], p, p_int, METRIC == KZ_SEUCLIDEAN ? ex.V[j] : 1.0, false);
        return kz_family_finish<T, METRIC>(acc, acc2, d, 0.0, 0.0, 0.0);
    }
}
// (one thread, one pair; ex: only the metrics beyond the Minkowski family read it)
template <typename T>
__device__ __forceinline__ double kz_family_value_seq(const T* __restrict__ a, const T* __restrict__ b, int d, int metric, double p,
                                                      const kz_family_pair_args& ex = {nullptr, nullptr, nullptr}) {
    const int p_int = kz_family_p_int(metric, p, kz_f32_rows<T>);
    if (metric == KZ_MANHATTAN) return kz_family_value_seq_m<T, KZ_MANHATTAN>(a, b, d, p, p_int, ex);
    if (metric == KZ_CHEBYSHEV) return kz_family_value_seq_m<T, KZ_CHEBYSHEV>(a, b, d, p, p_int, ex);
    if (metric == KZ_BRAYCURTIS) return kz_family_value_seq_m<T, KZ_BRAYCURTIS>(a, b, d, p, p_int, ex);
    if (metric == KZ_SEUCLIDEAN) return kz_family_value_seq_m<T, KZ_SEUCLIDEAN>(a, b, d, p, p_int, ex);
    if (metric == KZ_CORRELATION) return kz_family_value_seq_m<T, KZ_CORRELATION>(a, b, d, p, p_int, ex);
    if (metric == KZ_HAMMING) return kz_family_value_seq_m<T, KZ_HAMMING>(a, b, d, p, p_int, ex);
    return kz_family_value_seq_m<T, KZ_MINKOWSKI>(a, b, d, p, p_int, ex);
}
// Search-time agreement of the two matrices beyond the metric id: the Minkowski exponent, seuclidean's V (set on both, bit-identical)
static inline bool kz_metric_params_match(const kz_matrix* a, const kz_matrix* b) {
    if (a->metric != b->metric || a->mink_p != b->mink_p) return false;
    if (a->metric != KZ_SEUCLIDEAN) return true;
    return a->seu_v_host && b->seu_v_host && a->d == b->d && memcmp(a->seu_v_host, b->seu_v_host, (size_t)a->d * sizeof(double)) == 0;
}

// The exact float64 value the search ranks an index row by (squared euclidean distance / cosine distance / the Minkowski family's
// reduced distance): the re-rank of kz_knn_finalize_kernel, the exact fallback and kz_pair_values all evaluate THIS expression.
template <typename T>
__device__ __forceinline__ double kz_exact_value(const T* q, const T* y, double qs, double ys, int d, int metric, int lane, double p = 2.0) {
    // (every lane the whole pair: no fused kernel ranks by this metric.  Metrics 6 .. 9 never come here -- their per-search state
    //  travels in kz_family_pair_args: the tiled kernel and kz_pair_values call kz_family_value_seq themselves)
    //  (the 2-byte storage types exist for metrics 0 .. 2 only, kz_matrix_create: they have no arithmetic for the family's differences)
    if constexpr (!kz_half_rows<T>) {
        if (metric >= KZ_MANHATTAN) return kz_family_value_seq<T>(q, y, d, metric, p);
    }
    if (metric == KZ_COSINE) {
        const double sim = kz_wave_dot_normalized(q, qs, y, ys, d, lane);
        double v = 1.0 - sim;  // sklearn cosine_distances: S *= -1; S += 1; clip(0, 2)
        v = fmin(fmax(v, 0.0), 2.0);
        return v;
    }
    const double dot = kz_wave_dot(q, y, d, lane);
    const double d2 = (qs + ys) - 2.0 * dot;  // |x|^2 - 2 x.y + |y|^2 (_argkmin.pyx.tp:494-499)
    return fmax(d2, 0.0);                     // _argkmin.pyx.tp:502
}

