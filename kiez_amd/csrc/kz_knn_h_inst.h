// Per-list-length translation unit of the fp16 fused kernels (included by kz_knn_h_kp{16,32,64,128}.hip with KZ_H_KP
// defined): the slice counts of one list length compile in parallel with the other list lengths.  With KZ_H_DUAL
// defined (kz_knn_hd_kp*.hip) the unit holds the dual-pass builds of the same kernels (kz_hd_* entry points).
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_h16.h"

#ifdef KZ_H_DUAL
#define KZ_H_DUALV true
#define KZ_H_NAME(base) KZ_H_CAT(kz_hd_##base##_kp, KZ_H_KP)
#else
#define KZ_H_DUALV false
#define KZ_H_NAME(base) KZ_H_CAT(kz_h_##base##_kp, KZ_H_KP)
#endif
#define KZ_H_CAT2(a, b) a##b
#define KZ_H_CAT(a, b) KZ_H_CAT2(a, b)
// the wide-row builds (32 .. 64 slices) of the same list length: their own translation units (kz_knn_hw_kp*.hip,
// kz_knn_hwd_kp*.hip, KZ_H_WIDE_ROWS defined) so that they compile in parallel with the narrow ones
#ifdef KZ_H_DUAL
#define KZ_HW_NAME(base) KZ_H_CAT(kz_hwd_##base##_kp, KZ_H_KP)
#else
#define KZ_HW_NAME(base) KZ_H_CAT(kz_hw_##base##_kp, KZ_H_KP)
#endif

// Occupancy class of a slice count: three workgroups per CU (168 VGPRs, 53 KiB of LDS each) while the stationary query
// tile fits, two (256 VGPRs, 80 KiB) beyond.
// Measured (MI355X, rocprof): d = 128, K' = 16: 2.93 ms at three per CU against 3.51 ms at two; d = 200, K' = 16 (single
// fragment set, kz_knn_h16.h: ONE_SET): 96.8 against 102.2 ms; d = 200, K' = 64 (lists in the output arrays, 13 spilled
// VGPRs at three per CU): 132 against 127 ms -- so beyond 8 slices only the K' = 16 build runs three per CU.
// Tried and dropped: a long-sweep build at three per CU with an 8-slot ring / one barrier per four slices and the lists in
// the output arrays instead of LDS (same-box A/B on ns: 98.0 against 88.7 ms).
constexpr int KZ_H_WPS3_MAX = 8;        // d <= 128: every list length
constexpr int KZ_H_WPS3_MAX_KP16 = 13;  // d <= 208: K' = 16 only

// (an ordinary `if`: both builds of every slice count are instantiated, as they were while a tuning knob could force two per CU)
template <int KP, int NSR>
static const void* kz_h_kernel_narrow(int* lds) {
    constexpr bool three = NSR <= KZ_H_WPS3_MAX || (KP == 16 && NSR <= KZ_H_WPS3_MAX_KP16);
    if (three) {
        constexpr int N3 = three ? NSR : 2;
        *lds = KzHCfg<KP, 3, NSR, KZ_H_DUALV>::LDS_BYTES;
        return (const void*)kz_knn_cand_h_kernel<KP, N3, 3, KZ_H_DUALV>;
    }
    *lds = KzHCfg<KP, 2, NSR, KZ_H_DUALV>::LDS_BYTES;
    return (const void*)kz_knn_cand_h_kernel<KP, NSR, 2, KZ_H_DUALV>;
}

// WIDE ROWS (d = 497 .. 1024: 32 .. 64 slices, the image zero-padded to a multiple of 8 slices -- kz_h_nsr): ONE workgroup per
// CU, one wave per SIMD.  The stationary query tile alone takes 4 NSR = 128 .. 256 registers a lane; at one wave per SIMD the
// wave owns the SIMD's whole 512-entry register file (VGPRs + AGPRs, kz_knn_h16.h) and the workgroup up to 160 KiB of LDS.
// No co-resident workgroup hides the tile epilogue -- but its cost is fixed while the MFMAs of a tile grow with d (48 slices:
// 3.7x those of d = 200).  Same kernel, same contract, same epilogue; the list modes of two per CU, an eight-slot ring.
template <int KP, int NSR>
static const void* kz_h_kernel(int* lds) {
    if constexpr (NSR > 24) {
        *lds = KzHCfg<KP, 1, NSR, KZ_H_DUALV>::LDS_BYTES;
        return (const void*)kz_knn_cand_h_kernel<KP, NSR, 1, KZ_H_DUALV>;
    } else {
        return kz_h_kernel_narrow<KP, NSR>(lds);
    }
}

// *blocks_per_cu = workgroups of the kernel resident per CU (each takes one query tile)
template <int KP, int NSR>
static int kz_h_occupancy(int* blocks_per_cu) {
    int lds = 0;
    const void* kern = kz_h_kernel<KP, NSR>(&lds);
    KZ_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int nb = 0;
    KZ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, lds));
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return KZ_OK;
}

template <int KP, int NSR>
static int kz_launch_h(kz_ctx* ctx, const KnnCandParams& p, int n_blocks) {
    int lds = 0;
    const void* kern = kz_h_kernel<KP, NSR>(&lds);
    KnnCandParams pc = p;
    void* args[] = {&pc};
    KZ_HIP(hipLaunchKernel(kern, dim3(n_blocks), dim3(256), args, (size_t)lds, ctx->stream));
    return KZ_OK;
}

#define KZ_DISPATCH_H_NSR(rc, fn, args, KPV)              \
    do {                                                  \
        switch (n_slices) {                               \
            case 2: rc = fn<KPV, 2> args; break;          \
            case 3: rc = fn<KPV, 3> args; break;          \
            case 4: rc = fn<KPV, 4> args; break;          \
            case 5: rc = fn<KPV, 5> args; break;          \
            case 6: rc = fn<KPV, 6> args; break;          \
            case 7: rc = fn<KPV, 7> args; break;          \
            case 8: rc = fn<KPV, 8> args; break;          \
            case 9: rc = fn<KPV, 9> args; break;          \
            case 10: rc = fn<KPV, 10> args; break;        \
            case 11: rc = fn<KPV, 11> args; break;        \
            case 12: rc = fn<KPV, 12> args; break;        \
            case 13: rc = fn<KPV, 13> args; break;        \
            case 14: rc = fn<KPV, 14> args; break;        \
            case 15: rc = fn<KPV, 15> args; break;        \
            case 16: rc = fn<KPV, 16> args; break;        \
            case 17: rc = fn<KPV, 17> args; break;        \
            case 18: rc = fn<KPV, 18> args; break;        \
            case 19: rc = fn<KPV, 19> args; break;        \
            case 20: rc = fn<KPV, 20> args; break;        \
            case 21: rc = fn<KPV, 21> args; break;        \
            case 22: rc = fn<KPV, 22> args; break;        \
            case 23: rc = fn<KPV, 23> args; break;        \
            default: rc = fn<KPV, 24> args; break;        \
        }                                                 \
    } while (0)

// (wide rows: the padded slice counts kz_h_nsr returns)
#define KZ_DISPATCH_HW_NSR(rc, fn, args, KPV)             \
    do {                                                  \
        switch (n_slices) {                               \
            case 32: rc = fn<KPV, 32> args; break;        \
            case 40: rc = fn<KPV, 40> args; break;        \
            case 48: rc = fn<KPV, 48> args; break;        \
            case 56: rc = fn<KPV, 56> args; break;        \
            case 64: rc = fn<KPV, 64> args; break;        \
            default:                                      \
                kz_set_error("kz_knn: no fp16 kernel for %d slices", n_slices); \
                rc = KZ_ERR_UNSUPPORTED;                  \
        }                                                 \
    } while (0)

#ifdef KZ_H_WIDE_ROWS
int KZ_HW_NAME(occupancy)(int n_slices, int* blocks_per_cu) {
    int rc;
    KZ_DISPATCH_HW_NSR(rc, kz_h_occupancy, (blocks_per_cu), KZ_H_KP);
    return rc;
}

int KZ_HW_NAME(launch)(int n_slices, kz_ctx* ctx, const KnnCandParams& p, int n_blocks) {
    int rc;
    KZ_DISPATCH_HW_NSR(rc, kz_launch_h, (ctx, p, n_blocks), KZ_H_KP);
    return rc;
}
#else
int KZ_HW_NAME(occupancy)(int n_slices, int* blocks_per_cu);
int KZ_HW_NAME(launch)(int n_slices, kz_ctx* ctx, const KnnCandParams& p, int n_blocks);

// (65 .. 128 slices, d = 1025 .. 2048: the parity-split builds, kz_knn_hx_inst.h -- units of their own as well; two workgroups per
//  work item, one query tile per item)
#ifdef KZ_H_DUAL
#define KZ_HX_FWD(base) KZ_H_CAT(kz_hxd_##base##_kp, KZ_H_KP)
#else
#define KZ_HX_FWD(base) KZ_H_CAT(kz_hx_##base##_kp, KZ_H_KP)
#endif
int KZ_HX_FWD(occupancy)(int n_slices, int* blocks_per_cu);
int KZ_HX_FWD(launch)(int n_slices, kz_ctx* ctx, const KnnCandParams& p, int n_items);

int KZ_H_NAME(occupancy)(int n_slices, int* blocks_per_cu) {
    if (n_slices > 64) return KZ_HX_FWD(occupancy)(n_slices, blocks_per_cu);
    if (n_slices > 24) return KZ_HW_NAME(occupancy)(n_slices, blocks_per_cu);
    int rc;
    KZ_DISPATCH_H_NSR(rc, kz_h_occupancy, (blocks_per_cu), KZ_H_KP);
    return rc;
}

// n_blocks = work items of the plan: one workgroup each, two beyond 64 slices (kz_launch_hx starts 2 n_blocks workgroups)
int KZ_H_NAME(launch)(int n_slices, kz_ctx* ctx, const KnnCandParams& p, int n_blocks) {
    if (n_slices > 64) return KZ_HX_FWD(launch)(n_slices, ctx, p, n_blocks);
    if (n_slices > 24) return KZ_HW_NAME(launch)(n_slices, ctx, p, n_blocks);
    int rc;
    KZ_DISPATCH_H_NSR(rc, kz_launch_h, (ctx, p, n_blocks), KZ_H_KP);
    return rc;
}
#endif
