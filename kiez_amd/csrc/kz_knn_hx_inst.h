// Per-list-length translation unit of the parity-split fp16 kernels (kz_knn_hx16.h; 65 .. 128 slices, d = 1025 .. 2048):
// included by kz_knn_hx_kp{16,32,64,128}.hip with KZ_H_KP defined, and by kz_knn_hxd_kp*.hip with KZ_H_DUAL too (the dual-pass
// builds, kz_hxd_* entry points).  Units of their own so that they compile in parallel with the other fp16 units; the entry
// points of kz_knn_h_inst.h forward here beyond 64 slices.
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_hx16.h"

#define KZ_HX_CAT2(a, b) a##b
#define KZ_HX_CAT(a, b) KZ_HX_CAT2(a, b)
#ifdef KZ_H_DUAL
#define KZ_HX_DUALV true
#define KZ_HX_NAME(base) KZ_HX_CAT(kz_hxd_##base##_kp, KZ_H_KP)
#else
#define KZ_HX_DUALV false
#define KZ_HX_NAME(base) KZ_HX_CAT(kz_hx_##base##_kp, KZ_H_KP)
#endif

// *blocks_per_cu = workgroups of the kernel resident per CU (one); the planner's slots are HALF the resident workgroups, because
// a work item is swept by two of them (kz_h_slots, kz_common.h)
template <int KP, int NS>
static int kz_hx_occupancy(int* blocks_per_cu) {
    const void* kern = (const void*)kz_knn_cand_hx_kernel<KP, NS, KZ_HX_DUALV>;
    const int lds = KzHxCfg<KP, KZ_HX_DUALV>::LDS_BYTES;
    KZ_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int nb = 0;
    KZ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, lds));
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return KZ_OK;
}

// n_items work items = 2 n_items workgroups (one per half of an item's query tile)
template <int KP, int NS>
static int kz_launch_hx(kz_ctx* ctx, const KnnCandParams& p, int n_items) {
    KnnCandParams pc = p;
    void* args[] = {&pc};
    KZ_HIP(hipLaunchKernel((const void*)kz_knn_cand_hx_kernel<KP, NS, KZ_HX_DUALV>, dim3(2 * n_items), dim3(256), args,
                           (size_t)KzHxCfg<KP, KZ_HX_DUALV>::LDS_BYTES, ctx->stream));
    return KZ_OK;
}

// (the padded slice counts kz_h_nsr returns beyond 64)
#define KZ_DISPATCH_HX_NSR(rc, fn, args, KPV)             \
    do {                                                  \
        switch (n_slices) {                               \
            case 80: rc = fn<KPV, 80> args; break;        \
            case 96: rc = fn<KPV, 96> args; break;        \
            case 112: rc = fn<KPV, 112> args; break;      \
            case 128: rc = fn<KPV, 128> args; break;      \
            default:                                      \
                kz_set_error("kz_knn: no fp16 kernel for %d slices", n_slices); \
                rc = KZ_ERR_UNSUPPORTED;                  \
        }                                                 \
    } while (0)

int KZ_HX_NAME(occupancy)(int n_slices, int* blocks_per_cu) {
    int rc;
    KZ_DISPATCH_HX_NSR(rc, kz_hx_occupancy, (blocks_per_cu), KZ_H_KP);
    return rc;
}

int KZ_HX_NAME(launch)(int n_slices, kz_ctx* ctx, const KnnCandParams& p, int n_items) {
    int rc;
    KZ_DISPATCH_HX_NSR(rc, kz_launch_hx, (ctx, p, n_items), KZ_H_KP);
    return rc;
}
