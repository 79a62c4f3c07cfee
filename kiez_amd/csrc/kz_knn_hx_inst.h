// Per-list-length translation unit of the parity-split fp16 kernels (kz_knn_hx16.h; 65 .. 128 slices, d = 1025 .. 2048):
// included by kz_knn_hx_kp{16,32,64,128}.hip with KZ_H_KP defined, and by kz_knn_hxd_kp*.hip with KZ_H_DUAL too (the dual-pass
// builds).  Units of their own so that they compile in parallel with the other fp16 units; what a unit exports is its
// kz_sweep_lookup (kz_knn_kernels.h).
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_hx16.h"
#define KZ_SWEEP_UNIT
#include "kz_knn_kernels.h"

#ifdef KZ_H_DUAL
#define KZ_HX_DUALV true
#else
#define KZ_HX_DUALV false
#endif

// One workgroup of the kernel is resident per CU, and a work item is swept by TWO of them (one per half of the item's query
// tile): the planner's slots are half the resident workgroups (kz_h_slots, kz_common.h), a launch starts two per item.
template <bool DUAL>
struct KzSweepBuilds<KZ_SWEEP_HX, DUAL> {
    using Slices = KzSlices<80, 128, 16>;   // (the padded slice counts kz_h_nsr returns beyond 64)
    template <int KP, int NS>
    static KzSweepKernel entry() {
        return {(const void*)kz_knn_cand_hx_kernel<KP, NS, DUAL>, KzHxCfg<KP, DUAL>::LDS_BYTES, 2, 1, KP, NS};
    }
};
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_HX, KZ_HX_DUALV, KZ_H_KP>(int);
