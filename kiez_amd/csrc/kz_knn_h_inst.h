// Per-list-length translation unit of the fp16 fused kernels (included by kz_knn_h_kp{16,32,64,128}.hip with KZ_H_KP
// defined): the slice counts of one list length compile in parallel with the other list lengths.  With KZ_H_DUAL
// defined (kz_knn_hd_kp*.hip) the unit holds the dual-pass builds of the same kernels.  What a unit exports is its
// kz_sweep_lookup (kz_knn_kernels.h).
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_h16.h"
#define KZ_SWEEP_UNIT
#include "kz_knn_kernels.h"

#ifdef KZ_H_DUAL
#define KZ_H_DUALV true
#else
#define KZ_H_DUALV false
#endif
// (the wide-row builds, 32 .. 64 slices, of the same list length: their own translation units -- kz_knn_hw_kp*.hip,
//  kz_knn_hwd_kp*.hip, KZ_H_WIDE_ROWS defined -- so that they compile in parallel with the narrow ones)

// Occupancy class of a slice count: three workgroups per CU (168 VGPRs, 53 KiB of LDS each) while the stationary query
// tile fits, two (256 VGPRs, 80 KiB) beyond.
// Measured (MI355X, rocprof): d = 128, K' = 16: 2.93 ms at three per CU against 3.51 ms at two; d = 200, K' = 16 (single
// fragment set, kz_knn_h16.h: ONE_SET): 96.8 against 102.2 ms; d = 200, K' = 64 (lists in the output arrays, 13 spilled
// VGPRs at three per CU): 132 against 127 ms -- so beyond 8 slices only the K' = 16 build runs three per CU.
// Tried and dropped: a long-sweep build at three per CU with an 8-slot ring / one barrier per four slices and the lists in
// the output arrays instead of LDS (same-box A/B on ns: 98.0 against 88.7 ms).
constexpr int KZ_H_WPS3_MAX = 8;        // d <= 128: every list length
constexpr int KZ_H_WPS3_MAX_KP16 = 13;  // d <= 208: K' = 16 only

template <bool DUAL>
struct KzHEntries {
    // (an ordinary `if`: both builds of every slice count are instantiated, as they were while a tuning knob could force two per CU)
    template <int KP, int NSR>
    static KzSweepKernel narrow() {
        constexpr bool three = NSR <= KZ_H_WPS3_MAX || (KP == 16 && NSR <= KZ_H_WPS3_MAX_KP16);
        if (three) {
            constexpr int N3 = three ? NSR : 2;
            return {(const void*)kz_knn_cand_h_kernel<KP, N3, 3, DUAL>, KzHCfg<KP, 3, NSR, DUAL>::LDS_BYTES, 1, 1, KP, NSR};
        }
        return {(const void*)kz_knn_cand_h_kernel<KP, NSR, 2, DUAL>, KzHCfg<KP, 2, NSR, DUAL>::LDS_BYTES, 1, 1, KP, NSR};
    }

    // WIDE ROWS (d = 497 .. 1024: 32 .. 64 slices, the image zero-padded to a multiple of 8 slices -- kz_h_nsr): ONE workgroup per
    // CU, one wave per SIMD.  The stationary query tile alone takes 4 NSR = 128 .. 256 registers a lane; at one wave per SIMD the
    // wave owns the SIMD's whole 512-entry register file (VGPRs + AGPRs, kz_knn_h16.h) and the workgroup up to 160 KiB of LDS.
    // No co-resident workgroup hides the tile epilogue -- but its cost is fixed while the MFMAs of a tile grow with d (48 slices:
    // 3.7x those of d = 200).  Same kernel, same contract, same epilogue; the list modes of two per CU, an eight-slot ring.
    template <int KP, int NSR>
    static KzSweepKernel entry() {
        if constexpr (NSR > 24)
            return {(const void*)kz_knn_cand_h_kernel<KP, NSR, 1, DUAL>, KzHCfg<KP, 1, NSR, DUAL>::LDS_BYTES, 1, 1, KP, NSR};
        else
            return narrow<KP, NSR>();
    }
};
// (wide rows: the padded slice counts kz_h_nsr returns.  65 .. 128 slices, d = 1025 .. 2048: the parity-split builds,
//  kz_knn_hx_inst.h -- units of their own as well)
template <bool DUAL>
struct KzSweepBuilds<KZ_SWEEP_H, DUAL> : KzHEntries<DUAL> {
    using Slices = KzSlices<2, 24>;
};
template <bool DUAL>
struct KzSweepBuilds<KZ_SWEEP_HW, DUAL> : KzHEntries<DUAL> {
    using Slices = KzSlices<32, 64, 8>;
};

#ifdef KZ_H_WIDE_ROWS
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_HW, KZ_H_DUALV, KZ_H_KP>(int);
#else
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_H, KZ_H_DUALV, KZ_H_KP>(int);
#endif
