// Per-list-length translation unit of the split-bf16 kernels (included by kz_knn_bf_kp{16,32,64,128}.hip with KZ_BF_KP
// defined): the slice counts of one list length compile in parallel with the other list lengths.  What a unit exports is its
// kz_sweep_lookup (kz_knn_kernels.h).
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_bf16.h"
#define KZ_SWEEP_UNIT
#include "kz_knn_kernels.h"

// Largest slice count that still runs the two-workgroups-per-CU kernel (beyond it: one workgroup per CU, overlapped scan)
#ifndef KZ_BF_TWO_WAVE_MAX
#define KZ_BF_TWO_WAVE_MAX 16
#endif
constexpr int KZ_TWM = KZ_BF_TWO_WAVE_MAX;

template <>
struct KzSweepBuilds<KZ_SWEEP_BF, false> {
    using Slices = KzSlices<2, 24>;
    // (both kernels of every slice count are named, as before: the set of builds does not depend on KZ_BF_TWO_WAVE_MAX)
    template <int KP, int NSR>
    static KzSweepKernel entry() {
        const void* two = (const void*)kz_knn_cand_bf_kernel<KP, (NSR <= KZ_TWM ? NSR : KZ_TWM), 2>;
        const void* one = (const void*)kz_knn_cand_bf_ov_kernel<KP, (NSR > KZ_TWM ? NSR : KZ_TWM + 1)>;
        return {NSR <= KZ_TWM ? two : one, NSR <= KZ_TWM ? KZ_BF_LDS : KZ_OV_LDS, 1, 1, KP, NSR};
    }
};
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_BF, false, KZ_BF_KP>(int);
