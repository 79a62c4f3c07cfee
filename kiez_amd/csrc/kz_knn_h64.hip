// fp16 fused kernel with 64 queries per wave (kz_knn_h64.h), K' = 16: ordinary and dual-pass builds for 4 .. 13 slices.
#include "kz_common.h"
#include "kz_knn_device.h"
#include "kz_knn_h64.h"
#define KZ_SWEEP_UNIT
#include "kz_knn_kernels.h"

// (slice counts 4 .. 13; a work item = a unit of two query tiles)
template <bool DUAL>
struct KzSweepBuilds<KZ_SWEEP_H64, DUAL> {
    using Slices = KzSlices<4, 13>;
    template <int KP, int NSR>
    static KzSweepKernel entry() {
        static_assert(KP == 16, "the 64-query kernel keeps lists of 16");
        return {(const void*)kz_knn_cand_h64_kernel<NSR, DUAL>, KzH64Cfg<NSR, DUAL>::LDS_BYTES, 1, 2, KP, NSR};
    }
};
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_H64, false, 16>(int);
template KzSweepKernel kz_sweep_lookup<KZ_SWEEP_H64, true, 16>(int);
