// The table of the fused sweep kernels (host side): what a build of one is (KzSweepKernel), which build a call runs
// (kz_sweep_kernel), how many of its workgroups a CU holds (kz_sweep_occupancy) and how it is started (kz_sweep_launch).
// The kernels are instantiated per list length K' in translation units of their own (parallel compilation): kz_knn_h_kp*.hip /
// kz_knn_hd_kp*.hip (fp16, 2 .. 24 slices; d = dual-pass builds), kz_knn_hw*_kp*.hip (wide rows, 32 .. 64 slices),
// kz_knn_hx*_kp*.hip (parity split, 80 .. 128 slices), kz_knn_bf_kp*.hip (split-bf16), kz_knn_h64.hip (64 queries per wave) and
// kz_knn.hip (float32 operands).  Each unit instantiates its kz_sweep_lookup below, a table over the slice counts it is built for.
#pragma once
#include <utility>

#include "kz_knn_device.h"

// Operand precision of the fused kernel ("tier").  kz_knn starts at the highest tier the shapes allow; rows whose
// candidate set cannot be certified under that tier's bound go down: fp16 / split-bf16 -> float32 operands (gathered into
// a dense query block) -> exact float64 brute force.  The result is the float64 neighbour order at every tier.
// (KZ_TIER_F32 / KZ_TIER_BF / KZ_TIER_H: kz_route.h)

struct KzSweepKernel {
    const void* fn;       // host stub of the __global__ (nullptr: no such build)
    int lds_bytes;        // dynamic LDS of a workgroup
    int wg_per_item;      // workgroups that sweep one work item (2: the parity-split builds; else 1)
    int tiles_per_item;   // query tiles per work item (2: the 64-query kernel; else 1)
    int KP, n_slices;     // what the entry was instantiated for -- filled by the same template that takes fn
};

// Slice counts FIRST, FIRST + STEP, .. LAST as a std::integer_sequence
template <int FIRST, int STEP, int... I>
constexpr std::integer_sequence<int, (FIRST + STEP * I)...> kz_slices_of(std::integer_sequence<int, I...>) {
    return {};
}
template <int FIRST, int LAST, int STEP = 1>
using KzSlices = decltype(kz_slices_of<FIRST, STEP>(std::make_integer_sequence<int, (LAST - FIRST) / STEP + 1>{}));

// One lookup per family, dual-pass flag and list length, exported by the unit that holds the builds.
enum { KZ_SWEEP_H, KZ_SWEEP_HW, KZ_SWEEP_HX, KZ_SWEEP_H64, KZ_SWEEP_BF };
template <int FAMILY, bool DUAL, int KP>
KzSweepKernel kz_sweep_lookup(int n_slices);

#ifdef KZ_SWEEP_UNIT
// A unit's side (KZ_SWEEP_UNIT defined in front of this header).  Its instance header specialises KzSweepBuilds for its family --
// Slices, the slice counts it is built for, and entry<KP, NS>(), the descriptor of one build -- and instantiates
// kz_sweep_lookup<family, dual, K'> explicitly.  The table holds entry<KP, NS>() for every NS of the list (this is what
// instantiates the kernels) and is searched by slice count: a count that is not in the list has no build and gets the empty
// descriptor, never a neighbouring entry.
template <int FAMILY, bool DUAL>
struct KzSweepBuilds;

template <class Builds, int KP, int... NS>
KzSweepKernel kz_sweep_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzSweepKernel table[] = {Builds::template entry<KP, NS>()...};
    for (const KzSweepKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzSweepKernel{};
}

template <int FAMILY, bool DUAL, int KP>
KzSweepKernel kz_sweep_lookup(int n_slices) {
    using Builds = KzSweepBuilds<FAMILY, DUAL>;
    return kz_sweep_table<Builds, KP>(n_slices, typename Builds::Slices{});
}
#else
// The callers' side (kz_knn.hip with kz_knn_dual.h).
// float32 operands (defined in kz_knn.hip, beside the kernel): one build per list length, whatever the slice count
KzSweepKernel kz_sweep_f32_kernel(int KP, int n_slices);

template <int FAMILY, bool DUAL>
static KzSweepKernel kz_sweep_lookup_kp(int KP, int n_slices) {
    switch (KP) {
        case 16: return kz_sweep_lookup<FAMILY, DUAL, 16>(n_slices);
        case 32: return kz_sweep_lookup<FAMILY, DUAL, 32>(n_slices);
        case 64: return kz_sweep_lookup<FAMILY, DUAL, 64>(n_slices);
        case 128: return kz_sweep_lookup<FAMILY, DUAL, 128>(n_slices);
    }
    return KzSweepKernel{};
}

// THE RESOLVER: the build that sweeps lists of KP entries over rows of n_slices slices (kz_h_nsr) at `tier`.  The dual-pass
// builds (`dual`) and the 64-query kernel (`q64`) exist in the fp16 tier only; the other tiers have one kernel and ignore both.
// No such build: KZ_ERR_UNSUPPORTED with a message -- or, with may_be_missing (a caller that asks whether a build exists),
// KZ_OK and k->fn == nullptr.
static int kz_sweep_kernel(int tier, bool dual, bool q64, int KP, int n_slices, KzSweepKernel* k, bool may_be_missing = false) {
    KzSweepKernel e{};
    if (tier == KZ_TIER_F32)
        e = kz_sweep_f32_kernel(KP, n_slices);
    else if (tier == KZ_TIER_BF)
        e = kz_sweep_lookup_kp<KZ_SWEEP_BF, false>(KP, n_slices);
    else if (q64)
        e = KP != 16 ? e : dual ? kz_sweep_lookup<KZ_SWEEP_H64, true, 16>(n_slices) : kz_sweep_lookup<KZ_SWEEP_H64, false, 16>(n_slices);
    else if (n_slices > 64)
        e = dual ? kz_sweep_lookup_kp<KZ_SWEEP_HX, true>(KP, n_slices) : kz_sweep_lookup_kp<KZ_SWEEP_HX, false>(KP, n_slices);
    else if (n_slices > 24)
        e = dual ? kz_sweep_lookup_kp<KZ_SWEEP_HW, true>(KP, n_slices) : kz_sweep_lookup_kp<KZ_SWEEP_HW, false>(KP, n_slices);
    else
        e = dual ? kz_sweep_lookup_kp<KZ_SWEEP_H, true>(KP, n_slices) : kz_sweep_lookup_kp<KZ_SWEEP_H, false>(KP, n_slices);
    *k = e;
    if (!e.fn && may_be_missing) return KZ_OK;
    if (!e.fn || e.KP != KP || e.n_slices != n_slices) {
        kz_set_error("kz_knn: no sweep kernel of tier %d%s%s for lists of %d over %d slices", tier, dual ? ", dual pass" : "",
                     q64 ? ", 64 queries per wave" : "", KP, n_slices);
        return KZ_ERR_UNSUPPORTED;
    }
    return KZ_OK;
}

// A workgroup may take more than 64 KiB of dynamic LDS only once the function's limit has been raised on the device.  This is the
// only place that does so, and BOTH the occupancy query and the launch go through it: neither depends on the other having run.
// The context remembers the functions it has raised (a context is one device), so a call pays for it once per kernel.
static int kz_sweep_raise_lds(kz_ctx* ctx, const KzSweepKernel& k) {
    constexpr int N = (int)(sizeof(kz_ctx::lds_raised) / sizeof(kz_ctx::lds_raised[0]));
    if (k.lds_bytes <= 64 * 1024) return KZ_OK;
    for (int i = 0; i < N; ++i)
        if (ctx->lds_raised[i] == k.fn) return KZ_OK;
    KZ_HIP(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes));
    ctx->lds_raised[ctx->lds_raised_next++ % N] = k.fn;   // (full: the oldest entry goes, and is raised again when it comes back)
    return KZ_OK;
}

// *blocks_per_cu = workgroups of the kernel resident per CU
static int kz_sweep_occupancy(kz_ctx* ctx, const KzSweepKernel& k, int* blocks_per_cu) {
    const int rc = kz_sweep_raise_lds(ctx, k);
    if (rc != KZ_OK) return rc;
    int nb = 0;
    KZ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, 256, k.lds_bytes));
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return KZ_OK;
}

// n_items work items of the plan: wg_per_item workgroups each
static int kz_sweep_launch(kz_ctx* ctx, const KzSweepKernel& k, const KnnCandParams& p, int n_items) {
    const int rc = kz_sweep_raise_lds(ctx, k);
    if (rc != KZ_OK) return rc;
    KnnCandParams pc = p;
    void* args[] = {&pc};
    KZ_HIP(hipLaunchKernel(k.fn, dim3(k.wg_per_item * n_items), dim3(256), args, (size_t)k.lds_bytes, ctx->stream));
    return KZ_OK;
}
#endif
