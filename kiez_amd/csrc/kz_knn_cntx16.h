// COUNT / EMIT SWEEP for 65 .. 128 slices (d = 1025 .. 2048): the epilogues of kz_knn_count_h_kernel (kz_knn_cnt16.h) and
// kz_knn_emit_h_kernel (kz_knn_emit16.h) behind a main loop whose K dimension is SPLIT BETWEEN WAVE PAIRS by slice parity -- the
// layout kz_knn_hx16.h proved for the list kernel.  One template, the epilogue chosen by EMIT.
//
// A 128-query tile of 128 slices (512 KiB of fp16 operands) is the whole register file of a CU.  So a workgroup (4 waves, one per
// SIMD, one workgroup per CU) owns 64 QUERIES -- one half of a query tile; a work item of the plan is swept by TWO workgroups -- and
// two waves share each group of 32 queries:
//   waves 0, 1  OWNERS of query groups 0, 1: the EVEN slices, the bias, the epilogue, the count register;
//   waves 2, 3  HELPERS of the same two groups: the ODD slices, nothing else.
// Each wave holds qf[NS / 2] (40 / 48 / 56 / 64 slices: 160 .. 256 registers of the unified VGPR + AGPR file).  All four waves step
// the global slice counter, the ring, the slice barriers and the 16-byte LDS-DMA copies (every wave copies its quarter of every
// slice); a wave fetches fragments and issues v_mfma_f32_32x32x16_f16 only for the slices of its parity, so its two fragment sets
// alternate between its own consecutive slices g and g + 2.  The bias tile arrives by 4-byte LDS-DMA as in the count kernel.
//
// EXCHANGE: at the end of a tile a helper stores its 64 partial sums per lane to LDS (16 KiB per helper), ONE workgroup barrier,
// the owner adds them to its own and runs the epilogue; the helper goes straight on to the next tile.  Two buffers, alternating by
// tile: a helper overwrites the buffer of tile t at the end of tile t + 2, behind the exchange barrier of tile t + 1, which the
// owner reaches only after the epilogue of tile t -- and the owner read that buffer into its accumulators before the epilogue began.
// The barrier is a raw s_barrier behind s_waitcnt lgkmcnt(0) (the helper's stores, everybody's LDS reads), NOT __syncthreads():
// its fence would wait vmcnt(0) and drain the LDS-DMA copies in flight.  Every wave meets the same barriers: NS / 4 slice barriers
// + 1 exchange barrier per tile; the early exit of an empty item is uniform over the workgroup, and a half whose 64 queries are all
// padding walks its barriers like any other (lo = hi = +inf: nothing counted, nothing logged).
//
// LDS of a workgroup: the ring (8 slots, 32 KiB), two bias rows (1 KiB), the 64 {lo, hi} of its queries (512 B), two exchange
// buffers of 2 x 16 KiB: 97.5 KiB.  No lists, no event pool.
//
// EPILOGUE (owners): the count kernel's / the emit kernel's, unchanged in meaning -- a max tree over the lane's 64 keys, one ballot
// against lo, then cnt += key > hi and the band log with one atomic per wave (kz_count_band), or the entry log with the
// KZ_EMIT_ABOVE bit (kz_emit_entries).  The row of accumulator position (mt, r) is the one kz_count_band documents; the query row
// is qt * 128 + 64 half + 32 group + j.  Log writes stay behind pos < log_cap and the counter still advances.  End of an item
// (count): the two lane halves are added with one cross-lane move, one integer atomic per query goes to rank[list[qrow]], guarded
// by qrow < n_list.  Pad index rows carry bias -inf, pad query rows lo = hi = +inf.
//
// ROUNDING: an owner's accumulator is fl(own chain + helper's chain): one more float32 addition, in an order that is as unspecified
// as the MFMA's internal one already was.  The certification's accumulation term, kz_gamma_acc_h = 2 (d_pad + 16) 2^-24, bounds the
// float32 sum of d_pad exact products + bias in ANY order (any summation tree over n terms errs by at most (n - 1) u sum|terms|,
// doubled for truncating internal adds): two partial chains joined by one addition are one such tree over the same d_pad + 1
// terms.  So kz_h_key_eps with kz_gamma_acc_h(index->kg), as kz_rank_band_kernel / kz_radius_band_kernel use it, holds unchanged,
// and the resolve kernels check it on every logged entry (max_err_ratio).  (Padding slices are zero: they add exactly nothing.)
//
// Waits: kz_knn_device.h "WAITCNT PASS" -- the prologue ends in kz_wait_vm0_seen, the epilogue's global pointers are
// address_space(1) (kz_count_band, kz_emit_entries and the rank atomic below).
#pragma once
#include <type_traits>

#include "kz_knn_emit16.h"   // KnnCountParams, KnnEmitParams, both epilogues' log writers, KzCountKernel

struct KzCntxCfg {
    static constexpr int RING = 8, PERIOD = 4;
    static constexpr int RING_BYTES = RING * 4096;
    static constexpr int BIAS_OFF = RING_BYTES;        // 2 x 128 floats
    static constexpr int LOHI_OFF = BIAS_OFF + 1024;   // 64 x {lo, hi}
    static constexpr int XBUF_OFF = LOHI_OFF + 512;    // [2 buffers][2 helpers][16 x 64 lanes] x 4 floats
    static constexpr int XBUF_WAVE = 16 * 64 * 16;
    static constexpr int LDS_BYTES = XBUF_OFF + 4 * XBUF_WAVE;
    static_assert(LDS_BYTES <= 160 * 1024, "workgroup exceeds the CU's LDS");
};

// NS = slices of the image (80 / 96 / 112 / 128: kz_h_nsr).  A launch of W work items is 2 W workgroups.
template <int NS, bool EMIT>
__global__ __launch_bounds__(256, 1) void kz_knn_cntx_h_kernel(std::conditional_t<EMIT, KnnEmitParams, KnnCountParams> p) {
    using Cfg = KzCntxCfg;
    constexpr int NSH = NS / 2;   // slices of one wave
    constexpr int R = Cfg::RING, P = Cfg::PERIOD;
    static_assert(R == 8 && P == 4, "slot arithmetic below: a ring of two periods of four slices");
    // a multiple of 16 slices: every tile starts at global slice parity 0 and barrier phase 0, and a wave's NS / 2 own slices are an
    // even number -- its fragment sets are in the same state at the start of every tile
    static_assert(NS % 16 == 0 && NS > 64 && NS <= 128, "slice counts of the parity-split builds");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ybuf = reinterpret_cast<float*>(smem);                    // R slots x 1024 floats
    float* bbuf = reinterpret_cast<float*>(smem + Cfg::BIAS_OFF);    // 2 x 128 bias floats
    float2* lbuf = reinterpret_cast<float2*>(smem + Cfg::LOHI_OFF);  // the intervals of the workgroup's 64 queries
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const int kh = wave >> 1;            // slice parity of this wave (uniform): 0 = owner, 1 = helper
    const int grp = wave & 1;            // its query group (uniform) ...
    const int grp_v = (tid >> 6) & 1;    // ... and the same as a vector value, for per-lane addresses
    // Workgroup -> (work item, half of its query tile): kz_knn_cand_hx_kernel's mapping.  The work table is in the order
    // kz_plan_fill_work lays out for ONE workgroup per item: workgroups with equal (id % 8) share an XCD and take consecutive items.
    // Kept: of 16 consecutive workgroups the first 8 take the lower halves of 8 consecutive items, the next 8 the upper halves --
    // both halves of an item run on one XCD and stream the same index slices through its L2.  The last W % 8 items: two consecutive
    // workgroups each.
    int item, half;
    {
        const int b = (int)blockIdx.x, full = (int)(gridDim.x >> 1) & ~7;
        if (b < 2 * full) {
            item = ((b >> 4) << 3) | (b & 7);
            half = (b >> 3) & 1;
        } else {
            item = full + ((b - 2 * full) >> 1);
            half = b & 1;
        }
    }
    const int4 wd = p.work[item];
    const int qt = wd.x, t_begin = wd.y, t_end = wd.z;
    if (t_end <= t_begin) return;   // (uniform over the workgroup: nobody is left at a barrier)
    const int qr = 64 * half + 32 * grp_v + j;   // this lane's query row within the tile
    const int qrow = qt * KZ_TILE + qr;

    // LDS-DMA of one 4 KiB slice, as in kz_knn_count_h_kernel: lane l of wave w copies 16 B from slice base + (64 w + l) * 16 to the
    // same offset of the slot; slices are issued strictly in order, and the ring runs up to R slices past the end of the sweep --
    // into the next tiles of the image or into the padding kz_himage_build allocates behind it (those slots are never used).
    const char* dma_src = reinterpret_cast<const char*>(p.ypack) + ((int64_t)t_begin * NS) * 4096;   // uniform
    int dma_slot = 0;   // uniform: slot of the next slice to issue
    const int lane_off = tid * 16;
    auto dma_next = [&]() {
        float* dst = ybuf + dma_slot * 1024 + wave * 256;
        kz_glds16_s(dma_src, (unsigned)lane_off, dst);
        dma_src += 4096;
        dma_slot = (dma_slot + 1) & (R - 1);
    };
#pragma unroll
    for (int i = 0; i < R; ++i) dma_next();
    bbuf[(t_begin & 1) * 128 + (tid & 127)] = p.ybias[(int64_t)t_begin * KZ_TILE + (tid & 127)];
    // the intervals of the workgroup's queries: re-read from LDS in every epilogue, as the count kernel does
    if (tid < 64) lbuf[tid] = p.lohi[(int64_t)qt * KZ_TILE + 64 * half + tid];
    // stationary query fragments: lane (j, h) holds k = 16 (2 u + kh) + 8 h + 0..7 of its query row
    const float* qbase = p.qpack + ((int64_t)qt * NS + kh) * 1024 + (h * KZ_TILE + qr) * 4;
    kz_f16x8 qf[NSH];
#pragma unroll
    for (int u = 0; u < NSH; ++u) qf[u] = *reinterpret_cast<const kz_f16x8*>(qbase + u * 2048);
    // the whole prologue ring must have landed before anyone reads it (the copies are inline asm, invisible to the compiler's barrier);
    // a wait the waitcnt pass sees: the 40 .. 64 query-fragment loads above are complete here (kz_knn_device.h "WAITCNT PASS")
    kz_wait_vm0_seen();
    __syncthreads();

    const float* fbase = ybuf + (h * KZ_TILE + j) * 4;  // this lane's fragment inside a slot: plane h, row j (+ 32 mt)
    // two static fragment sets, alternating between this wave's own consecutive slices (no register copies)
    kz_f16x8 f0[4], f1[4];
    int dma_due = 0;   // a barrier has released slots whose copies are still to be issued (uniform: late copies)
    auto fetch_frags = [&](kz_f16x8 (&f)[4], const int gi) {
        const float* fb = fbase + (gi & (R - 1)) * 1024;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) f[mt] = *reinterpret_cast<const kz_f16x8*>(fb + 128 * mt);
    };
    fetch_frags(f0, kh);   // this wave's first slice
    int g = 0;
    int cnt = 0;   // count sweep, owners: index rows surely closer than the gold row, this lane's keys
    f32x16 acc[4];
    // exchange buffers: 16 groups of four sums per lane, group i of lane l at float4 index 64 i + l (conflict-free ds_*_b128)
    typedef __attribute__((address_space(3))) f32x4e kz_lds_f32x4;

    // (always inlined, as in kz_knn_count_h_kernel: an out-of-line copy loses the scalar registers the LDS-DMA asm needs)
    auto run_tile = [&](const int tile) __attribute__((always_inline)) {
        if (kh == 0) {
            // (lane half re-made where it is used: an address derived from it would otherwise live across the tile)
            int h_now;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshrrev_b32 %0, 5, %0" : "=v"(h_now));
            const float* bp = bbuf + (tile & 1) * 128 + 4 * h_now;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 v = *reinterpret_cast<const float4*>(bp + 32 * mt + 8 * g4);
                    acc[mt][4 * g4 + 0] = v.x;
                    acc[mt][4 * g4 + 1] = v.y;
                    acc[mt][4 * g4 + 2] = v.z;
                    acc[mt][4 * g4 + 3] = v.w;
                }
            }
        } else {
            // (the bias is the owner's: a helper's chain starts at zero)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][i] = 0.0f;
            }
        }
        // bias rows of the next tile by LDS-DMA (waves 0 and 1), issued at the start of this tile: every tile contains a slice
        // barrier behind this point whose vmcnt(0) + s_barrier make them visible before the next tile reads them.  Pinned BEHIND
        // the accumulator init.
        __builtin_amdgcn_sched_barrier(0);
        {
            unsigned off4;
            asm volatile("v_lshrrev_b32 %0, 2, %1" : "=v"(off4) : "v"(lane_off));
            if (wave < 2) kz_glds4_s(p.ybias + (int64_t)min(tile + 1, p.n_ytiles - 1) * KZ_TILE, off4, bbuf + ((tile + 1) & 1) * 128 + wave * 64);
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const bool mine = (u & 1) == kh;            // (uniform)
            const bool set1 = ((u >> 1) & 1) != 0;      // (compile time: which fragment set holds this wave's slice u)
            kz_f16x8 (&cur)[4] = set1 ? f1 : f0;
            // fragments of this wave's NEXT slice, g + 2, under this slice's MFMAs
            __builtin_amdgcn_sched_barrier(0);
            if (mine) {
                if (set1)
                    fetch_frags(f0, g + 2);
                else
                    fetch_frags(f1, g + 2);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (mine) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[mt], qf[u >> 1], acc[mt], 0, 0, 0);
            }
            // (the copies the PREVIOUS slice's barrier released, issued here)
            if (dma_due) {
#pragma unroll
                for (int i = 0; i < P; ++i) dma_next();
                dma_due = 0;
            }
            // One barrier per P = 4 slices, after the slices g with (g + 3) % 4 == 0 -- ONE SLICE EARLIER in the period than the
            // count kernel's, because a wave reads TWO slices ahead (kz_knn_cand_hx_kernel's rule and argument: when slice g ends,
            // the waves of its parity have fetched slice g + 2 and the other waves slice g + 1, so every wave that passes the barrier
            // holds, of all slices <= g + 2, the fragments it will ever want; the slots of slices g-1 .. g+2 take slices g+7 .. g+10,
            // and the reads before the next barrier are of slices g+3 .. g+6, every wave's youngest copies at this one).  g = u
            // (mod 4) because NS is a multiple of four: the phase is a compile-time one.
            if ((u & 3) == 1) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                dma_due = 1;
            }
            ++g;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- exchange: the helper's partial sums to its owner (vector LDS stores; buffer tile & 1, see the header) ----
        int lane_x;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_x));
        kz_lds_f32x4* const xb = (kz_lds_f32x4*)(smem + Cfg::XBUF_OFF) + ((tile & 1) * 2 + grp) * (Cfg::XBUF_WAVE / 16) + lane_x;
        if (kh != 0) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    f32x4e v;
                    v.x = acc[mt][4 * g4 + 0];
                    v.y = acc[mt][4 * g4 + 1];
                    v.z = acc[mt][4 * g4 + 2];
                    v.w = acc[mt][4 * g4 + 3];
                    xb[64 * (4 * mt + g4)] = v;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kh == 0) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4e v = xb[64 * (4 * mt + g4)];
                    acc[mt][4 * g4 + 0] += v.x;
                    acc[mt][4 * g4 + 1] += v.y;
                    acc[mt][4 * g4 + 2] += v.z;
                    acc[mt][4 * g4 + 3] += v.w;
                }
            }
            // ---- the counting / emitting epilogue (kz_knn_count_h_kernel's, kz_knn_emit_h_kernel's) ----
            float m;
            {
                float m4[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const float a = fmaxf(fmaxf(acc[mt][0], acc[mt][1]), fmaxf(acc[mt][2], acc[mt][3]));
                    const float b = fmaxf(fmaxf(acc[mt][4], acc[mt][5]), fmaxf(acc[mt][6], acc[mt][7]));
                    const float c = fmaxf(fmaxf(acc[mt][8], acc[mt][9]), fmaxf(acc[mt][10], acc[mt][11]));
                    const float e = fmaxf(fmaxf(acc[mt][12], acc[mt][13]), fmaxf(acc[mt][14], acc[mt][15]));
                    m4[mt] = fmaxf(fmaxf(a, b), fmaxf(c, e));
                }
                m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
            }
            const float2 lh = lbuf[32 * ((tid >> 6) & 1) + (tid & 31)];
            if (__builtin_amdgcn_ballot_w64(m >= lh.x) != 0ull) {
                if constexpr (EMIT) {
                    int nb = 0;
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) nb += acc[mt][r] >= lh.x ? 1 : 0;
                    }
                    kz_emit_entries(acc, lh.x, lh.y, nb, tile, qrow, p);
                } else {
                    int c = 0, nb = 0;
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = acc[mt][r];
                            c += v > lh.y ? 1 : 0;
                            nb += (v >= lh.x && v <= lh.y) ? 1 : 0;
                        }
                    }
                    cnt += c;
                    if (__builtin_amdgcn_ballot_w64(nb > 0) != 0ull) kz_count_band(acc, lh.x, lh.y, nb, tile, qrow, p);
                }
            }
        }
    };

    for (int tile = t_begin; tile < t_end; ++tile) run_tile(tile);
    if constexpr (!EMIT) {
        // the two lane halves of an owner hold keys of the same query: one cross-lane move, one atomic per query
        cnt += __shfl_xor(cnt, 32, 64);
        int lane_now;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_now));
        if (kh == 0 && lane_now < 32 && cnt > 0 && qrow < p.n_list) {
            kz_cnt_glb_i32* list = (kz_cnt_glb_i32*)p.list;
            kz_cnt_glb_u64* rank = (kz_cnt_glb_u64*)p.rank;
            __hip_atomic_fetch_add(rank + list[qrow], (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The builds live in two instantiation units (kz_knn_cnt_x.hip, kz_knn_emit_x.hip), each exporting the lookup over the padded slice
// counts kz_h_nsr returns beyond 64: a count without a build gets the empty descriptor.
KzCountKernel kz_count_lookup_x(int n_slices);
KzCountKernel kz_emit_lookup_x(int n_slices);

template <bool EMIT, int... NS>
static KzCountKernel kz_cntx_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzCountKernel table[] = {{(const void*)kz_knn_cntx_h_kernel<NS, EMIT>, KzCntxCfg::LDS_BYTES, NS, 2}...};
    for (const KzCountKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzCountKernel{};
}
