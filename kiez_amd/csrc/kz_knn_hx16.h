// fp16 first pass for 65 .. 128 slices (d = 1025 .. 2048): the kernel of kz_knn_h16.h with the K dimension SPLIT BETWEEN WAVE
// PAIRS by slice parity.
//
// kz_knn_cand_h_kernel keeps the query tile stationary in registers, 4 per slice for a wave's 32 queries: 64 slices fill the
// unified VGPR + AGPR file of a wave that owns its SIMD, and a 128-query tile of 128 slices (512 KiB of fp16 operands) is the
// whole register file of the CU.  Here a workgroup (4 waves, one per SIMD, one workgroup per CU) owns 64 QUERIES -- one half of a
// query tile; a work item of the plan is swept by TWO workgroups -- and two waves share each group of 32 queries:
//   waves 0, 1  OWNERS of query groups 0, 1: the EVEN slices, the bias, the epilogue, the lists, the event pool;
//   waves 2, 3  HELPERS of the same two groups: the ODD slices, nothing else.
// Each wave holds qf[NS / 2] (40 / 48 / 56 / 64 slices: the register allocation of the wide-row builds).  All four waves step the
// global slice counter, the ring, the slice barriers and the LDS-DMA exactly as kz_knn_cand_h_kernel does (every wave copies its
// quarter of every slice); a wave fetches fragments and issues MFMAs only for the slices of its parity, so its two fragment sets
// alternate between its own consecutive slices g and g + 2.  Same image, same list layout, same epilogue (kz_knn_epi3.h).
//
// EXCHANGE: at the end of a tile a helper stores its 64 partial sums per lane to LDS (16 KiB per helper), ONE workgroup barrier,
// the owner adds them to its own and runs the epilogue; the helper goes straight on to the next tile.  Two buffers, alternating by
// tile: a helper overwrites the buffer of tile t at the end of tile t + 2, behind the exchange barrier of tile t + 1, which the
// owner reaches only after the epilogue of tile t -- whose inputs were that buffer.  The barrier is a raw s_barrier behind
// s_waitcnt lgkmcnt(0) (the helper's stores, everybody's LDS reads), NOT __syncthreads(): its fence would wait vmcnt(0) and drain
// the LDS-DMA copies in flight.  Every wave meets the same barriers: NS / 4 slice barriers + 1 exchange barrier per tile.
//
// ROUNDING: an accumulator is now fl(own chain + helper's chain): one more float32 addition, in an order that is as unspecified
// as the MFMA's internal one already was.  The certification's accumulation term, kz_gamma_acc_h = 2 (d_pad + 16) 2^-24, bounds the
// float32 sum of d_pad exact products + bias in ANY order (any summation tree over n terms errs by at most (n - 1) u sum|terms|,
// doubled for truncating internal adds): two partial chains joined by one addition are one such tree over the same d_pad + 1
// terms, so the bound holds unchanged.  (Padding slices are zero: they add exactly nothing and are not counted.)
#pragma once
#include "kz_knn_epi3.h"
#include "kz_knn_h16.h"

// LDS of a workgroup: the ring (8 slots), bias / merge flags / thresholds as in KzHCfg, event pools of the TWO owner waves, the
// lists (or keys) in the [entry][128] layout of KzListRef with columns 0 .. 63 in use (KzListRef's stride is a constant shared
// with kz_knn_epi3.h: half of the 16 .. 32 KiB block is unused, which the 160 KiB of a lone workgroup can afford), two exchange
// buffers of 2 x 16 KiB.  141 KiB (142.5 KiB dual pass) at K' = 32 and 64, 125 KiB at K' = 16, 109 KiB at K' = 128.
template <int KP, bool DUAL = false>
struct KzHxCfg {
    // where the lists live (KzListRef): the modes of the one-workgroup-per-CU builds of KzHCfg
    static constexpr int LMODE = KP <= 32 ? 1 : (KP == 64 ? 2 : 0);
    static constexpr int RING = 8, PERIOD = 4;
    static constexpr int CAP = 256;                                    // event-pool entries per owner wave (24 B each)
    static constexpr int RING_BYTES = RING * 4096;
    static constexpr int BIAS_OFF = RING_BYTES;                        // 2 x 128 floats
    static constexpr int SYNC_OFF = BIAS_OFF + 1024;                   // 4 merge flags (+ padding)
    static constexpr int THETA_OFF = SYNC_OFF + 256;                   // dual pass: 3 x 64 threshold floats + the queries' offsets
    static constexpr int POOLK_OFF = THETA_OFF + (DUAL ? 768 + 768 : 0);   // [2 owners][CAP] x 4 floats
    static constexpr int POOLM_OFF = POOLK_OFF + 2 * CAP * 16;         // [2 owners][CAP] x {code, next}
    static constexpr int LIST_OFF = POOLM_OFF + 2 * CAP * 8;           // keys [KP][128], then rows [KP][128]
    static constexpr int LIST_BLOCK = LMODE == 1 ? KP * 128 * 8 : (LMODE == 2 ? KP * 128 * 4 : 0);
    static constexpr int XBUF_OFF = LIST_OFF + LIST_BLOCK;             // [2 buffers][2 helpers][16 x 64 lanes] x 4 floats
    static constexpr int XBUF_WAVE = 16 * 64 * 16;
    static constexpr int LDS_BYTES = XBUF_OFF + 4 * XBUF_WAVE;
    static_assert(LDS_BYTES <= 160 * 1024, "workgroup exceeds the CU's LDS");
};

// NS = slices of the image (80 / 96 / 112 / 128: kz_h_nsr).  A launch of W work items is 2 W workgroups.
template <int KP, int NS, bool DUAL = false>
__global__ __launch_bounds__(256, 1) void kz_knn_cand_hx_kernel(KnnCandParams p) {
    using Cfg = KzHxCfg<KP, DUAL>;
    constexpr int NSH = NS / 2;   // slices of one wave
    constexpr int R = Cfg::RING, P = Cfg::PERIOD, CAP = Cfg::CAP;
    static_assert(R == 8 && P == 4, "slot arithmetic below: a ring of two periods of four slices");
    // a multiple of 16 slices: every tile starts at global slice parity 0 and barrier phase 0, and a wave's NS / 2 own slices are an
    // even number -- its fragment sets are in the same state at the start of every tile
    static_assert(NS % 16 == 0 && NS > 64 && NS <= 128, "slice counts of the parity-split builds");
    constexpr int IN_LDS = Cfg::LMODE;   // list storage mode (KzListRef)
    // kz_merge_pool3: block minima re-read per merge instead of carried -- the one build that sits on the 512-register limit (with
    // them carried it spilled one VGPR, an address of the column flush)
    constexpr bool RECOMP = DUAL && KP == 128 && NS == 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ybuf = reinterpret_cast<float*>(smem);                       // R slots x 1024 floats
    float* bbuf = reinterpret_cast<float*>(smem + Cfg::BIAS_OFF);       // 2 x 128 bias floats
    float* tbuf = reinterpret_cast<float*>(smem + Cfg::THETA_OFF);      // dual pass: 3 x 64 thresholds, then -bias of the 64 queries
    kz_lds_i32* msync = (kz_lds_i32*)(smem + Cfg::SYNC_OFF);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const int kh = wave >> 1;                 // slice parity of this wave (uniform): 0 = owner, 1 = helper
    const int grp = wave & 1;                 // its query group (uniform) ...
    const int grp_v = (tid >> 6) & 1;         // ... and the same as a vector value, for per-lane addresses
    // Workgroup -> (work item, half of its query tile).  The work table is in the order kz_plan_fill_work lays out for ONE
    // workgroup per item: workgroups with equal (id % 8) share an XCD and take consecutive items.  Kept: of 16 consecutive
    // workgroups the first 8 take the lower halves of 8 consecutive items, the next 8 the upper halves -- item i runs on the XCD
    // of workgroup i, both halves on the same one (they stream the same index slices through its L2).  The last W % 8 items:
    // two consecutive workgroups each.
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
    const int qt = wd.x, t_begin = wd.y, t_end = wd.z, s = wd.w;
    const int total = (t_end - t_begin) * NS;
    const int qr = 64 * half + 32 * grp_v + j;   // this lane's query row within the tile

    // this query's list in the output arrays (ONE list per query and index range, K' contiguous entries)
    auto out_list_offset = [&]() { return kz_list_contig_off((int64_t)qt * KZ_TILE + qr, p.lay, KP, s); };
    KzCandState3<IN_LDS> st;
    if constexpr (IN_LDS == 1) {
        st.list.k = (kz_lds_f32*)(smem + Cfg::LIST_OFF) + 32 * grp_v + j;
        st.list.i_off = KP * 128;
    } else if constexpr (IN_LDS == 2) {
        st.list.k = (kz_lds_f32*)(smem + Cfg::LIST_OFF) + 32 * grp_v + j;
        st.list.ib = p.out_idx;
        {
            // (uniform: the offsets of this wave's query 0 and of its query 1 -- lists of consecutive queries are equally spaced)
            const int64_t row0 = (int64_t)qt * KZ_TILE + 64 * half + 32 * grp;
            const int64_t o0 = kz_list_contig_off(row0, p.lay, KP, s);
            st.list.off_u = (unsigned)o0;
            st.list.stride = (unsigned)(kz_list_contig_off(row0 + 1, p.lay, KP, s) - o0);
        }
    } else {
        st.list.kb = p.out_key;
        st.list.ib = p.out_idx;
        st.list.off = (unsigned)out_list_offset();
    }
    KzWavePool pool;
    pool.keys = (__attribute__((address_space(3))) f32x4e*)(smem + Cfg::POOLK_OFF) + grp * CAP;
    pool.meta = (__attribute__((address_space(3))) i32x2e*)(smem + Cfg::POOLM_OFF) + grp * CAP;
    // (seeded lists: KnnCandParams::qfloor)
    const float fl = p.qfloor ? p.qfloor[(int64_t)(p.qt0 + qt) * KZ_TILE + qr] : -INFINITY;
    if (h == 0 && kh == 0) {  // the list belongs to the query: lane-half 0 of the owner (kz_merge_logs3)
#pragma unroll 4
        for (int e = 0; e < KP; ++e) {
            st.list.kp()[e * KzListRef<IN_LDS>::KSTRIDE] = fl;
            st.list.ip()[e * KzListRef<IN_LDS>::ISTRIDE] = -1;
        }
    }
    if (total <= 0) {
        if constexpr (IN_LDS != 0) {
            const int64_t listoff = out_list_offset();
            if (h == 0 && kh == 0)
                for (int e = 0; e < KP; ++e) {
                    p.out_key[listoff + e] = -INFINITY;
                    if constexpr (IN_LDS == 1) p.out_idx[listoff + e] = -1;   // (hybrid: the rows were initialised in place above)
                }
        }
        return;
    }
    st.tau = fl;
    KzBlockMin3<KP> bmin;
    bmin.init(fl);
    st.head = -1;
    pool.cnt = 0;
    pool.tiles_done = 0;
    pool.next_merge = 1;

    // LDS-DMA of one 4 KiB slice, as in kz_knn_cand_h_kernel: lane l of wave w copies 16 B from slice base + (64 w + l) * 16 to the
    // same offset of the slot; slices are issued strictly in order, and the ring runs up to R slices past the end of the sweep --
    // into the next tiles of the image or into the padding kz_himage_build allocates behind it (those slots are never used).
    const char* dma_src = reinterpret_cast<const char*>(p.ypack) + ((int64_t)t_begin * NS) * 4096;   // uniform
    int dma_slot = 0;   // uniform: slot of the next slice to issue
    const int lane_off = tid * 16;
    auto dma_next = [&]() {
        float* dst = ybuf + dma_slot * 1024 + wave * 256;  // wave-uniform LDS base (floats)
        kz_glds16_s(dma_src, (unsigned)lane_off, dst);
        dma_src += 4096;
        dma_slot = (dma_slot + 1) & (R - 1);
    };
#pragma unroll
    for (int i = 0; i < R; ++i) dma_next();
    bbuf[(t_begin & 1) * 128 + (tid & 127)] = p.ybias[(int64_t)t_begin * KZ_TILE + (tid & 127)];
    KzDualRef du;
    if constexpr (DUAL) {
        if (tid < 64) tbuf[tid] = p.theta[(int64_t)t_begin * KZ_TILE + tid];
        du.qrow0 = (p.qt0 + qt) * KZ_TILE + 64 * half + 32 * grp;
        // this query's own offset: read back from LDS in every epilogue (kz_knn_cand_h_kernel)
        if (h == 0 && kh == 0) tbuf[192 + 32 * grp_v + j] = p.qnbias[du.qrow0 + j];
    }
    if (tid < 4) msync[tid] = 0;
    // stationary query fragments: lane (j, h) holds k = 16 (2 u + kh) + 8 h + 0..7 of its query row
    const float* qbase = p.qpack + ((int64_t)(p.qt0 + qt) * NS + kh) * 1024 + (h * KZ_TILE + qr) * 4;
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
    int dma_due = 0;   // a barrier has released slots whose copies are still to be issued (uniform; KZ_H_DMA_LATE of kz_knn_h16.h)
    auto fetch_frags = [&](kz_f16x8 (&f)[4], const int gi) {
        const float* fb = fbase + (gi & (R - 1)) * 1024;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) f[mt] = *reinterpret_cast<const kz_f16x8*>(fb + 128 * mt);
    };
    fetch_frags(f0, kh);   // this wave's first slice
    int g = 0;
    int th_cur = 0;   // dual pass: threshold buffer of the current tile (uniform)
    f32x16 acc[4];
    // exchange buffers: 16 groups of four sums per lane, group i of lane l at float4 index 64 i + l (conflict-free ds_*_b128)
    typedef __attribute__((address_space(3))) f32x4e kz_lds_f32x4;

    // (always inlined, as in kz_knn_cand_h_kernel: an out-of-line copy loses the scalar registers the LDS-DMA asm needs)
    auto run_tile = [&](const int tile) __attribute__((always_inline)) {
        if (kh == 0) {
            // (lane half and, below, lane number re-made where they are used: the addresses derived from them, kept in registers
            //  across the tile, were spilled in the K' = 128 dual-pass build of 128 slices -- and reloaded behind a wait for the
            //  whole DMA ring, as kz_knn_cand_h_kernel found at three workgroups per CU)
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
        // bias rows of the next tile by LDS-DMA (waves 0 and 1) and, dual pass, its smallest thresholds (wave 2), issued at the
        // start of this tile: every tile contains a slice barrier behind this point whose vmcnt(0) + s_barrier make them visible
        // before the next tile reads them (kz_knn_cand_h_kernel).  Pinned BEHIND the accumulator init.
        __builtin_amdgcn_sched_barrier(0);
        {
            unsigned off4;
            asm volatile("v_lshrrev_b32 %0, 2, %1" : "=v"(off4) : "v"(lane_off));
            if (wave < 2)
                kz_glds4_s(p.ybias + (int64_t)min(tile + 1, p.n_ytiles - 1) * KZ_TILE, off4, bbuf + ((tile + 1) & 1) * 128 + wave * 64);
            else if (DUAL && wave == 2)
                // (THREE buffers, read at the END of a tile: the one written here was last read two tiles ago)
                kz_glds4_s(p.theta + ((int64_t)min(tile + 1, p.n_ytiles - 1) - 1) * KZ_TILE, off4, tbuf + (th_cur == 2 ? 0 : th_cur + 1) * 64);
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
            // One barrier per P = 4 slices, after the slices g with (g + 3) % 4 == 0 -- ONE SLICE EARLIER in the period than
            // kz_knn_cand_h_kernel's, because a wave reads TWO slices ahead.  When slice g ends, the waves of its parity have
            // fetched slice g + 2 and the other waves slice g + 1 (during slice g - 1); slice g + 2 has g's parity, so nobody else
            // will ever read it.  Every wave that passes the barrier therefore holds, of all slices <= g + 2, the fragments it will
            // ever want: the slots of slices g-1 .. g+2 take slices g+7 .. g+10.  The reads between this barrier and the next
            // (during slices g+1 .. g+4) are of slices g+3 .. g+6: those were issued behind the PREVIOUS barrier (g - 4: slices
            // g+3 .. g+6) and are every wave's youngest copies at this one, hence vmcnt(0) here makes them visible to all.  First
            // period: the prologue's eight slices (0 .. 7) cover the reads before the barrier of slice 1 (slices 0 .. 3) and
            // before that of slice 5 (4 .. 7).  g = u (mod 4) because NS is a multiple of four: the phase is a compile-time one.
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
            float cthr = INFINITY;
            if constexpr (DUAL) {
                int j_now;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_and_b32 %0, 31, %0" : "=v"(j_now));
                cthr = tbuf[192 + 32 * grp + j_now] + tbuf[th_cur * 64];   // this query's offset + the tile's smallest theta
            }
            kz_tile_epilogue3<KP, CAP, IN_LDS, DUAL, RECOMP>(acc, st, pool, bmin, tile, tile == t_end - 1, msync, du, cthr);
        }
        if constexpr (DUAL) th_cur = th_cur == 2 ? 0 : th_cur + 1;
    };

    for (int tile = t_begin; tile < t_end; ++tile) run_tile(tile);
    if constexpr (IN_LDS != 0) {
        // the sweep is over: what lived in LDS goes to the output arrays in the layout kz_knn_finalize_kernel reads
        const int64_t listoff = out_list_offset();
        int lane_now;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_now));
        if (lane_now < 32 && kh == 0) {
#pragma unroll 4
            for (int e = 0; e < KP; ++e) {
                p.out_key[listoff + e] = st.list.kp()[e * 128];
                if constexpr (IN_LDS == 1) p.out_idx[listoff + e] = st.list.ip()[e * 128];
            }
        }
    }
}
