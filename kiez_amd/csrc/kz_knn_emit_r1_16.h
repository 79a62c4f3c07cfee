// EMIT SWEEP WITH A RANK-ONE THRESHOLD (kz_knn_reduced_sweep.h: kz_knn_reduced_sweep): the emit sweep of kz_knn_emit16.h for a threshold
// that is not a number per query row but depends on the index row too.  Under a pointwise hubness reduction "w_ij <= tau_i" is a bound
// on the pair's ranking value, v_ij <= P_i + Q_i U_j + V_j (kz_knn_reduced_sweep.h has the forms); in the units of the fp16 tier's key
//     key~_ij + V'_j + Q'_i U_j  >=  P'_i .
// V'_j is FOLDED INTO THE BIAS ROW the sweep adds anyway (a shifted copy of the image's: acc starts from it), Q'_i U_j is one FMA per
// accumulator element, and {P'_i, Q'_i} stand in the per-query LDS slot where the emit kernel keeps {lo, hi}.  The kernel logs every
// pair with fma(Q'_i, U_j, acc) >= P'_i as {query row, index row, t} -- t is the FMA's result, the left-hand side above: the resolve
// step recomputes it from the pair's exact value and checks the rounding bound on every entry.  There is no "above hi" bit: being
// under tau says nothing about being one of the k smallest.
//
// The main loop is a COPY of kz_knn_emit_h_kernel's (which is a copy of the count kernel's, for the reason given there: the existing
// builds' generated code stays what it is): 4 waves x 32 queries, the query tile stationary in qf[NSR], the index image by saddr-form
// LDS-DMA through a ring of 2 P slots with one barrier per P slices, one v_mfma_f32_32x32x16_f16 per 16 k, the hand-written waits
// (kz_knn_device.h "WAITCNT PASS"), kz_plan.h work items unchanged.
//
// NEW DATA MOVEMENT
//   * U tile: 128 floats per index tile, by the same 4-byte LDS-DMA as the bias tile and at the same place -- waves 0 and 1 copy the
//     NEXT tile's bias as before, waves 2 and 3 (idle there until now) copy THIS tile's U.  Two buffers by tile parity.  The copy is
//     issued at the tile's start, is complete at the tile's slice barrier (s_waitcnt vmcnt(0) in front of s_barrier: every tile has
//     one, static_assert below) and is read in the tile's epilogue; buffer (tile & 1) was last read in the epilogue of tile - 2, and
//     the slice barrier of tile - 1 lies between that read and this write.  (Copying the NEXT tile's U as the bias does would be a
//     race: the buffer's last reader is the epilogue of tile - 1, and no barrier separates a wave still in it from one that has begun
//     this tile.)  Read with the bias tile's float4 pattern: the row of acc[mt][r] is the same one.
//   * {P', Q'} per query: 128 float2 in LDS, written in the prologue, re-read in every epilogue (no room for two more registers
//     beside the stationary query tile at three workgroups per CU).
//   * {Umin, Umax} of the tile's real rows: one 8-byte scalar load per tile from a [n_ytiles] array.
// LDS: ring + 2 bias rows + 2 U rows + 128 slots = 19 / 35 KiB (KzR1Cfg).  Occupancy classes as KzCntCfg: slice counts 2 .. 13 (d <= 208)
// run three workgroups per CU -- 2 .. 8 with two fragment sets (114 .. 154 VGPRs), 9 .. 13 with one (132 .. 151) -- and 14 .. 24 (d <= 384)
// two per CU with late copies (178 .. 218 VGPRs); no build spills (tools/spills.py; DESIGN.md section 3.1d has the table).
//
// EPILOGUE.  Cheap reject first: the max tree over the lane's 64 keys, m, and
//     m + max(Q' Umin, Q' Umax)   (+ 2^-22 of the magnitudes)   >=   P'
// -- no row of the tile can pass if that fails (below) -- as one ballot: the common tile costs what the emit kernel's costs plus two
// multiplies, a max and an FMA.  Only where a lane passes does the wave read the U tile, form t = fma(Q', U_j, acc) for its 64 elements,
// count t >= P', take ONE range of the log with one atomic (prefix sum over the lanes) and write its entries in accumulator order;
// entries past the capacity are dropped while the counter advances, so the host sees the overflow (kz_emit_entries' scheme).
// Why the reject is safe: t = fl(Q' U_j + acc_j) >= P' needs Q' U_j + acc_j >= P' (1 - 2^-24 sign-wise), acc_j <= m and
// Q' U_j <= max(Q' Umin, Q' Umax) =: X exactly; the computed fl(fl(X) + m) differs from X + m by at most 2^-23 (|X| + |m|), and
// |X| + |m| >= |P'| (1 - 2^-23) whenever X + m is that close to P'.  The margin 2^-22 (|X| + |m|) is twice what is needed.
// Pad index rows carry bias -inf (t = -inf) and U = 0; pad query rows carry P' = +inf, Q' = 0: the left-hand side is finite (a tile
// has a real row), nothing passes, and no NaN is formed (the unit is built with -fno-honor-nans).
#pragma once
#include <type_traits>
#include <utility>

#include "kz_knn_cnt16.h"   // KzCntCfg, KzCountKernel, kz_f16x8, the address_space(1) pointer types

struct KnnEmitR1Params {
    const float* qpack;    // fp16 image of the query rows
    const float* ypack;    // fp16 image of the index
    const float* ybias;    // [index tiles x 128] the image's bias row + V' (pad rows -inf)
    const float* yu;       // [index tiles x 128] U (pad rows 0)
    const float2* urange;  // [index tiles] {Umin, Umax} over the tile's real rows
    const int4* work;      // {query tile, first index tile, end index tile, range} per workgroup (kz_plan.h)
    int n_ytiles;
    const float2* pq;      // [query rows incl. padding] {P', Q'}
    unsigned long long* log_cnt;   // entries of the launch (counted also past the log's capacity)
    long long log_cap;
    i32x2e* log_meta;      // [log_cap] {query row, index row}
    float* log_key;        // [log_cap] t = fma(Q', U, key~ + V')
};

typedef __attribute__((address_space(4))) float kz_r1_const_f32;

template <int WPS, int NSR>
struct KzR1Cfg {
    static constexpr int RING = KzCntCfg<WPS, NSR>::RING;
    static constexpr int PERIOD = RING / 2;
    static constexpr int BIAS_OFF = RING * 4096;      // 2 x 128 floats
    static constexpr int U_OFF = BIAS_OFF + 1024;     // 2 x 128 floats
    static constexpr int PQ_OFF = U_OFF + 1024;       // 128 x {P', Q'}
    static constexpr int LDS_BYTES = PQ_OFF + 1024;
};

// The entries of one tile: t[] holds the lane's 64 left-hand sides; the wave reserves sum(nb) log entries with one atomic; a lane
// writes its nb entries in accumulator order.  Row of position (mt, r) of lane half h: tile * 128 + 32 mt + 8 (r >> 2) + 4 h + (r & 3).
__device__ __forceinline__ void kz_emit_r1_entries(const f32x16 (&t)[4], const float thr, const int nb, const int tile, const int qrow,
                                                   const KnnEmitR1Params& p) {
    const int lane = threadIdx.x & 63;
    int incl = nb;   // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int s = __shfl_up(incl, off, 64);
        if (lane >= off) incl += s;
    }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    kz_cnt_glb_u64* log_cnt = (kz_cnt_glb_u64*)p.log_cnt;
    unsigned long long base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(log_cnt, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    if (nb > 0) {
        kz_cnt_glb_i32x2* log_meta = (kz_cnt_glb_i32x2*)p.log_meta;
        kz_cnt_glb_f32* log_key = (kz_cnt_glb_f32*)p.log_key;
        long long pos = (long long)base + (incl - nb);
        const int rowbase = tile * KZ_TILE + 4 * (lane >> 5);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = t[mt][r];
                if (v >= thr) {
                    if (pos < p.log_cap) {
                        i32x2e mo;
                        mo.x = qrow;
                        mo.y = rowbase + 32 * mt + 8 * (r >> 2) + (r & 3);
                        log_meta[pos] = mo;
                        log_key[pos] = v;
                    }
                    ++pos;
                }
            }
        }
    }
}

template <int NSR, int WPS>
__global__ __launch_bounds__(256, WPS) void kz_knn_emit_r1_h_kernel(KnnEmitR1Params p) {
    using Cfg = KzR1Cfg<WPS, NSR>;
    constexpr int R = Cfg::RING, P = Cfg::PERIOD;
    static_assert((R & (R - 1)) == 0 && R == 2 * P, "slot arithmetic below: a power-of-two ring of two periods");
    static_assert(NSR >= 2 && P <= NSR, "every tile must contain a slice barrier (the bias and U double buffers rely on it)");
    // (the loop's switches are kz_knn_cand_h_kernel's, see there: late copies at two per CU, no fragment carry across the epilogue and
    //  one fragment set beyond 8 slices at three per CU)
    constexpr bool LATE = WPS <= 2;
    constexpr bool CARRY = WPS != 3;
    constexpr bool ONE_SET = WPS == 3 && NSR > 8;
    constexpr int LAG = ONE_SET ? 1 : 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ybuf = reinterpret_cast<float*>(smem);
    float* bbuf = reinterpret_cast<float*>(smem + Cfg::BIAS_OFF);
    float* ubuf = reinterpret_cast<float*>(smem + Cfg::U_OFF);
    float2* lbuf = reinterpret_cast<float2*>(smem + Cfg::PQ_OFF);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const int4 wd = p.work[blockIdx.x];
    const int t_begin = wd.y, t_end = wd.z;
    const int qt = wd.x;
    if (t_end <= t_begin) return;
    const int wave_v = tid >> 6;
    const int qrow = qt * KZ_TILE + 32 * wave_v + j;

    const char* dma_src = reinterpret_cast<const char*>(p.ypack) + ((int64_t)t_begin * NSR) * 4096;   // uniform
    int dma_slot = 0;
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
    // {P', Q'} of the tile's queries: re-read from LDS in every epilogue
    if (tid < 128) lbuf[tid] = p.pq[(int64_t)qt * KZ_TILE + tid];
    const float* qbase = p.qpack + ((int64_t)qt * NSR) * 1024 + (h * KZ_TILE + 32 * wave_v + j) * 4;
    kz_f16x8 qf[NSR];
#pragma unroll
    for (int u = 0; u < NSR; ++u) qf[u] = *reinterpret_cast<const kz_f16x8*>(qbase + u * 1024);
    kz_wait_vm0_seen();
    __syncthreads();

    const float* fbase = ybuf + (h * KZ_TILE + j) * 4;
    kz_f16x8 f0[4], f1[4];
    int dma_due = 0;
    auto fetch_frags = [&](kz_f16x8 (&f)[4], const int gi) {
        const float* fb = fbase + (gi & (R - 1)) * 1024;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) f[mt] = *reinterpret_cast<const kz_f16x8*>(fb + 128 * mt);
    };
    if (CARRY) fetch_frags(f0, 0);
    int g = 0;
    f32x16 acc[4];

    auto run_tile = [&](const int tile, auto start_parity) __attribute__((always_inline)) {
        constexpr int P0 = decltype(start_parity)::value;
        {
            int h_now = h;
            if constexpr (WPS == 3) {
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshrrev_b32 %0, 5, %0" : "=v"(h_now));
            }
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
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            // waves 0, 1: the next tile's bias (threads 0 .. 127 -> floats 0 .. 127); waves 2, 3: this tile's U (threads 128 .. 255 ->
            // floats 0 .. 127: the base is taken 128 floats back)
            unsigned off4;
            asm volatile("v_lshrrev_b32 %0, 2, %1" : "=v"(off4) : "v"(lane_off));
            if (wave < 2)
                kz_glds4_s(p.ybias + (int64_t)min(tile + 1, p.n_ytiles - 1) * KZ_TILE, off4, bbuf + ((tile + 1) & 1) * 128 + wave * 64);
            else
                kz_glds4_s(reinterpret_cast<const char*>(p.yu) + ((int64_t)tile * KZ_TILE - 128) * 4, off4, ubuf + (tile & 1) * 128 + (wave - 2) * 64);
        }
        constexpr bool carry_in = !ONE_SET && (CARRY || (P0 == 1 && (NSR & 1)));
        constexpr bool carry_out = !ONE_SET && (CARRY || (((P0 + NSR) & 1) != 0));
        if (!carry_in && !ONE_SET) {
            if (P0)
                fetch_frags(f1, g);
            else
                fetch_frags(f0, g);
        }
#pragma unroll
        for (int u = 0; u < NSR; ++u) {
            const bool odd = ((P0 + u) & 1) != 0;
            kz_f16x8 (&cur)[4] = (odd && !ONE_SET) ? f1 : f0;
            __builtin_amdgcn_sched_barrier(0);
            if (ONE_SET) {
                fetch_frags(f0, g);
            } else if (carry_out || u + 1 < NSR) {
                if (odd)
                    fetch_frags(f0, g + 1);
                else
                    fetch_frags(f1, g + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[mt], qf[u], acc[mt], 0, 0, 0);
            if constexpr (LATE) {
                if (dma_due) {
#pragma unroll
                    for (int i = 0; i < P; ++i) dma_next();
                    dma_due = 0;
                }
            }
            // (one barrier per P slices: kz_knn_cand_h_kernel's rule, word for word)
            if ((ONE_SET ? odd : !odd) && (P == 2 || ((g + LAG) & (P - 1)) == 0)) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if constexpr (LATE) {
                    dma_due = 1;
                } else {
#pragma unroll
                    for (int i = 0; i < P; ++i) dma_next();
                }
            }
            ++g;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- the rank-one epilogue ----
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
        const float2 pq = lbuf[32 * (tid >> 6) + (tid & 31)];
        // (uniform, through the constant address space: a SCALAR load -- a vector load would be awaited with vmcnt(0), a wait for the
        //  whole DMA ring in every tile; tools/check_waits.py reports that as a vmcnt finding)
        const kz_r1_const_f32* ur = (const kz_r1_const_f32*)p.urange + 2 * (int64_t)__builtin_amdgcn_readfirstlane(tile);
        const float x = fmaxf(pq.y * ur[0], pq.y * ur[1]);
        const float reach = fmaf(2.384185791015625e-07f /* 2^-22 */, fabsf(x) + fabsf(m), x + m);
        if (__builtin_amdgcn_ballot_w64(reach >= pq.x) != 0ull) {
            int h_now;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshrrev_b32 %0, 5, %0" : "=v"(h_now));
            const float* up = ubuf + (tile & 1) * 128 + 4 * h_now;
            int nb = 0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 u4 = *reinterpret_cast<const float4*>(up + 32 * mt + 8 * g4);
                    acc[mt][4 * g4 + 0] = fmaf(pq.y, u4.x, acc[mt][4 * g4 + 0]);
                    acc[mt][4 * g4 + 1] = fmaf(pq.y, u4.y, acc[mt][4 * g4 + 1]);
                    acc[mt][4 * g4 + 2] = fmaf(pq.y, u4.z, acc[mt][4 * g4 + 2]);
                    acc[mt][4 * g4 + 3] = fmaf(pq.y, u4.w, acc[mt][4 * g4 + 3]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) nb += acc[mt][r] >= pq.x ? 1 : 0;
            }
            if (__builtin_amdgcn_ballot_w64(nb > 0) != 0ull) kz_emit_r1_entries(acc, pq.x, nb, tile, qrow, p);
        }
    };

    int tile = t_begin;
    for (;;) {
        run_tile(tile, std::integral_constant<int, 0>{});
        if (++tile >= t_end) break;
        run_tile(tile, std::integral_constant<int, (NSR & 1)>{});
        if (++tile >= t_end) break;
    }
}

// The builds live in two instantiation units (kz_knn_emit_r1_lo.hip: 2 .. 13 slices, three workgroups per CU; kz_knn_emit_r1_hi.hip:
// 14 .. 24 slices, two) and come back in the count kernel's descriptor: a slice count without a build gets the empty descriptor.
KzCountKernel kz_emit_r1_lookup_lo(int n_slices);
KzCountKernel kz_emit_r1_lookup_hi(int n_slices);

template <int WPS, int... NS>
static KzCountKernel kz_emit_r1_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzCountKernel table[] = {{(const void*)kz_knn_emit_r1_h_kernel<NS, WPS>, KzR1Cfg<WPS, NS>::LDS_BYTES, NS}...};
    for (const KzCountKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzCountKernel{};
}
