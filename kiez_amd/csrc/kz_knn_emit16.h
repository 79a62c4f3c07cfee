// EMIT SWEEP of the fp16 tier (kz_radius_sweep.h: kz_radius_neighbors_sweep): the main loop of kz_knn_count_h_kernel (kz_knn_cnt16.h)
// with an epilogue that EMITS instead of counting.  Every query row of the launch carries an interval [lo, hi] of approximate keys
// (kz_radius_band_kernel: the key of the radius -+ the tier's rounding bound).  Per query the kernel
//   * logs every index row whose key is >= lo -- inside the radius or undecided -- as {query row, index row, key} to a global log,
//     with one bit that says "key above hi": surely inside (the resolve kernel checks that claim on every such entry);
//   * ignores everything below lo -- surely outside.
// Nothing else leaves the kernel: no count register, no per-row counter, no rank atomic.  The LDS of a workgroup is the DMA ring, two
// bias rows and the 128 intervals (18 / 34 KiB), the registers the stationary query tile, the accumulators and one or two fragment
// sets -- KzCntCfg's three occupancy classes, unchanged.
//
// The main loop is a COPY of the count kernel's, not a shared template: the count builds' generated code stays what it was.  4 waves
// x 32 queries, the query tile stationary in qf[NSR], the index image by saddr-form LDS-DMA through a ring of 2 P slots with one
// barrier per P slices, the bias tile by 4-byte LDS-DMA, one v_mfma_f32_32x32x16_f16 per 16 k, the hand-written waits
// (kz_knn_device.h "WAITCNT PASS": the prologue ends in kz_wait_vm0_seen, the epilogue's pointers are address_space(1)).
//
// Epilogue of a tile: a max tree over the lane's 64 keys against the row's lo from LDS; if no lane of the wave reaches its lo the
// tile is done (one ballot: the common case -- a radius admits a few dozen of the index's rows).  Else the wave takes ONE range of the
// log with one atomic (prefix sum of the lanes' entry counts) and every lane writes its entries in accumulator order.  Entries past
// the log's capacity are dropped; the counter still advances, so the host sees the overflow.
// Pad index rows carry bias -inf (kz_pack.hip): below every finite lo.  Pad query rows carry lo = hi = +inf: nothing
// logged.
#pragma once
#include <type_traits>
#include <utility>

#include "kz_knn_cnt16.h"   // KzCntCfg, kz_f16x8, the address_space(1) pointer types

constexpr int KZ_EMIT_ABOVE = (int)0x80000000;   // bit of a log entry's query row: the key was above hi

struct KnnEmitParams {
    const float* qpack;    // fp16 image of the query rows
    const float* ypack;    // fp16 image of the index
    const float* ybias;
    const int4* work;      // {query tile, first index tile, end index tile, range} per workgroup (kz_plan.h)
    int n_ytiles;
    const float2* lohi;    // [query rows incl. padding] {lo, hi}
    unsigned long long* log_cnt;   // entries of the launch (counted also past the log's capacity)
    long long log_cap;
    i32x2e* log_meta;      // [log_cap] {query row | KZ_EMIT_ABOVE, index row}
    float* log_key;        // [log_cap] approximate key
};

// The entries of one tile: the wave reserves sum(nb) log entries with one atomic; a lane writes its nb entries in accumulator order.
// Row of accumulator position (mt, r) of lane half h: tile * 128 + 32 mt + 8 (r >> 2) + 4 h + (r & 3)  (kz_range_group).
__device__ __forceinline__ void kz_emit_entries(const f32x16 (&acc)[4], const float lo, const float hi, const int nb, const int tile, const int qrow,
                                                const KnnEmitParams& p) {
    const int lane = threadIdx.x & 63;
    int incl = nb;   // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
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
                const float v = acc[mt][r];
                if (v >= lo) {
                    if (pos < p.log_cap) {
                        i32x2e mo;
                        mo.x = v > hi ? (qrow | KZ_EMIT_ABOVE) : qrow;
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
__global__ __launch_bounds__(256, WPS) void kz_knn_emit_h_kernel(KnnEmitParams p) {
    using Cfg = KzCntCfg<WPS, NSR>;
    constexpr int R = Cfg::RING, P = Cfg::PERIOD;
    static_assert((R & (R - 1)) == 0 && R == 2 * P, "slot arithmetic below: a power-of-two ring of two periods");
    static_assert(NSR >= 2 && P <= NSR, "every tile must contain a slice barrier (the bias double buffer relies on it)");
    // (the loop's switches are kz_knn_cand_h_kernel's, see there: late copies at two per CU, no fragment carry across the epilogue and
    //  one fragment set beyond 8 slices at three per CU)
    constexpr bool LATE = WPS <= 2;
    constexpr bool CARRY = WPS != 3;
    constexpr bool ONE_SET = WPS == 3 && NSR > 8;
    constexpr int LAG = ONE_SET ? 1 : 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ybuf = reinterpret_cast<float*>(smem);
    float* bbuf = reinterpret_cast<float*>(smem + Cfg::BIAS_OFF);
    float2* lbuf = reinterpret_cast<float2*>(smem + Cfg::LOHI_OFF);
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
    // the intervals of the tile's queries: re-read from LDS in every epilogue (the count kernel's reason: no room beside the
    // stationary query tile at three workgroups per CU)
    if (tid < 128) lbuf[tid] = p.lohi[(int64_t)qt * KZ_TILE + tid];
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
            unsigned off4;
            asm volatile("v_lshrrev_b32 %0, 2, %1" : "=v"(off4) : "v"(lane_off));
            if (wave < 2) kz_glds4_s(p.ybias + (int64_t)min(tile + 1, p.n_ytiles - 1) * KZ_TILE, off4, bbuf + ((tile + 1) & 1) * 128 + wave * 64);
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
        // ---- the emitting epilogue ----
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
        const float2 lh = lbuf[32 * (tid >> 6) + (tid & 31)];
        if (__builtin_amdgcn_ballot_w64(m >= lh.x) != 0ull) {
            int nb = 0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) nb += acc[mt][r] >= lh.x ? 1 : 0;
            }
            kz_emit_entries(acc, lh.x, lh.y, nb, tile, qrow, p);
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

// The builds live in instantiation units beside the count kernel's (kz_knn_emit_lo.hip: 2 .. 13 slices, three workgroups per CU;
// kz_knn_emit_hi.hip: 14 .. 24 slices, two; kz_knn_emit_w.hip: the wide rows, 32 .. 64 slices, one) and come back in the count
// kernel's descriptor: a slice count without a build gets the empty descriptor.
KzCountKernel kz_emit_lookup_lo(int n_slices);
KzCountKernel kz_emit_lookup_hi(int n_slices);
KzCountKernel kz_emit_lookup_w(int n_slices);

template <int WPS, int... NS>
static KzCountKernel kz_emit_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzCountKernel table[] = {{(const void*)kz_knn_emit_h_kernel<NS, WPS>, KzCntCfg<WPS, NS>::LDS_BYTES, NS}...};
    for (const KzCountKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzCountKernel{};
}
