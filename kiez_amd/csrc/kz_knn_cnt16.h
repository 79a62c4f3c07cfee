// COUNT SWEEP of the fp16 tier (kz_rank_sweep.h: kz_gold_ranks_sweep): the main loop of kz_knn_cand_h_kernel (kz_knn_h16.h) with an
// epilogue that COUNTS instead of selecting.  Every query row of the launch carries an interval [lo, hi] of approximate keys
// (kz_rank_band_kernel: the exact key of its gold row -+ the tier's rounding bound).  Per query the kernel
//   * counts the index rows whose key is above hi -- surely closer than the gold row -- in a lane-private integer;
//   * logs the rows with lo <= key <= hi -- undecided: the BAND -- as {query row, index row, key} to a global log;
//   * ignores everything below lo -- surely farther.
// No lists, no event pool, no merges: the LDS of a workgroup is the DMA ring, two bias rows and the intervals (18 / 34 KiB), the
// registers the stationary query tile, the accumulators and one or two fragment sets.
//
// Main loop: 4 waves x 32 queries, the query tile stationary in qf[NSR], the index image by saddr-form LDS-DMA through a ring of
// 2 P slots with one barrier per P slices, the bias tile by 4-byte LDS-DMA, one v_mfma_f32_32x32x16_f16 per 16 k -- the loop of
// kz_knn_cand_h_kernel in the ring / fragment-set configurations that kernel runs today (KzCntCfg), wait discipline included
// (kz_knn_device.h "WAITCNT PASS": the prologue ends in kz_wait_vm0_seen, the epilogue's pointers are address_space(1)).
//
// Epilogue of a tile: a max tree over the lane's 64 keys; if no lane of the wave reaches its lo the tile is done (one compare: the
// common case wherever gold rows rank well).  Else cnt += (key > hi) over the 64 keys, and where a lane has band keys the wave takes
// ONE range of the log with one atomic (prefix sum of the lanes' band counts), every lane writes its entries and bumps its row's
// band counter.  Entries past the log's capacity are dropped; the counter still advances, so the host sees the overflow.
// End of an item: the two lane halves of a query are added with one cross-lane move and ONE integer atomic per query goes to the
// row's rank entry -- several index ranges of a query add into it, in any order.
// Pad index rows carry bias -inf (kz_pack.hip): below every finite lo.  Pad query rows carry lo = hi = +inf: nothing counted, nothing
// logged.
#pragma once
#include <type_traits>
#include <utility>

#include "kz_knn_device.h"

typedef _Float16 kz_f16x8 __attribute__((ext_vector_type(8)));

struct KnnCountParams {
    const float* qpack;    // fp16 image of the listed query rows
    const float* ypack;    // fp16 image of the index
    const float* ybias;
    const int4* work;      // {query tile, first index tile, end index tile, range} per workgroup (kz_plan.h)
    int n_ytiles;
    const float2* lohi;    // [query rows incl. padding] {lo, hi}
    const int* list;       // [n_list] listed row -> row of the rank vector
    int n_list;
    long long* rank;       // the caller's rank vector: += surely-closer count of listed row r at rank[list[r]]
    int* band_cnt;         // [query rows incl. padding] band entries per listed row (counted also past the log's capacity)
    unsigned long long* log_cnt;   // band entries of the launch
    long long log_cap;
    i32x2e* log_meta;      // [log_cap] {listed row, index row}
    float* log_key;        // [log_cap] approximate key
};

// Occupancy classes.  Three workgroups per CU (168 VGPRs) up to 13 slices -- every width the list kernel runs three per CU at any
// list length -- two beyond; the ring and fragment-set configuration of a class is the list kernel's for that class.
constexpr int KZ_CNT_WPS3_MAX = 13;
template <int WPS, int NSR>
struct KzCntCfg {
    static constexpr int RING = (WPS == 3 || NSR < 4) ? 4 : 8;
    static constexpr int PERIOD = RING / 2;
    static constexpr int RING_BYTES = RING * 4096;
    static constexpr int BIAS_OFF = RING_BYTES;        // 2 x 128 floats
    static constexpr int LOHI_OFF = BIAS_OFF + 1024;   // 128 x {lo, hi}
    static constexpr int LDS_BYTES = LOHI_OFF + 1024;
};

typedef __attribute__((address_space(1))) unsigned long long kz_cnt_glb_u64;
typedef __attribute__((address_space(1))) int kz_cnt_glb_i32;
typedef __attribute__((address_space(1))) i32x2e kz_cnt_glb_i32x2;
typedef __attribute__((address_space(1))) float kz_cnt_glb_f32;

// The band of one tile: the wave reserves sum(nb) log entries with one atomic; a lane writes its nb entries in accumulator order.
// Row of accumulator position (mt, r) of lane half h: tile * 128 + 32 mt + 8 (r >> 2) + 4 h + (r & 3)  (kz_range_group).
__device__ __forceinline__ void kz_count_band(const f32x16 (&acc)[4], const float lo, const float hi, const int nb, const int tile, const int qrow,
                                              const KnnCountParams& p) {
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
        __hip_atomic_fetch_add((kz_cnt_glb_i32*)p.band_cnt + qrow, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long pos = (long long)base + (incl - nb);
        const int rowbase = tile * KZ_TILE + 4 * (lane >> 5);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[mt][r];
                if (v >= lo && v <= hi) {
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
__global__ __launch_bounds__(256, WPS) void kz_knn_count_h_kernel(KnnCountParams p) {
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
    // the intervals of the tile's queries: re-read from LDS in every epilogue (two registers held across the sweep are what the
    // stationary query tile has no room for at three workgroups per CU -- the dual build's tbuf[192 + ...] for the same reason)
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
    int cnt = 0;   // index rows surely closer than the gold row, this lane's keys
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
        // ---- the counting epilogue ----
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
            int c = 0, nb = 0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[mt][r];
                    c += v > lh.y ? 1 : 0;
                    nb += (v >= lh.x && v <= lh.y) ? 1 : 0;
                }
                // (one workgroup per CU: with the whole register file to itself the scheduler issues the compares of all 64 keys ahead
                //  of the serial add chain, their masks fill the scalar registers and 19 .. 21 kernel arguments and lane masks are
                //  spilled to make room.  The two sums are pinned after every accumulator: 16 masks at a time.  Folds away at WPS >= 2)
                if constexpr (WPS == 1) {
                    asm volatile("" : "+v"(c), "+v"(nb));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            cnt += c;
            if (__builtin_amdgcn_ballot_w64(nb > 0) != 0ull) kz_count_band(acc, lh.x, lh.y, nb, tile, qrow, p);
        }
    };

    int tile = t_begin;
    for (;;) {
        run_tile(tile, std::integral_constant<int, 0>{});
        if (++tile >= t_end) break;
        run_tile(tile, std::integral_constant<int, (NSR & 1)>{});
        if (++tile >= t_end) break;
    }
    // the two lane halves hold keys of the same query: one cross-lane move, one atomic per query
    cnt += __shfl_xor(cnt, 32, 64);
    int lane_now;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_now));
    if (lane_now < 32 && cnt > 0 && qrow < p.n_list) {
        kz_cnt_glb_i32* list = (kz_cnt_glb_i32*)p.list;
        kz_cnt_glb_u64* rank = (kz_cnt_glb_u64*)p.rank;
        __hip_atomic_fetch_add(rank + list[qrow], (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// What the host needs of a build.  The builds live in instantiation units of their own (kz_knn_cnt_lo.hip: 2 .. 13 slices, three
// workgroups per CU; kz_knn_cnt_hi.hip: 14 .. 24 slices, two; kz_knn_cnt_w.hip: the WIDE ROWS, 32 .. 64 slices in steps of 8 -- one
// workgroup per CU, one wave per SIMD, the stationary query tile qf[NSR] of 128 .. 256 registers in the unified VGPR + AGPR file,
// as kz_knn_h_inst.h "WIDE ROWS"; KzCntCfg<1, NSR> is the eight-slot ring, and the loop's switches at WPS = 1 are the list
// kernel's: late copies, fragment carry, two fragment sets), each exporting the lookup over its slice counts: a count without a
// build gets the empty descriptor, never a neighbouring entry.  (80 .. 128 slices: kz_knn_cntx16.h.)
struct KzCountKernel {
    const void* fn;   // nullptr: no build for this slice count
    int lds_bytes;
    int n_slices;
    int wg_per_item = 1;   // workgroups that sweep one work item (2: the parity-split builds, kz_knn_cntx16.h)
};
KzCountKernel kz_count_lookup_lo(int n_slices);
KzCountKernel kz_count_lookup_hi(int n_slices);
KzCountKernel kz_count_lookup_w(int n_slices);

template <int WPS, int... NS>
static KzCountKernel kz_count_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzCountKernel table[] = {{(const void*)kz_knn_count_h_kernel<NS, WPS>, KzCntCfg<WPS, NS>::LDS_BYTES, NS}...};
    for (const KzCountKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzCountKernel{};
}
