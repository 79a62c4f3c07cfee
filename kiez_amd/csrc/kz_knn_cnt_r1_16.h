// COUNT SWEEP WITH A RANK-ONE THRESHOLD (kz_rank_r1_sweep.h: kz_gold_ranks_reduced_sweep): the count sweep of kz_knn_cnt16.h for an
// interval that is not two numbers per query row but depends on the index row too -- ranks under a pointwise hubness reduction.
// "w_ij against w_ig" is a bound on the pair's ranking value that is rank one plus separable (kz_knn_reduced_sweep.h "THE FORMS"); in
// the units of the fp16 tier's key the kernel forms
//     t_ij = fma(Q'_i, U_j, key~_ij + V'_j)
// and orders it against TWO numbers of the query row:  t < P_lo'  -- surely farther than the gold row: ignored;  t > P_hi'  -- surely
// closer: counted in a lane-private integer;  P_lo' <= t <= P_hi'  -- undecided, the BAND: logged as {listed row, index row, t}.
// It is the count epilogue of kz_knn_count_h_kernel on the data movement of kz_knn_emit_r1_h_kernel; neither kernel does both.
//
// The main loop is a COPY of kz_knn_count_h_kernel's (as the two emit kernels' are, so that the existing builds' generated code stays
// what it is): 4 waves x 32 queries, the query tile stationary in qf[NSR], the index image by saddr-form LDS-DMA through a ring of 2 P
// slots with one barrier per P slices, one v_mfma_f32_32x32x16_f16 per 16 k, the hand-written waits (kz_knn_device.h "WAITCNT PASS"),
// kz_plan.h work items unchanged, the ring / fragment-set configurations of KzCntCfg.
//
// DATA MOVEMENT: the rank-one kernel's.
//   * the bias row is the shifted copy bias + h V' / scale (kz_r1_index_kernel): acc starts from it;
//   * U tile: 128 floats per index tile by 4-byte LDS-DMA -- waves 0 and 1 copy the NEXT tile's bias, waves 2 and 3 copy THIS tile's
//     U.  Two buffers by tile parity.  Lifetime: the copy is issued at the tile's start, is complete at the tile's slice barrier
//     (s_waitcnt vmcnt(0) in front of s_barrier; every tile has one: static_assert below) and is read in the tile's epilogue only.
//     Buffer (tile & 1) was last read in the epilogue of tile - 2; the slice barrier of tile - 1 lies between that read and this
//     write, because a wave reaches that barrier only behind its own epilogue of tile - 2.  (Copying the NEXT tile's U, as the bias
//     does, would race: the buffer's last reader is the epilogue of tile - 1 and no barrier separates a wave still in it from one
//     that has begun this tile.)  The epilogue here reads the U tile up to twice (count, then band): both inside the same epilogue.
//   * {Umin, Umax} of the tile's real rows: one 8-byte scalar load per tile from a [n_ytiles] array;
//   * {P_lo', P_hi', Q'} per query: 128 x 16 bytes in LDS, written in the prologue, re-read in every epilogue (no room for three more
//     registers beside the stationary query tile at three workgroups per CU); beside them 16 bytes {U_good, U_far} that only a tile
//     which passes the reject reads (below).
// LDS: ring + 2 bias rows + 2 U rows + 4 KiB = 22 / 38 KiB (KzCntR1Cfg).
//
// EPILOGUE of a tile.  The max tree m over the lane's 64 keys, then the emit-r1 kernel's cheap reject against P_lo':
//     m + max(Q' Umin, Q' Umax) + 2^-22 (|X| + |m|)  >=  P_lo'
// as one ballot (kz_knn_emit_r1_16.h shows why no row of the tile reaches P_lo' where it fails; P_lo' <= P_hi', so none is above
// P_hi' either): the common tile costs the count kernel's plus two multiplies, a max and an FMA.  Else the wave reads the U tile and
// forms t = fma(Q', U_j, acc_j) on the fly for its 64 elements -- no t[] array is kept: cnt += (t > P_hi'), nb += (P_lo' <= t <= P_hi').
// Two per-row numbers guard the squared (euclidean CSLS / DUAL) forms, whose bound ((c + b_j) / s)^2 says nothing where c + b_j < 0:
// an element with U_j < U_far has a NEGATIVE outward distance bound -- surely farther whatever its key -- and is dropped; an element
// is COUNTED only with U_j > U_good (its inward bound is positive); between the two it can only be logged.  Every other form
// passes -inf for both.
// Where a lane has band entries the wave takes ONE range of the log with one atomic (prefix sum of the lanes' nb), every lane forms
// its t again (the same FMA on the same operands: the same bits), writes its entries and bumps its row's band counter.  Entries past
// the log's capacity are dropped; the counters still advance, so the host sees the overflow.
// End of an item: the two lane halves of a query are added with one cross-lane move and ONE integer atomic per query goes to
// rank[list[qrow]] -- several index ranges of a query add into it, in any order.
// Pad index rows carry bias -inf and U = 0: t = -inf, below every finite P_lo'.  Pad query rows (and rows the host does not trust)
// carry P_lo' = P_hi' = +inf, Q' = 0: nothing counted, nothing logged; no NaN is formed (the unit is built with -fno-honor-nans).
#pragma once
#include <type_traits>
#include <utility>

#include "kz_knn_emit_r1_16.h"   // KzCntCfg, KzCountKernel, kz_f16x8, the address_space(1) / (4) pointer types

struct KnnCountR1Params {
    const float* qpack;    // fp16 image of the listed query rows
    const float* ypack;    // fp16 image of the index
    const float* ybias;    // [index tiles x 128] the image's bias row + V' (pad rows -inf)
    const float* yu;       // [index tiles x 128] U (pad rows 0)
    const float2* urange;  // [index tiles] {Umin, Umax} over the tile's real rows
    const int4* work;      // {query tile, first index tile, end index tile, range} per workgroup (kz_plan.h)
    int n_ytiles;
    const float4* plq;     // [2 x query rows incl. padding] {P_lo', P_hi', Q', 0}, {U_good, U_far, 0, 0}
    const struct KnnCountR1Out* out;   // (device memory) where the counts and the band go
};
// What only the band path and the end of an item read: behind ONE pointer, fetched there by scalar loads, so that the sixteen scalar
// registers these would take do not stay live across the sweep (with them in the parameter block every build spilled scalars).
struct KnnCountR1Out {
    const int* list;       // [n_list] listed row -> row of the rank vector
    long long* rank;       // the caller's rank vector: += surely-closer count of listed row r at rank[list[r]]
    int* band_cnt;         // [query rows incl. padding] band entries per listed row (counted also past the log's capacity)
    unsigned long long* log_cnt;   // band entries of the launch
    long long log_cap;
    i32x2e* log_meta;      // [log_cap] {listed row, index row}
    float* log_key;        // [log_cap] t = fma(Q', U, key~ + V')
    int n_list;
    int pad;
};
typedef const __attribute__((address_space(4))) KnnCountR1Out kz_r1_const_out;

template <int WPS, int NSR>
struct KzCntR1Cfg {
    static constexpr int RING = KzCntCfg<WPS, NSR>::RING;
    static constexpr int PERIOD = RING / 2;
    static constexpr int BIAS_OFF = RING * 4096;      // 2 x 128 floats
    static constexpr int U_OFF = BIAS_OFF + 1024;     // 2 x 128 floats
    static constexpr int PLQ_OFF = U_OFF + 1024;      // 128 x {P_lo', P_hi', Q', 0, U_good, U_far, 0, 0}
    static constexpr int LDS_BYTES = PLQ_OFF + 4096;
};

// The band of one tile: the wave reserves sum(nb) log entries with one atomic; a lane forms its 64 t again from acc and the U tile
// (up: the lane half's view of it) and writes its nb entries in accumulator order.
// Row of accumulator position (mt, r) of lane half h: tile * 128 + 32 mt + 8 (r >> 2) + 4 h + (r & 3)  (kz_range_group).
__device__ __forceinline__ void kz_count_r1_band(const f32x16 (&acc)[4], const float* up, const float lo, const float hi, const float qv, const float ug,
                                                 const float uf, const int nb, const int tile, const int qrow, kz_r1_const_out* o) {
    const int lane = threadIdx.x & 63;
    int incl = nb;   // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int s = __shfl_up(incl, off, 64);
        if (lane >= off) incl += s;
    }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    kz_cnt_glb_u64* log_cnt = (kz_cnt_glb_u64*)o->log_cnt;
    const long long log_cap = o->log_cap;
    unsigned long long base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(log_cnt, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    if (nb > 0) {
        kz_cnt_glb_i32x2* log_meta = (kz_cnt_glb_i32x2*)o->log_meta;
        kz_cnt_glb_f32* log_key = (kz_cnt_glb_f32*)o->log_key;
        __hip_atomic_fetch_add((kz_cnt_glb_i32*)o->band_cnt + qrow, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long pos = (long long)base + (incl - nb);
        const int rowbase = tile * KZ_TILE + 4 * (lane >> 5);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 u4 = *reinterpret_cast<const float4*>(up + 32 * mt + 8 * g4);
                const float uu[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = fmaf(qv, uu[e], acc[mt][4 * g4 + e]);
                    t = uu[e] < uf ? -INFINITY : t;
                    const float ta = uu[e] > ug ? t : -INFINITY;
                    if (t >= lo && !(ta > hi)) {
                        if (pos < log_cap) {
                            i32x2e mo;
                            mo.x = qrow;
                            mo.y = rowbase + 32 * mt + 8 * g4 + e;
                            log_meta[pos] = mo;
                            log_key[pos] = t;
                        }
                        ++pos;
                    }
                }
            }
        }
    }
}

template <int NSR, int WPS>
__global__ __launch_bounds__(256, WPS) void kz_knn_count_r1_h_kernel(KnnCountR1Params p) {
    using Cfg = KzCntR1Cfg<WPS, NSR>;
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
    float4* lbuf = reinterpret_cast<float4*>(smem + Cfg::PLQ_OFF);
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
    // {P_lo', P_hi', Q'} of the tile's queries: re-read from LDS in every epilogue
    lbuf[tid] = p.plq[(int64_t)qt * 2 * KZ_TILE + tid];
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
        // ---- the rank-one counting epilogue ----
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
        const float4 pl = lbuf[2 * (32 * (tid >> 6) + (tid & 31))];   // {P_lo', P_hi', Q'}
        // (uniform, through the constant address space: a SCALAR load -- a vector load would be awaited with vmcnt(0), a wait for the
        //  whole DMA ring in every tile; tools/check_waits.py reports that as a vmcnt finding)
        const kz_r1_const_f32* ur = (const kz_r1_const_f32*)p.urange + 2 * (int64_t)__builtin_amdgcn_readfirstlane(tile);
        const float x = fmaxf(pl.z * ur[0], pl.z * ur[1]);
        const float reach = fmaf(2.384185791015625e-07f /* 2^-22 */, fabsf(x) + fabsf(m), x + m);
        if (__builtin_amdgcn_ballot_w64(reach >= pl.x) != 0ull) {
            int h_now;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshrrev_b32 %0, 5, %0" : "=v"(h_now));
            const float* up = ubuf + (tile & 1) * 128 + 4 * h_now;
            const float4 ut = lbuf[2 * (32 * (tid >> 6) + (tid & 31)) + 1];   // {U_good, U_far}
            int c = 0, ge = 0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 u4 = *reinterpret_cast<const float4*>(up + 32 * mt + 8 * g4);
                    const float uu[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // (one compare, one select or add each: no mask is combined with another, the compares go through VCC)
                        float t = fmaf(pl.z, uu[e], acc[mt][4 * g4 + e]);
                        t = uu[e] < ut.y ? -INFINITY : t;                       // surely farther whatever its key: dropped
                        const float ta = uu[e] > ut.x ? t : -INFINITY;          // may be counted only behind U_good
                        ge += t >= pl.x ? 1 : 0;
                        c += ta > pl.y ? 1 : 0;
                    }
                }
            }
            cnt += c;
            const int nb = ge - c;   // (P_lo' <= P_hi': every counted element is among the ge)
            if (__builtin_amdgcn_ballot_w64(nb > 0) != 0ull)
                kz_count_r1_band(acc, up, pl.x, pl.y, pl.z, ut.x, ut.y, nb, tile, qrow, (kz_r1_const_out*)p.out);
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
    kz_r1_const_out* o = (kz_r1_const_out*)p.out;
    if (lane_now < 32 && cnt > 0 && qrow < o->n_list) {
        kz_cnt_glb_i32* list = (kz_cnt_glb_i32*)o->list;
        kz_cnt_glb_u64* rank = (kz_cnt_glb_u64*)o->rank;
        __hip_atomic_fetch_add(rank + list[qrow], (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The builds live in two instantiation units (kz_knn_cnt_r1_lo.hip: 2 .. 13 slices, three workgroups per CU; kz_knn_cnt_r1_hi.hip:
// 14 .. 24 slices, two) and come back in the count kernel's descriptor: a slice count without a build gets the empty descriptor.
KzCountKernel kz_count_r1_lookup_lo(int n_slices);
KzCountKernel kz_count_r1_lookup_hi(int n_slices);

template <int WPS, int... NS>
static KzCountKernel kz_count_r1_table(int n_slices, std::integer_sequence<int, NS...>) {
    static const KzCountKernel table[] = {{(const void*)kz_knn_count_r1_h_kernel<NS, WPS>, KzCntR1Cfg<WPS, NS>::LDS_BYTES, NS}...};
    for (const KzCountKernel& k : table)
        if (k.n_slices == n_slices) return k;
    return KzCountKernel{};
}
