// Exact k-nearest-neighbour search on MI355X (gfx950):  replaces SklearnNN._kneighbors
// (kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101 -> sklearn brute-force ArgKmin,
//  sklearn/metrics/_pairwise_distances_reduction/_argkmin.pyx.tp:311-510).
//
// Three stages (DESIGN.md "Kernels"):
//   1. kz_knn_cand_kernel   fused  X.Y^T (float32 MFMA 32x32x2)  +  per-query top-K' candidate lists.
//                           The n_q x n_i similarity matrix never leaves registers.
//   2. kz_knn_finalize      (kz_knn_finalize.h) merge the lists, CERTIFY that the true top-k is inside the candidate set using a
//                           rigorous float32 rounding bound, re-rank the K' candidates with exact float64
//                           distances, sort, strip the query itself (single-source mode), write [q, k].
//   3. kz_exact_*           (kz_exact.h) exact float64 brute force for the (rare) rows that could not be certified.
// This file: the float32-operand kernel, launch plumbing, the escalation helpers and the host ladder kz_knn_impl.
// Result: neighbour order == order of the float64 distances the reference computes; no approximation.
#include <chrono>
#include <vector>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "kz_common.h"
#include "kz_bool.h"
#include "kz_precomputed.h"
#include "kz_floor.h"

#include "kz_knn_device.h"
#include "kz_knn_kernels.h"

// The shipped fused kernel (kernel_variant 0).
// NRES = number of leading 16-k slices whose QUERY fragments stay resident in registers for the whole sweep
// (8 slices = d 128 = 64 VGPRs); slices beyond NRES are streamed from L2 with non-temporal loads.  Residency is opt-in
// (force_nres): at the register budget of three waves per SIMD it spills and measured slower than streaming
// (HISTORY.md section 7); NRES = 0 is what runs by default.
template <int KP, int NRES>
__global__ __launch_bounds__(256, 3) void kz_knn_cand_kernel(KnnCandParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ybuf = reinterpret_cast<float*>(smem);  // 2 x 2048 floats (+ 2 x 128 bias floats behind them)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int j = lane & 31;
    const int h = lane >> 5;

    // The host schedules the work (kz_knn): large items first, small items to fill the tail, and an XCD-aware
    // order (blocks b and b+8 share an XCD and its L2: co-resident blocks stream the SAME index range).
    const int4 wd = p.work[blockIdx.x];
    const int qt = wd.x;
    const int t_begin = wd.y;
    const int t_end = wd.z;
    const int s = wd.w;
    const int NS = p.kg >> 2;  // >= NRES (host picks NRES)
    const int total = (t_end - t_begin) * NS;

    // Candidate state of this lane = one (query, lane-half) pair:
    //   list  K' best (key, row) so far, UNSORTED, living directly in the output arrays (global memory, L2-resident);
    //         touched only at merges;
    //   log   up to KZ_LOG_CAP keys that beat the pruning threshold since the last merge (LDS, append-only).
    // The threshold is only refreshed at merges, which follow a geometric schedule in the number of tiles seen
    // (identical for every lane, so merges run with all 64 lanes busy); a full log forces an early merge.
    const int64_t listoff = kz_list_wave_base((int64_t)qt * KZ_TILE + 32 * wave + j, p.lay, KP, s) + h * 32 + j;
    KzCandState st;
    st.lk = p.out_key + listoff;
    st.li = p.out_idx + listoff;
    st.sk = reinterpret_cast<float*>(smem + KZ_CAND_LDS_BASE) + tid;
    st.si = reinterpret_cast<int*>(smem + KZ_CAND_LDS_BASE + KZ_LOG_CAP * 256 * 4) + tid;
#pragma unroll 4
    for (int e = 0; e < KP; ++e) {
        st.lk[e * KZ_LSTRIDE] = -INFINITY;
        st.li[e * KZ_LSTRIDE] = -1;
    }
    st.tau = -INFINITY;
    st.minpos = 0;
    st.cnt = 0;
    st.tiles_done = 0;
    st.next_merge = 1;

    if (total > 0) {
        const float4* ysrc = reinterpret_cast<const float4*>(p.ypack + ((int64_t)t_begin * NS) * 2048);
        const float* qbase = p.qpack + ((int64_t)(p.qt0 + qt) * p.kg) * 512 + (32 * wave + j) * 4;
        float* bbuf = ybuf + 4096;  // 2 x 128 floats: accumulator-init (bias) rows of the current / next tile
        // prologue: slice 0 and the bias rows of the first tile
        {
            float4* nb = reinterpret_cast<float4*>(ybuf);
            nb[tid] = ysrc[tid];
            nb[tid + 256] = ysrc[256 + tid];
            bbuf[(t_begin & 1) * 128 + (tid & 127)] = p.ybias[(int64_t)t_begin * KZ_TILE + (tid & 127)];
        }
        // resident query fragments: lane (j, h) needs k-groups 4*sl + 2*t + h of its query row
        float4 qres[NRES > 0 ? NRES : 1][2];
#pragma unroll
        for (int u = 0; u < NRES; ++u) {
            qres[u][0] = *reinterpret_cast<const float4*>(qbase + (4 * u + h) * 512);
            qres[u][1] = *reinterpret_cast<const float4*>(qbase + (4 * u + 2 + h) * 512);
        }
        // streamed query fragments (slices >= NRES), current slice in qb
        float4 qb0 = make_float4(0.f, 0.f, 0.f, 0.f), qb1 = qb0;
        if (NRES == 0 || NS > NRES) {
            qb0 = *reinterpret_cast<const float4*>(qbase + (4 * NRES + h) * 512);
            qb1 = *reinterpret_cast<const float4*>(qbase + (4 * NRES + 2 + h) * 512);
        }
        __syncthreads();

        int g = 0;
        f32x16 acc[4];
        const float* bias_n = p.ybias + (tid & 127);
        int tile = t_begin;

        // One 16-k slice: prefetch the next index slice (HBM/L2 -> registers) and the next tile's bias rows, run the
        // 32 MFMAs of the current slice out of LDS, then refill the other LDS buffer.  All loads are UNCONDITIONAL so
        // that hipcc's s_waitcnt placement keeps them in flight behind the MFMAs (a clamp re-reads the last slice at
        // the very end, harmless); sched_barriers pin loads above and the LDS refill below the MFMA block.
        // Lane (j, h) feeds k = 4*(2t+h)+jj for jj = 0..3: the k order inside a slice is permuted identically for
        // A and B, which leaves the dot product unchanged.
        auto slice_step = [&](const float4& bq0, const float4& bq1, const bool stream_q, const int sl_next) {
            const int gn = min(g + 1, total - 1);
            const float4* src = ysrc + (int64_t)gn * 512;
            const float4 ya0 = src[tid];
            const float4 ya1 = src[256 + tid];
            const int tile_n = min(tile + 1, p.n_ytiles - 1);
            const float bn = bias_n[(int64_t)tile_n * KZ_TILE];
            float4 qn0, qn1;
            if (stream_q) {
                // streaming policy for the query fragments: +2.6 % on C1 (they are never re-used from L1/L2 soon)
                qn0 = kz_nt_load4(reinterpret_cast<const float4*>(qbase + (4 * sl_next + h) * 512));
                qn1 = kz_nt_load4(reinterpret_cast<const float4*>(qbase + (4 * sl_next + 2 + h) * 512));
            }
            __builtin_amdgcn_sched_barrier(0);
            const float* buf = ybuf + (g & 1) * 2048;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float4 a[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    a[mt] = *reinterpret_cast<const float4*>(buf + ((2 * t + h) * KZ_TILE + 32 * mt + j) * 4);
                const float4 bq = t ? bq1 : bq0;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt].x, bq.x, acc[mt], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt].y, bq.y, acc[mt], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt].z, bq.z, acc[mt], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt].w, bq.w, acc[mt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                float4* nb = reinterpret_cast<float4*>(ybuf + ((g + 1) & 1) * 2048);
                nb[tid] = ya0;
                nb[tid + 256] = ya1;
                bbuf[((tile + 1) & 1) * 128 + (tid & 127)] = bn;
                if (stream_q) {
                    qb0 = qn0;
                    qb1 = qn1;
                }
            }
            // Raw barrier: __syncthreads() is fence + s_barrier and the fence drains vmcnt(0), i.e. it would wait here for
            // the query-fragment loads that are only needed at the top of the next slice.  LDS visibility needs lgkmcnt only.
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            ++g;
        };

        for (; tile < t_end; ++tile) {
            __builtin_amdgcn_sched_barrier(0);  // do not hoist the next tile's init above the epilogue (64 VGPRs)
            {
                const float* bp = bbuf + (tile & 1) * 128 + 4 * h;
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
            // resident slices: fully unrolled, fragments by static register index
#pragma unroll
            for (int u = 0; u < NRES; ++u) {
                // the last resident slice prefetches the first streamed one (if any)
                slice_step(qres[u][0], qres[u][1], (u == NRES - 1) && (NS > NRES), NRES);
            }
            // streamed slices
            if (NRES == 0 || NS > NRES) {
                int sl = NRES;
                do {  // the do-while spares the compiler a zero-trip path
                    const int sln = (sl + 1 == NS) ? NRES : sl + 1;
                    const float4 c0 = qb0, c1 = qb1;
                    slice_step(c0, c1, true, sln);
                } while (++sl < NS);
            }
            __builtin_amdgcn_sched_barrier(0);
            kz_tile_epilogue<KP>(acc, st, tile, tile == t_end - 1, h);
        }
    }
}

#include "kz_knn_bf16.h"

#include "kz_knn_finalize.h"

// (KZ_ESC_SHORT_MAX_ROWS, KZ_MAX_PIECES: kz_route.h)
static int kz_max_pieces(int KP, int halves) {
    const int m = KZ_FIN_MAXM / (halves * KP);
    return m < KZ_MAX_PIECES ? m : KZ_MAX_PIECES;
}

#include "kz_exact.h"

// ---------------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------------
// (kz_pick_list_len: kz_route.h)

// The float32-operand kernel's entries of the kernel table (kz_knn_kernels.h): one build per list length, any slice count
template <int... KPS>
static KzSweepKernel kz_sweep_f32_table(int KP, int n_slices, std::integer_sequence<int, KPS...>) {
    static const KzSweepKernel table[] = {{(const void*)kz_knn_cand_kernel<KPS, 0>, KZ_CAND_LDS, 1, 1, KPS, 0}...};
    for (KzSweepKernel k : table)
        if (k.KP == KP) {
            k.n_slices = n_slices;
            return k;
        }
    return KzSweepKernel{};
}
KzSweepKernel kz_sweep_f32_kernel(int KP, int n_slices) {
    return kz_sweep_f32_table(KP, n_slices, std::integer_sequence<int, 16, 32, 64, 128>{});
}

// (kz_plan_rounds, kz_plan_pass, kz_plan_fill_work: kz_plan.h)
extern "C" int kz_knn_plan(int64_t n_query_rows, int64_t n_index_rows, int k_eff, int slots, int force_splits, int min_splits,
                           int* n_rounds, int* round_qtiles, int* round_pieces, int* round_piece_tiles) {
    KZ_REQUIRE(n_rounds && round_qtiles && round_pieces && round_piece_tiles, "kz_knn_plan: null argument");
    KZ_REQUIRE(n_query_rows > 0 && n_index_rows > 0 && slots > 0, "kz_knn_plan: sizes must be positive");
    const int KP = kz_pick_list_len(k_eff);
    KZ_REQUIRE(KP > 0, "kz_knn_plan: k=%d exceeds the supported maximum of 110 neighbours per query", k_eff);
    const int n_qtiles = (int)((n_query_rows + KZ_TILE - 1) / KZ_TILE);
    const int n_ytiles = (int)((n_index_rows + KZ_TILE - 1) / KZ_TILE);
    int sp[KZ_MAX_REGIONS];
    kz_plan_rounds(n_qtiles, n_ytiles, slots, kz_max_pieces(KP, 1), force_splits, min_splits, n_rounds, round_qtiles, sp);
    for (int r = 0; r < *n_rounds; ++r) {
        const int len = (n_ytiles + sp[r] - 1) / sp[r];
        round_piece_tiles[r] = len;
        round_pieces[r] = (n_ytiles + len - 1) / len;
    }
    return KZ_OK;
}

// Rows of a query matrix gathered into a dense block (escalation of uncertified rows to the float32-operand kernel)
__global__ __launch_bounds__(256) void kz_gather_rows_kernel(const char* __restrict__ raw, const int* __restrict__ rows,
                                                             int64_t row0, int n_rows, int64_t row_bytes,
                                                             char* __restrict__ out, int64_t* __restrict__ self_ids,
                                                             const int64_t* __restrict__ parent_self) {
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    const int64_t src = row0 + rows[r];
    const char* sp = raw + src * row_bytes;
    char* dp = out + (int64_t)r * row_bytes;
    // (float32 / float64 rows, and 2-byte rows of an even width on a 4-byte aligned base: 4 bytes per thread.  2-byte rows of an odd
    //  width -- every other row starts 2 bytes off, and the last 4-byte copy would run 2 bytes past the row: 2 bytes per thread)
    if (((row_bytes | (int64_t)reinterpret_cast<uintptr_t>(raw) | (int64_t)reinterpret_cast<uintptr_t>(out)) & 3) == 0) {
        for (int64_t b = threadIdx.x * 4; b < row_bytes; b += 256 * 4) *reinterpret_cast<int*>(dp + b) = *reinterpret_cast<const int*>(sp + b);
    } else {
        for (int64_t b = threadIdx.x * 2; b < row_bytes; b += 256 * 2)
            *reinterpret_cast<unsigned short*>(dp + b) = *reinterpret_cast<const unsigned short*>(sp + b);
    }
    // index row to strip for this query: its own row, or (subset of a subset) what its parent recorded for it
    if (self_ids && threadIdx.x == 0) self_ids[r] = parent_self ? parent_self[src] : src;
}

__global__ void kz_iota_kernel(int* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

__global__ void kz_strided_rows_kernel(int* __restrict__ out, int n, int64_t stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int)((int64_t)i * stride);
}

__global__ __launch_bounds__(256) void kz_scatter_rows_kernel(const double* __restrict__ sd, const int64_t* __restrict__ si,
                                                              const int* __restrict__ rows, int n_rows, int k,
                                                              double* __restrict__ od, int64_t* __restrict__ oi) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_rows * k) return;
    const int r = (int)(t / k), c = (int)(t - (int64_t)r * k);
    od[(int64_t)rows[r] * k + c] = sd[t];
    oi[(int64_t)rows[r] * k + c] = si[t];
}

// (KZ_TIER_F32 / KZ_TIER_BF / KZ_TIER_H, the operand precision of the fused kernel: kz_knn_kernels.h)
// One launch of a fused kernel: list layout, scratch carve-up and the uploaded work table.
struct KzPass {
    KzListLayout lay;
    int W;            // workgroups
    int W0;           // boot_first: the first W0 items of the table are the items of index range 0 (else 0)
    float* out_key;   // candidate lists (scratch)
    int* out_idx;
    int* fail_list;   // [fail_rows] (scratch)
    double* fail_tau; // [fail_rows] (scratch; KnnFinParams::fail_tau)
    int4* d_work;     // [W] (scratch)
};

// The plan of one launch of a tier's fused kernel (kz_plan_pass): tier decides the list layout (fp16: K' contiguous entries per
// list; float32 kernels: two lane-half lists per query and range).  tpw = query tiles per workgroup (2: the 64-query kernel,
// kz_knn_h64.h): the plan is made for UNITS of tpw consecutive query tiles -- one work item = one unit x one index range, w4.x =
// its first tile -- and converted back to tiles for the list layout (a region ends on a unit boundary, the last one at the last tile).
static void kz_plan_tier_pass(const kz_ctx* ctx, int n_qtiles, int n_ytiles, int slots, int max_pieces, int KP, int tier, int tpw, int force_pieces,
                              int min_pieces, KzPlan* pl) {
    kz_plan_pass(n_qtiles, n_ytiles, slots, max_pieces, (tier == KZ_TIER_H ? 1 : 2) * KP, tier == KZ_TIER_F32 ? 2 : 1, tier == KZ_TIER_H ? 1 : 0, tpw,
                 force_pieces > 0 ? force_pieces : ctx->force_splits, min_pieces > 1 ? min_pieces : 1, pl);
}
// Carves the context's scratch block for a planned pass and uploads its work table (n_ytiles, slots, tier, tpw: what the plan was made with).
static int kz_prepare_pass(kz_ctx* ctx, const KzPlan& pl, int n_ytiles, int slots, int tier, int64_t fail_rows, KzPass* out, int tpw = 1,
                           bool boot_first = false) {
    const KzListLayout& lay = pl.lay;
    const int W = pl.W;
    const size_t list_elems = pl.list_elems;
    // (the kernels address a launch's lists with 32-bit element offsets -- kz_knn_h16.h "off_u"; a K' = 16 chunk of 2 M rows over
    //  KZ_MAX_PIECES = 128 ranges is exactly 2^32 elements: refused here instead of wrapping there)
    KZ_REQUIRE(list_elems < ((size_t)1 << 32), "kz_knn: the candidate lists of one launch exceed 2^32 entries (%zu): fewer rows per chunk (option chunk_rows)", list_elems);
    const size_t key_bytes = (list_elems * 4 + 255) & ~(size_t)255;
    const size_t fail_bytes = ((size_t)fail_rows * 4 + 255) & ~(size_t)255;
    const size_t tau_bytes = ((size_t)fail_rows * 8 + 255) & ~(size_t)255;
    const size_t work_bytes = ((size_t)W * sizeof(int4) + 255) & ~(size_t)255;
    void* scratch = nullptr;
    int rc = kz_scratch(ctx, key_bytes * 2 + fail_bytes + tau_bytes + work_bytes, &scratch);
    if (rc != KZ_OK) return rc;
    out->lay = lay;
    out->W = W;
    out->out_key = (float*)scratch;
    out->out_idx = (int*)((char*)scratch + key_bytes);
    out->fail_list = (int*)((char*)scratch + 2 * key_bytes);
    out->fail_tau = (double*)((char*)scratch + 2 * key_bytes + fail_bytes);
    out->d_work = (int4*)((char*)scratch + 2 * key_bytes + fail_bytes + tau_bytes);
    {
        // host-side table (pinned staging grows on demand)
        const size_t need = work_bytes;
        if (need * 2 > ctx->h_stage_bytes) {
            KZ_HIP(hipStreamSynchronize(ctx->stream));
            if (ctx->h_stage) KZ_HIP(hipHostFree(ctx->h_stage));
            ctx->h_stage = nullptr;
            ctx->h_stage_bytes = 0;
            KZ_HIP(hipHostMalloc(&ctx->h_stage, need * 4, hipHostMallocDefault));
            ctx->h_stage_bytes = need * 4;
        }
        // The table of the PREVIOUS pass may still be in flight out of h_stage when two passes follow each other without a
        // read-back in between (dual pass: sample sweep, then the main sweep): passes alternate between the two halves of
        // the staging buffer, and every second pass is followed by a stream synchronisation in any case (kz_knn_impl's
        // fail-counter read).
        ctx->h_stage_flip ^= 1;
        int4* hw = (int4*)((char*)ctx->h_stage + (ctx->h_stage_flip ? ctx->h_stage_bytes / 2 : 0));
        static_assert(sizeof(KzWorkItem) == sizeof(int4), "work items are uploaded as int4");
        // (fp16 kernel: query groups of four times what an XCD holds, see kz_plan_fill_work; "qgroup" overrides.  500k x 500k,
        //  ten ranges per query tile, main kernel: 24: 109.3 ms, 96: 107.6, 384: 102.5, 768 .. 4096: 101.9 .. 103.2)
        const int per_xcd = (slots + 7) / 8;
        const int qgroup = tier == KZ_TIER_H && 4 * per_xcd > KZ_QGROUP ? 4 * per_xcd : KZ_QGROUP;
        kz_plan_fill_work(pl, n_ytiles, tpw, (KzWorkItem*)hw, qgroup);
        out->W0 = 0;
        if (boot_first) {
            // RANGE-0 BOOTSTRAP (kz_knn_impl): the items of index range 0 first -- they are launched on their own, the others
            // behind them with a floor read off range 0's lists.  (Stable: both groups keep the XCD-aware order among themselves.)
            KzWorkItem* w = (KzWorkItem*)hw;
            out->W0 = (int)(std::stable_partition(w, w + W, [](const KzWorkItem& it) { return it.w == 0; }) - w);
        }
        KZ_HIP(hipMemcpyAsync(out->d_work, hw, (size_t)W * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    }
    return KZ_OK;
}

// ---------------------------------------------------------------------------------------------------
// POPULATION FLOOR (seeded lists).  A list that starts empty (threshold -inf) takes K' (1 + ln(n / K')) events per query over a
// sweep, half of them in the first few tiles.  A strided probe of the query rows (an escalation-style sub-search: the tier
// probe of an ordinary search, a probe of its own in kz_knn_dual; exact float64 results, written to their places) shows where
// the k-th best key of a row lies as a function of |q_c|^2: least squares over the probe, the floor = the model minus the
// largest shortfall seen (times "floor_margin").  Every list of the main sweep then STARTS at its row's floor
// (KnnCandParams::qfloor), and the finalize kernel counts the floor into its bound on the rows outside the lists
// (KnnFinParams::list_floor).  A row whose k-th key lies below its floor ends with fewer than k candidates, is not certified
// and is searched again like any other uncertified row: the floor decides how many rows take that path, never a result.  Whatever
// the data looks like, a row falls short of the largest shortfall among P probe rows with probability 1 / (P + 1) (the rows are
// exchangeable): at most ~n / P rows of a call take the detour.
// ---------------------------------------------------------------------------------------------------
// probe row i = matrix row i * stride: (|q_c|^2, exact key of its k-th neighbour) from the probe's float64 distances.
// key = (|q_c|^2 - d^2) / 2 with d^2 = the squared distance (cosine: 2 x distance, rows are unit vectors).
__global__ void kz_floor_pairs_kernel(const double* __restrict__ dist, const double* __restrict__ rowq, int n_probe, int64_t stride, int k,
                                      int metric, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_probe) return;
    const int64_t r = (int64_t)i * stride;
    const double v = dist[r * k + k - 1];
    const double d2 = metric == KZ_EUCLIDEAN ? v * v : (metric == KZ_COSINE ? 2.0 * v : v);
    const double x = rowq[r * 3];
    out[2 * i] = x;
    out[2 * i + 1] = 0.5 * (x - d2);
}
// floor of list row p (matrix row row_map[p]) in the units of the sweep's approximate keys: the model's key minus the
// margin, minus the rounding bound of this row's approximate keys (the finalize kernel's eps_q), scaled and rounded down.
// Pad rows: +inf (no events at all).
__global__ void kz_floor_rows_kernel(const int* __restrict__ row_map, int64_t n, int64_t n_pad, const double* __restrict__ rowq,
                                     const double* __restrict__ y_hmax, const double* __restrict__ hscale, double alpha, double beta,
                                     double margin, double eps_mult, double gamma_acc, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pad) return;
    const int64_t r = row_map ? (int64_t)row_map[p] : (p < n ? p : -1);   // (no map: the rows in their own order)
    if (r < 0) {
        out[p] = INFINITY;
        return;
    }
    const double qc2 = rowq[r * 3 + 0], qh = rowq[r * 3 + 1], qr = rowq[r * 3 + 2];
    const double Yh = y_hmax[0], Ry = y_hmax[1], Yc2 = y_hmax[2];
    const double qc = sqrt(qc2), yc = sqrt(Yc2);
    const double eps = eps_mult * (qr * Yh + qh * Ry + qr * Ry + gamma_acc * (0.5 * Yc2 + qh * Yh) +
                                   1.1920928955078125e-07 * (qc + yc) * (qc + yc) + 1e-12 * (0.5 * Yc2 + qc2));
    const double f = (alpha + beta * qc2 - margin - eps) / hscale[1];
    float ff = (float)f;
    if ((double)ff > f) ff = nextafterf(ff, -INFINITY);
    out[p] = ff;
}

static inline double kz_gamma_acc_h(int kg) { return 2.0 * (double)(kg * 4 + 16) * 5.9604644775390625e-08; }
// model = {alpha, beta, margin}; *ok = false when the probe's values are not finite (no floor then).  `dist`: [.., k] results whose
// row i * stride is probe row i; rowq: the query image's per-row statistics, same row numbering.  Waits for the stream.
static int kz_floor_model(kz_ctx* ctx, const double* dist, const double* rowq, int n_probe, int64_t stride, int k, int metric, double* model,
                          bool* ok, double* r2 = nullptr) {   // (r2: the share of the keys' variance the fit explains, kz_floor_r2)
    KzPoolBuf<double> d_pairs;
    int rc = d_pairs.alloc(ctx, (size_t)n_probe * 16);
    if (rc != KZ_OK) return rc;
    std::vector<double> hp((size_t)n_probe * 2);
    hipLaunchKernelGGL(kz_floor_pairs_kernel, dim3((unsigned)((n_probe + 255) / 256)), dim3(256), 0, ctx->stream, dist, rowq, n_probe, stride, k,
                       metric, d_pairs.get());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hp.data(), d_pairs.get(), (size_t)n_probe * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d_pairs.reset();
    if (e != hipSuccess) {
        kz_set_error("kz_knn: floor probe failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    *ok = kz_floor_fit(hp.data(), n_probe, ctx->floor_margin, model);
    if (r2) *r2 = *ok ? kz_floor_r2(hp.data(), n_probe) : 0.0;
    return KZ_OK;
}

// RANGE-0 BOOTSTRAP of the short-list routes (round 5).  A query keeps one list of 16 per index RANGE of the row-dealt image, and
// range 0 of a dealt image is a systematic 1 / P sample of the index: the smallest key of its full list -- the 16th best over the
// sample, about rank 16 P over everything -- is a lower bound of the query's 16 P-th best key, known after 1 / P of the sweep.  The
// other P - 1 ranges are swept behind it with their lists STARTING at that floor (KnnCandParams::qfloor, as the population floor of
// the seeded lists does): keys at or below it never become events.  A list that starts empty takes 16 (1 + ln(n / (16 P)))
// events; with the floor a range sees about the 16 P / P = 16 rows above it -- P = 32 lists on 300 k rows: ~3 800 events per query
// without, ~700 with.  The finalize kernel counts the floor into its bound (KnnFinParams::list_floor) exactly as for seeded lists:
// a floor can only make a row uncertified (searched again), never change a result.
__global__ void kz_boot_floor_kernel(const float* __restrict__ in_key, const int* __restrict__ in_idx, KzListLayout lay, int KP, int64_t list_row0,
                                     int64_t q_begin, int64_t q_count, const float* __restrict__ prev, float* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= q_count) return;
    const int64_t l0 = kz_list_contig_off(list_row0 + q, lay, KP, 0);
    float mn = INFINITY;
    bool full = true;
    for (int e = 0; e < KP; ++e) {
        full = full && in_idx[l0 + e] >= 0;
        mn = fminf(mn, in_key[l0 + e]);
    }
    float f = full ? mn : -INFINITY;
    if (prev) f = fmaxf(f, prev[q_begin + q]);
    out[q_begin + q] = f;
}

__global__ void kz_floor_nudge_kernel(float* __restrict__ f, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && f[i] > -INFINITY) f[i] = nextafterf(f[i], -INFINITY);
}

// Escalation of uncertified rows: gather rows cq_begin + fail_list[0 .. n_fail) of `query` into a dense block, search it
// again (kz_knn_impl with the given precision / minimum list length; that call sends ITS uncertified rows further down)
// and scatter the results into out_dist / out_ind at the rows' positions.  Ends with a stream synchronisation.
// Dual pass (kz_knn_dual.h): what the main sweep needs to report the events of the index rows besides its own lists.
struct KzDualPass {
    int probed;                    // the caller's tier probe has looked at this data (and chose the shared fp16 sweep): no ladder after the fact
    const float* qpack;            // fp16 image of the query rows in a load-balanced order (kz_knn_dual.h "stratified deal") ...
    const int* row_map;            // ... and [query tiles * 128] the matrix row of each of its rows
    const float* ypack;            // fp16 image of the index rows SORTED by their event threshold (kz_himage_pack_permuted) ...
    const float* ybias;            // ... and its accumulator-init rows
    const int* perm;               // [index rows] matrix row of image row r: list entries are translated by the finalize kernel
    const float* theta;            // [index tiles * 128] per row of the sorted image: the smallest threshold of its tile
    const float* qnbias;           // [query tiles * 128]
    const float* qfloor;           // [query tiles * 128] or nullptr: seeded forward lists (kz_knn_dual.h "population floor")
    void* log_keys;
    void* log_meta;
    unsigned long long* log_cnt;   // device counter
    long long log_cap;
    int broken;                    // set by kz_knn_impl when a chunk did not run the dual build (tier change): events incomplete
    int short_pieces, short_ksel, short_kp;  // > 0: the forward lists are short_pieces lists of 16 per query (the image interleaves the index tiles
                                   // over the ranges, kz_knn_dual.h), the finalize kernel selects short_ksel of their entries
    double main_ms;
    // called by kz_knn_impl right behind the launch of the LAST chunk's sweep (the event log is complete once that kernel has
    // run): kz_knn_dual enqueues the reverse direction's chain on the context's second stream there, so that it runs beside the
    // forward direction's finalize kernel, read-back and re-search instead of behind them
    int (*post_sweep)(void* user);
    void* post_user;
    int post_called;
    // NESTED sample sweep (kz_knn_dual.h "NESTED"): the pass is the sweep of b x sample(a) -- its index side is only the first
    // n_ytiles tiles of `ypack` (the sorted sample image; `index` stays the whole matrix a), its forward lists are wanted RAW
    // (thresholds are read off them by the caller's post_sweep hook: lists_* below are filled in before the hook runs) and are
    // never finalized; at most max_entries list entries per query (the threshold kernel ranks <= 256).
    int n_ytiles;
    int raw_lists;
    int max_entries;
    int no_q64;                    // the 32-queries-per-wave build whatever "h_q64" says (kz_range.h reads that build's log format)
    const float* lists_key;
    const int* lists_idx;
    KzListLayout lists_lay;
    int lists_KP;
};
// query rows one launch of the fused kernels takes (the candidate lists of a launch stay below ~1 GiB)
static inline int64_t kz_rows_per_chunk(const kz_ctx* ctx, int KP_mem, bool wide_route) {
    return ctx->chunk_rows > 0 ? ctx->chunk_rows : (int64_t)128 * 4096 * (wide_route ? 1 : (KP_mem <= 16 ? 4 : (KP_mem <= 32 ? 2 : 1)));
}
// SPECULATIVE RESCUE (round 6).  A pass on data that is fine still leaves a HANDFUL of rows uncertified (near-ties around the k-th
// place, a crowded index range: 2 - 20 rows of a 15 k .. 1 M row search), and what they cost was never the arithmetic: the host had to
// learn the count (read-back + stream synchronisation), gather the rows into a sub-matrix, pack it, sweep the whole index for one
// query tile (a latency-bound launch: 108 us on a 15 k-row index), finalize, scatter, synchronise again -- 0.25 ms per search of a
// 15 k x 15 k step that takes 1.7 ms (bench.py "ea15k"), 1.3 ms per step on a 1 M-row index.  The exact float64 kernels answer a row
// for n d multiply-adds whatever the data: they are launched BEHIND the finalize kernel, before the host knows anything, for up to R
// rows -- grid sized for R, the count read from device memory (kz_spec_row_live), every workgroup of a dead row returns at once.  R is
// 4 .. "spec_rows" (64), as many as "spec_elems" / (n d) allows (a row of a 1 M x 200 index is 0.2 G multiply-adds: R = 8).  The
// read-back that follows tells the host whether that was all (count <= R: the results are in place -- the exact float64 order, what
// every route returns) or whether the ordinary re-search has to run (count > R: the speculative launches did nothing).
// (two selection levels from two chunks on: a handful of rows, nothing else hides the single-level kernel's passes over the row)
constexpr int KZ_SPEC_TWO_LEVEL_FROM = 2;
struct KzSpec {   // (the buffers in reverse release order: qd, vals, cand_v, cand_i)
    int R = 0;            // rows the speculative launches cover (0: not launched)
    KzPoolBuf<int> cand_i;
    KzPoolBuf<double> cand_v;
    KzPoolBuf<double> vals;
    KzPoolBuf<double> qd;   // float64 operand rows of the (up to R) query rows: kz_exact_lanes.h
};
static int kz_spec_rows(const kz_ctx* ctx, const kz_matrix* index, int k_eff) {
    if (ctx->spec_rows <= 0 || index->metric >= KZ_MANHATTAN || k_eff > 64) return 0;
    const double nd = (double)index->n * (double)index->d;
    int R = (int)(KZ_K_SPEC_ELEMS / (nd > 1.0 ? nd : 1.0)) & ~3;
    // (where the one-pair-per-lane kernel takes the launch -- kz_spec_rescue -- the index is staged once per block of 16 query rows
    //  whatever their number: 32 rows cost little more than 4; 1 M x 200: 0.53 ms for 4 rows, the re-search of 16 took 3.5 ms)
    if (R < 32 && nd <= 1.0e9 && ctx->exact_rows >= 2 && index->dtype == KZ_F32 && (index->d & 3) == 0 && index->d <= 512 &&   // (<= 4 GB of rows staged, 1.3 GB of values)
        index->n >= (int64_t)4 * 64 * ctx->n_cus && ((uintptr_t)index->raw & 15u) == 0)
        R = 32;
    if (R > ctx->spec_rows) R = ctx->spec_rows & ~3;
    return R < 4 ? 0 : R;
}
// The buffers of a speculation for R rows (ahead of the launches where those run on another stream than the pool's: the reverse
// chains of kz_knn_dual -- a buffer handed out here may have been released by work that is still in flight on the context's stream).
// No memory: sp stays empty and nothing is speculated (the ordinary re-search will do).
static int kz_spec_alloc(kz_ctx* ctx, KzSpec& sp, int R, const kz_matrix* index, int k_eff) {
    KzExactSelection sel;
    int rc = kz_exact_selection(index, k_eff, KZ_SPEC_TWO_LEVEL_FROM, &sel);
    if (rc != KZ_OK) return rc;
    KzSpec s;   // (all or nothing)
    rc = s.vals.alloc(ctx, (size_t)R * (size_t)index->n * 8);
    if (rc == KZ_OK && sel.two_level) rc = s.cand_v.alloc(ctx, sel.cand_entries(R) * 8);
    if (rc == KZ_OK && sel.two_level) rc = s.cand_i.alloc(ctx, sel.cand_entries(R) * 4);
    if (rc == KZ_OK) rc = s.qd.alloc(ctx, kz_exact_lanes_qd_bytes(R, (int)index->d));
    if (rc != KZ_OK) return rc == KZ_ERR_NOMEM ? KZ_OK : rc;
    sp = std::move(s);
    return KZ_OK;
}
// fail_list / fail_count: the finalize kernel's device-side list and counter (fail_list holds rows relative to q0).  The caller's
// sp keeps its buffers whatever happens here: they are released by sp's owner, behind the stream the launches are on.
static int kz_spec_rescue(kz_ctx* ctx, KzSpec& sp, int R, const kz_matrix* query, int64_t q0, const int* fail_list, const int* fail_count,
                          const kz_matrix* index, int k, int exclude_self, const int64_t* d_self_ids, double* out_dist, int64_t* out_ind) {
    const int k_eff = k + (exclude_self ? 1 : 0);
    KzExactSelection sel;
    int rc = kz_exact_selection(index, k_eff, KZ_SPEC_TWO_LEVEL_FROM, &sel);
    if (rc != KZ_OK) return rc;
    if (!sp.vals.get()) {   // (not allocated ahead by the caller: kz_spec_alloc)
        rc = kz_spec_alloc(ctx, sp, R, index, k_eff);
        if (rc != KZ_OK || !sp.vals.get()) return rc;
    }
    KzExactLaunch ln;
    ln.dyn_n = fail_count;
    // (one pair per lane from ~4 workgroups of 64 index rows per CU on: on a 15 k-row index its 235 workgroups run one per CU, all
    //  latency -- 73 us against the cooperative kernel's 60.  Where it applies: a pass over a 500 k x 200 index per FOUR rows made the
    //  cooperative kernel 2 ms for 16 rows -- on the critical path behind the forward finalize; 0.3 ms)
    ln.try_lanes = index->dtype == KZ_F32 && index->n >= (int64_t)4 * KZ_XL_ROWS * ctx->n_cus;
    ln.lanes_qd = sp.qd.get();
    // (a handful of rows: short stretches of index rows per wave, so that the launch is wide -- 15 k rows: 235 x R / 4 workgroups)
    const int rpw = (int)(index->n / 1024);
    ln.rows_per_wave = rpw < 16 ? 16 : (rpw > 256 ? 256 : rpw);
    ln.pair_blocks_max = 256;   // (grid-stride; dead rows cost their dispatch)
    ln.two_level_from = KZ_SPEC_TWO_LEVEL_FROM;
    rc = kz_exact_distances(ctx, fail_list, 0, R, q0, query, index, sp.vals.get(), ln);
    if (rc != KZ_OK) return rc;
    kz_exact_select(ctx, sel, fail_list, 0, R, q0, index, k, exclude_self, d_self_ids, sp.vals.get(), sp.cand_v.get(), sp.cand_i.get(), out_dist,
                    out_ind, fail_count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kz_set_error("kz_knn: speculative exact re-search failed to launch: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    sp.R = R;
    return KZ_OK;
}

// (KzResearch -- what a re-search asks of kz_knn_impl -- and kz_research_wide: kz_route.h)

// What every entry point asks of a query / index pair and its two output arrays (`who`: the entry point, as its messages name it)
static int kz_require_pair(const char* who, const kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index,
                           const void* out0, const void* out1) {
    KZ_REQUIRE(ctx && query && index && out0 && out1, "%s: null argument", who);
    KZ_REQUIRE(query->ctx == ctx && index->ctx == ctx, "%s: matrices belong to a different context", who);
    KZ_REQUIRE(!query->raw_only && !index->raw_only, "%s: a rows-only matrix (kz_matrix_create rows_on_device = 3) cannot be searched", who);
    {   // (a precomputed distance matrix: the two views of one storage, whose extents differ -- the feature test is not theirs)
        const int rcv = kz_precomputed_require_pair(who, query, index);
        if (rcv != KZ_OK) return rcv;
    }
    KZ_REQUIRE(query->pre || query->d == index->d, "%s: feature dimensions differ (%lld vs %lld)", who, (long long)query->d, (long long)index->d);
    KZ_REQUIRE(query->dtype == index->dtype, "%s: query and index must have the same dtype", who);
    KZ_REQUIRE(query->metric == index->metric && query->mink_p == index->mink_p, "%s: query and index were packed for different metrics", who);
    KZ_REQUIRE(kz_metric_params_match(query, index), "%s: seuclidean needs the same V (kz_matrix_set_seuclidean_v) on query and index", who);
    KZ_REQUIRE(q_begin >= 0 && q_count >= 0 && q_begin + q_count <= query->n, "%s: query row range out of bounds", who);
    // (device values of a precomputed matrix: the validation kernel's verdict, read by the first call on the pair -- every entry point
    //  comes through here, and the kernels behind all of them assume finite values >= 0)
    if (query->pre) return kz_precomputed_check(query->ctx, query->pre);
    return KZ_OK;
}

// KZ_PRECOMPUTED: the exact stage ALONE, entered before kz_knn_impl derives any list geometry or scratch size (a view has no tiles,
// no k-groups and no operand image to derive them from): the value batch (kz_exact_distances -> kz_precomputed.hip), the one- or
// two-level selection, kz_emit_sorted -- the values come back as they are (kz_output_distance), ordered by (value, index row).
// Any k <= min(index.n, KZ_EXACT_MAX_K).  Ends synchronised with the stream.
static int kz_knn_precomputed(kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, int k, double* d_dist,
                              int64_t* d_ind, kz_knn_stats* stats) {
    if (k > KZ_EXACT_MAX_K) {
        kz_set_error("kz_knn: k=%d exceeds the supported maximum of %d neighbours per query", k, KZ_EXACT_MAX_K);
        return KZ_ERR_UNSUPPORTED;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    // (released when this function ends, stream-ordered: fl, cand_v, cand_i)
    KzPoolBuf<int> cand_i;
    KzPoolBuf<double> cand_v;
    KzPoolBuf<int> fl;   // every row of the range, as the row list the exact stage takes
    int rc = fl.alloc(ctx, (size_t)q_count * sizeof(int));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((q_count + 255) / 256)), dim3(256), 0, ctx->stream, fl.get(), (int)q_count);
    KZ_HIP(hipGetLastError());
    int batch = 0;
    double* vals = nullptr;
    rc = kz_exact_begin(ctx, index, (int)q_count, &batch, &vals);
    if (rc != KZ_OK) return rc;
    // (two levels from TWO chunks on: here EVERY row of the call is selected from its whole value row -- the fallback's default of
    //  five is sized for a handful of rows, where a second launch costs more than one workgroup's k passes over a short row;
    //  15 k x 15 k, k = 10: the one-level kernel was 3.6 of the call's 4.3 ms.  Not for long lists: k survivors per chunk of 4 096
    //  thin nothing out once k is a large share of the chunk)
    KzExactSelection sel;
    rc = kz_exact_selection(index, k, k <= KZ_EXACT_CHUNK / 8 ? 2 : KzExactLaunch().two_level_from, &sel);
    if (rc != KZ_OK) return rc;
    if (sel.two_level) {
        rc = cand_v.alloc(ctx, sel.cand_entries(batch) * 8);
        if (rc == KZ_OK) rc = cand_i.alloc(ctx, sel.cand_entries(batch) * 4);
        if (rc != KZ_OK) return rc;
    }
    for (int b0 = 0; b0 < (int)q_count; b0 += batch) {
        const int nb = (int)q_count - b0 < batch ? (int)q_count - b0 : batch;
        rc = kz_exact_distances(ctx, fl.get(), b0, nb, q_begin, query, index, vals);
        if (rc != KZ_OK) return rc;
        kz_exact_select(ctx, sel, fl.get(), b0, nb, q_begin, index, k, 0, nullptr, vals, cand_v.get(), cand_i.get(), d_dist, d_ind);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[4], ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        kz_set_error("kz_knn: exact kernels on a precomputed matrix failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    if (stats) {
        float ms = 0;
        KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
        stats->fallback_ms = ms;
        stats->n_fallback_rows = q_count;
        stats->first_pass = 0;
    }
    return KZ_OK;
}

static int kz_knn_impl(kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, int k,
                       int exclude_self, const int64_t* d_self_ids, KzResearch rs, double* d_dist,
                       int64_t* d_ind, kz_knn_stats* stats, KzDualPass* dual);
static int kz_escalate_rows(kz_ctx* ctx, kz_matrix* query, int64_t cq_begin, const int* fail_list, int n_fail, kz_matrix* index, int k,
                            int exclude_self, const int64_t* d_self_ids, KzResearch rs, double* out_dist,
                            int64_t* out_ind, kz_knn_stats* st2, float* ms_out, const int* out_rows = nullptr) {
    // (out_rows: where the results of row i of the list go -- row out_rows[i] of out_dist / out_ind instead of the row's own place)
    KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    const size_t row_bytes = (size_t)query->d * kz_elem_size(query->dtype);
    // (released when the function returns: qsub, fl, sub_raw, sub_self, sub_dist, sub_ind)
    KzPoolBuf<int64_t> sub_ind;
    KzPoolBuf<double> sub_dist;
    KzPoolBuf<int64_t> sub_self;
    KzPoolBuf<void> sub_raw;
    KzPoolBuf<int> fl;
    KzMatrixPtr qsub;
    int rc = fl.alloc(ctx, (size_t)n_fail * sizeof(int));
    if (rc == KZ_OK) rc = sub_raw.alloc(ctx, (size_t)n_fail * row_bytes);
    if (rc == KZ_OK && exclude_self) rc = sub_self.alloc(ctx, (size_t)n_fail * 8);
    if (rc == KZ_OK) rc = sub_dist.alloc(ctx, (size_t)n_fail * k * 8);
    if (rc == KZ_OK) rc = sub_ind.alloc(ctx, (size_t)n_fail * k * 8);
    if (rc != KZ_OK) return rc;
    hipError_t e = hipMemcpyAsync(fl.get(), fail_list, (size_t)n_fail * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kz_gather_rows_kernel, dim3(n_fail), dim3(256), 0, ctx->stream, (const char*)query->raw, fl.get(), cq_begin,
                           n_fail, (int64_t)row_bytes, (char*)sub_raw.get(), sub_self.get(), d_self_ids);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        kz_set_error("kz_knn: gathering the escalated rows failed: %s", hipGetErrorString(e));
        return KZ_ERR_HIP;
    }
    kz_matrix* qsub_new = nullptr;
    rc = kz_matrix_create(ctx, sub_raw.get(), 2, n_fail, query->d, query->dtype, query->metric, &qsub_new);
    qsub.reset(qsub_new);
    memset(st2, 0, sizeof(*st2));
    if (rc == KZ_OK)
        rc = kz_knn_impl(ctx, qsub.get(), 0, n_fail, index, k, exclude_self, sub_self.get(), rs, sub_dist.get(), sub_ind.get(), st2, nullptr);
    if (rc == KZ_OK) {
        hipLaunchKernelGGL(kz_scatter_rows_kernel, dim3((unsigned)(((int64_t)n_fail * k + 255) / 256)), dim3(256), 0, ctx->stream,
                           sub_dist.get(), sub_ind.get(), out_rows ? out_rows : fl.get(), n_fail, k, out_dist, out_ind);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ctx->ev[4], ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            kz_set_error("kz_knn: scattering the escalated rows failed: %s", hipGetErrorString(e));
            rc = KZ_ERR_HIP;
        }
    }
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipEventElapsedTime(ms_out, ctx->ev[3], ctx->ev[4]));
    return KZ_OK;
}

// d_self_ids (device, optional): index row to strip per query when exclude_self is set and the query matrix is not the
// index matrix itself (escalated subsets).  rs: what a re-search asks for (KzResearch).  Escalated subsets of the fp16 tier are
// first re-done with LONGER lists on the same operand images (rs.min_kp): the certification compares the K'-th approximate key with
// the k-th exact one, so more margin in ranks is usually all a failed row needs, and unlike the float32 tier it costs no new image
// of the index.
// LADDER AFTER THE FACT (round 5).  A pass that leaves MORE THAN HALF of its rows uncertified without a tier probe having looked at
// the data first (searches below the probe's size gates; tools/cliff_probe.py: 100k x 101k x 128, tight clusters, 60 - 100 ms
// against 5.6 on uniform rows) used to hand all of them to the split-bf16 operands, where rows of a tight cluster fail again --
// what they lack is margin in ranks.  Now a strided sample of the failed rows goes through the fp16 tier's WIDE route first (their
// results are final either way); at most a quarter of the sample uncertified there: every failed row takes that route, else the
// caller's choice (rs).  Fewer than 4096 failed rows: the caller's choice at once.
__global__ void kz_strided_pick_kernel(const int* __restrict__ in, int n_out, int64_t stride, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_out) out[i] = in[(int64_t)i * stride];
}
static int kz_escalate_ladder(kz_ctx* ctx, kz_matrix* query, int64_t cq_begin, const int* fail_list, int n_fail, kz_matrix* index, int k,
                              int exclude_self, const int64_t* d_self_ids, KzResearch rs, double* out_dist, int64_t* out_ind,
                              kz_knn_stats* st, float* ms_out) {
    float ms_probe = 0;
    // (the wide route wants at least 8 index tiles per list: a small index gets fewer lists, down to 8 -- 128 entries per query)
    int P = ctx->wide_lists;
    if ((int64_t)index->n_tiles < (int64_t)8 * P) P = (int)(index->n_tiles / 8);
    KzPoolBuf<int> keep;   // (the caller's list lives in the pass's scratch block, which the probe's own search reuses: a private copy)
    if (P >= 8 && ctx->esc_ladder && n_fail >= 4096) {
        const int n_probe = 1024;
        KzPoolBuf<int> plist;
        int rc = plist.alloc(ctx, (size_t)n_probe * sizeof(int));
        if (rc == KZ_OK) rc = keep.alloc(ctx, (size_t)n_fail * sizeof(int));
        if (rc != KZ_OK) return rc;
        if (hipMemcpyAsync(keep.get(), fail_list, (size_t)n_fail * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            kz_set_error("kz_knn: copying the list of uncertified rows failed");
            return KZ_ERR_HIP;
        }
        hipLaunchKernelGGL(kz_strided_pick_kernel, dim3((n_probe + 255) / 256), dim3(256), 0, ctx->stream, keep.get(), n_probe, (int64_t)(n_fail / n_probe),
                           plist.get());
        kz_knn_stats stw;
        memset(&stw, 0, sizeof(stw));
        rc = kz_escalate_rows(ctx, query, cq_begin, plist.get(), n_probe, index, k, exclude_self, d_self_ids, kz_research_wide(P), out_dist, out_ind,
                              &stw, &ms_probe);
        plist.reset();
        if (rc != KZ_OK) return rc;
        if (stw.wide_lists > 0 && (int64_t)stw.n_first_pass_fail * 4 <= n_probe) rs = kz_research_wide(P);
        fail_list = keep.get();
    }
    const int rc = kz_escalate_rows(ctx, query, cq_begin, fail_list, n_fail, index, k, exclude_self, d_self_ids, rs, out_dist, out_ind, st, ms_out);
    if (ms_out) *ms_out += ms_probe;
    return rc;
}

#include "kz_range.h"

// ---------------------------------------------------------------------------------------------------
// kz_knn_impl.  The route of a call is DECIDED in kz_route.h (pure: KzRouteIn, KzResearch -> KzRoute, KzAfterPass) and EXECUTED by
// the stages below, which kz_knn_impl runs in sequence: lists and tier, the routes of lists of 16 on the dealt image, the tier
// probe, then per chunk of query rows: plan, sweep, finalize, read-back, and the way down for the rows left uncertified.
// ---------------------------------------------------------------------------------------------------
// The arguments of one kz_knn_impl call, as every stage reads them (none of them changes during the call).
struct KzCall {
    kz_ctx* ctx;
    kz_matrix* query;
    int64_t q_begin, q_count;
    kz_matrix* index;
    int k, exclude_self;
    const int64_t* d_self_ids;
    double* d_dist;
    int64_t* d_ind;
    KzDualPass* dual;
};
// The tallies of one call (kz_knn_stats without the route fields).
struct KzTally {
    double main_ms = 0, fin_ms = 0, fb_ms = 0;
    float probe_ms = 0;   // (tier probe: reported under its own field, kz_knn_stats.probe_ms)
    int64_t n_fail_total = 0, n_escalated = 0, n_first_fail = 0, n_spec = 0, n_range = 0, n_range_pairs = 0, n_range_group = 0;
    double max_err_ratio = 0.0;
    int last_splits = 1, last_blocks = 0;
    void add(const kz_knn_stats& s) {   // a sub-search's (its own escalated rows, and what it sent further down)
        n_escalated += s.n_escalated_rows;
        n_fail_total += s.n_fallback_rows;
        n_range += s.n_range_rows;
        n_range_pairs += s.n_range_pairs;
        n_range_group += s.n_range_group_rows;
        if (s.max_err_ratio > max_err_ratio) max_err_ratio = s.max_err_ratio;
    }
    void write(kz_knn_stats* st) const {
        st->main_kernel_ms = main_ms;
        st->finalize_ms = fin_ms;
        st->fallback_ms = fb_ms;
        st->probe_ms = probe_ms;
        st->n_fallback_rows = n_fail_total;
        st->n_splits = last_splits;
        st->n_blocks = last_blocks;
        st->n_escalated_rows = n_escalated;
        st->max_err_ratio = max_err_ratio;
        st->n_first_pass_fail = n_first_fail > 0x7fffffff ? 0x7fffffff : (int32_t)n_first_fail;
        st->n_spec_rows = n_spec > 0x7fffffff ? 0x7fffffff : (int32_t)n_spec;
        st->n_range_rows = n_range;
        st->n_range_pairs = n_range_pairs;
        st->n_range_group_rows = n_range_group;
    }
};
// One chunk of the call's query rows: one launch of the tier's kernel.
struct KzChunk {
    int64_t cq_begin, cq_count;
    int qt0, n_qtiles, force_pieces;
    KzPlan pl;
};

static KzRouteIn kz_route_in(const KzCall& c, int k_eff) {
    const kz_ctx* ctx = c.ctx;
    KzRouteIn in;
    in.n_tiles = c.index->n_tiles;
    in.n = c.index->n;
    in.kg = c.index->kg;
    // (slices of the fp16 image: kz_h_nsr pads 32 .. 64 to a multiple of 8 and 65 .. 128 to a multiple of 16 -- the other tiers never
    //  read n_slices beyond 24)
    in.n_slices = kz_h_nsr(c.index->kg);
    in.gemm_form = c.index->metric < KZ_MANHATTAN;
    in.same_kg = c.query->kg == c.index->kg;
    in.range_ok = kz_range_shapes_ok(ctx, c.query, c.index);
    in.k_eff = k_eff;
    in.dual = c.dual != nullptr;
    in.precision = ctx->precision;
    in.esc_bf = ctx->esc_bf;
    in.short_ord = ctx->short_ord;
    in.short_ord_min_tiles = ctx->short_ord_min_tiles;
    in.wide_lists = ctx->wide_lists;
    in.wide_sel = ctx->wide_sel;
    in.tier_probe = ctx->tier_probe;
    in.chunk_rows = ctx->chunk_rows;
    in.probe_min_pairs = ctx->probe_min_pairs;
    if (c.dual) {
        in.short_pieces = c.dual->short_pieces;
        in.short_ksel = c.dual->short_ksel;
        in.short_kp = c.dual->short_kp;
        in.dual_probed = c.dual->probed != 0;
    }
    return in;
}

// The wide route with P lists, if its geometry allows (KZ_ERR_UNSUPPORTED) and the dealt image can be had (KZ_ERR_NOMEM).
static int kz_take_wide(kz_matrix* index, const KzRouteIn& in, KzRoute* route, int P) {
    int sel = 0;
    if (!kz_route_wide_geometry(in, *route, P, &sel)) return KZ_ERR_UNSUPPORTED;
    const int rc = kz_himage_dealt(index, P);
    if (rc != KZ_OK) return rc;
    kz_route_take_dealt(route, P, sel, true);
    return KZ_OK;
}

// TIER PROBE (kz_route.h: kz_probe_wanted has said yes): a strided sample of the query rows through the fp16 pass, its verdict applied
// to the route; on data that is fine, the population floor of the seeded lists from the sample's results (*qfloor_ord).
static int kz_tier_probe(const KzCall& c, const KzRouteIn& in, KzRoute* route, float** qfloor_ord, float* probe_ms) {
    kz_ctx* ctx = c.ctx;
    const int n_probe = ctx->tier_probe;
    KzPoolBuf<int> plist;
    int rc = plist.alloc(ctx, (size_t)n_probe * sizeof(int));
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL(kz_strided_rows_kernel, dim3((unsigned)((n_probe + 255) / 256)), dim3(256), 0, ctx->stream, plist.get(), n_probe,
                       c.q_count / n_probe);
    kz_knn_stats stp;
    float pms = 0;
    KzResearch probe_rs;
    probe_rs.prec = 0;
    rc = kz_escalate_rows(ctx, c.query, c.q_begin, plist.get(), n_probe, c.index, c.k, c.exclude_self, c.d_self_ids, probe_rs, c.d_dist, c.d_ind, &stp,
                          &pms);
    if (rc != KZ_OK) return rc;
    *probe_ms = pms;
    const KzProbeVerdict verdict = kz_probe_verdict(n_probe, stp.n_first_pass_fail, ctx->wide_lists);
    bool hard = verdict.hard;
    if (verdict.try_wide) {
        int sel = 0;
        if (kz_route_wide_geometry(in, *route, ctx->wide_lists, &sel)) {
            kz_knn_stats stw;
            float wms = 0;
            rc = kz_escalate_rows(ctx, c.query, c.q_begin, plist.get(), n_probe, c.index, c.k, c.exclude_self, c.d_self_ids,
                                  kz_research_wide(ctx->wide_lists), c.d_dist, c.d_ind, &stw, &wms);
            if (rc != KZ_OK) return rc;
            *probe_ms += wms;
            if (kz_probe_wide_wins(n_probe, stp.n_first_pass_fail, stw.n_first_pass_fail) && kz_take_wide(c.index, in, route, ctx->wide_lists) == KZ_OK)
                hard = false;
        }
    }
    plist.reset();
    if (hard) {
        kz_route_start_hard(in, route);
    } else if (ctx->list_floor && !route->wide_route) {
        // POPULATION FLOOR (above kz_escalate_rows): the probe's results are the model's input
        double model[3];
        bool ok = false;
        rc = kz_floor_model(ctx, c.d_dist, c.query->himg->rowq + c.q_begin * 3, n_probe, c.q_count / n_probe, c.k, c.index->metric, model, &ok);
        if (rc != KZ_OK) return rc;
        const int64_t n_pad = (int64_t)c.query->n_tiles * KZ_TILE;
        if (ok) rc = kz_floor_buf(ctx, (size_t)n_pad * 4, qfloor_ord);
        if (rc != KZ_OK) return rc;
        if (*qfloor_ord) {
            hipLaunchKernelGGL(kz_floor_rows_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, ctx->stream, (const int*)nullptr, c.query->n,
                               n_pad, c.query->himg->rowq, c.index->himg->d_max, c.index->himg->center->d_scale, model[0], model[1], model[2],
                               ctx->eps_scale, kz_gamma_acc_h(c.index->kg), *qfloor_ord);
            KZ_HIP(hipGetLastError());
        }
    }
    return KZ_OK;
}

// 64 QUERIES PER WAVE (kz_knn_h64.h): K' = 16 sweeps of 4 .. 13 slices -- half the LDS fragment reads per MFMA and half the
// LDS-DMA volume per query of the 32-query kernel at two waves per SIMD instead of three; a work item = a unit of two query
// tiles (tpw = 2).  Measured (profiles/r04_ablation.md section 2): the shared sweep at 13 slices -1.5 % (250k x 1M x 200: 90.6 ->
// 89.2 ms), the ordinary kernel +0.8 % there, +8 % at 8 slices, and a launch of fewer than ~4 rounds of units does not fill the
// chip (100k x 100k: +30 %).  Option "h_q64": 2 (default) = the shared sweep from 9 slices on over >= 4 rounds of units,
// 1 = wherever the kernel is built for (tests), 0 = never.
static int kz_q64_wanted(const KzCall& c, const KzRoute& route, int n_slices, bool* q64) {
    const kz_ctx* ctx = c.ctx;
    const KzDualPass* dual = c.dual;
    bool q64_ok = false;
    if (route.tier == KZ_TIER_H && route.cur.KP == 16 && !route.exact_only) {   // (is there a 64-query build for these rows?  The resolver may come back empty)
        KzSweepKernel k64;
        const int rc = kz_sweep_kernel(KZ_TIER_H, dual != nullptr, true, route.cur.KP, n_slices, &k64, true);
        if (rc != KZ_OK) return rc;
        q64_ok = k64.fn != nullptr;
    }
    *q64 = q64_ok && !(dual && dual->no_q64) && (ctx->h_q64 == 1 || (ctx->h_q64 == 2 && dual && n_slices >= 9 &&
                                                 (c.q_count + 2 * KZ_TILE - 1) / (2 * KZ_TILE) >= (int64_t)4 * 2 * ctx->n_cus));
    return KZ_OK;
}

// The operand images the chunk's tier sweeps (built on first use).
static int kz_tier_images(const KzCall& c, const KzResearch& rs, const KzRoute& route) {
    if (route.tier == KZ_TIER_BF) {
        int rc = kz_matrix_image_bf(c.query);
        if (rc == KZ_OK) rc = kz_matrix_image_bf(c.index);
        if (rc != KZ_OK) return rc;
    } else if (route.tier == KZ_TIER_F32 && !route.exact_only) {
        int rc = kz_matrix_image_f32(c.query);
        if (rc == KZ_OK) rc = kz_matrix_image_f32(c.index);
        if (rc != KZ_OK) return rc;
    }
    if (route.tier == KZ_TIER_H && route.short_ord && route.cur.pieces >= 2) {
        // (a re-search of the previous chunk's uncertified rows may have selected -- or packed -- the index dealt over another
        //  number of ranges: this route's own image again; cached, two are kept)
        // (any failure ends the call: launching on whatever image the last sub-search selected would certify against the wrong
        //  range layout; unreachable while a slot exists once the route is chosen)
        const int rcd = kz_himage_dealt(c.index, route.wide_route || rs.wide_lists > 0 ? route.cur.pieces : route.route_P);
        if (rcd != KZ_OK) {
            if (rcd == KZ_ERR_NOMEM) kz_set_error("kz_knn: out of device memory for the row-dealt image of the index");
            return rcd;
        }
    }
    return KZ_OK;
}

// ---- schedule: which workgroup sweeps which (query tile, index-tile range): kz_prepare_pass above --------------
// The chunk that starts at row c0 of the call and its plan; *max_rows_per_chunk is halved where a chunk's lists would pass 2^32 entries.
static void kz_chunk_plan(const KzCall& c, const KzRoute& route, int slots, int tpw_h, int n_ytiles, int64_t c0, int64_t* max_rows_per_chunk,
                          KzChunk* ch) {
    const KzDualPass* dual = c.dual;
    const int tier = route.tier, KP = route.cur.KP;
    ch->cq_begin = c.q_begin + c0;
    ch->qt0 = (int)(ch->cq_begin / KZ_TILE);
    for (;;) {
        ch->cq_count = (c.q_count - c0 < *max_rows_per_chunk) ? (c.q_count - c0) : *max_rows_per_chunk;
        ch->n_qtiles = (int)((ch->cq_begin + ch->cq_count - 1) / KZ_TILE) - ch->qt0 + 1;
        ch->force_pieces = kz_route_sub_pieces(route, (ch->n_qtiles + tpw_h - 1) / tpw_h, slots, n_ytiles);
        int max_pieces = kz_max_pieces(KP, tier == KZ_TIER_F32 ? 2 : 1);
        if (dual && dual->max_entries > 0 && max_pieces > dual->max_entries / KP) max_pieces = dual->max_entries / KP;
        // The kernels address a launch's lists with 32-bit element offsets: a chunk whose plan would pass 2^32 entries (K' = 16,
        // 2 M rows over 128 ranges) is halved.
        kz_plan_tier_pass(c.ctx, ch->n_qtiles, n_ytiles, slots, max_pieces, KP, tier, tier == KZ_TIER_H ? tpw_h : 1, ch->force_pieces,
                          route.min_pieces_call, &ch->pl);
        if (ch->pl.list_elems < ((size_t)1 << 32) || ch->cq_count <= 8 * KZ_TILE || (dual && dual->raw_lists)) break;
        *max_rows_per_chunk = ((ch->cq_count / 2 + KZ_TILE - 1) / KZ_TILE) * KZ_TILE;
    }
}

// The chunk's sweep, between ev[0] and the caller's ev[1]: the dual build, the range-0 boot, the plain launch (and its two diagnostic
// variants), or -- exact-only -- the list of every row.  boot_floor: this chunk's range-0 floor, if any (the finalize kernel must
// know it); stamp_buf: diagnostic "abl_stamp".
static int kz_chunk_sweep(const KzCall& c, const KzRoute& route, const KzSweepKernel& kern, const KzChunk& ch, const KzPass& ps, bool q64, bool boot,
                          const float* qfloor_ord, int n_ytiles, KzPoolBuf<float>& boot_floor, KzPoolBuf<unsigned long long>& stamp_buf) {
    kz_ctx* ctx = c.ctx;
    kz_matrix *query = c.query, *index = c.index;
    const KzDualPass* dual = c.dual;
    const int tier = route.tier, KP = route.cur.KP, W = ps.W;
    const bool short_ord = route.short_ord;
    int rc = KZ_OK;
    KnnCandParams cp;
    memset(&cp, 0, sizeof(cp));
    if (tier == KZ_TIER_H) {
        cp.qpack = (const float*)query->himg->packed;
        cp.ypack = (const float*)(short_ord ? index->himg->dealt_packed : index->himg->packed);
        cp.ybias = short_ord ? index->himg->dealt_bias : index->himg->bias;
    } else {
        cp.qpack = tier == KZ_TIER_BF ? (const float*)query->packed_bf : query->packed;
        cp.ypack = tier == KZ_TIER_BF ? (const float*)index->packed_bf : index->packed;
        cp.ybias = index->bias;
    }
    cp.work = ps.d_work;
    cp.qt0 = ch.qt0;
    cp.n_ytiles = n_ytiles;
    cp.n_qtiles = ch.n_qtiles;
    cp.lay = ps.lay;
    cp.kg = index->kg;
    cp.out_key = ps.out_key;
    cp.out_idx = ps.out_idx;
    if (tier == KZ_TIER_H && !dual) cp.qfloor = qfloor_ord;
    KZ_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    if (route.exact_only) {
        // every row of the chunk goes to the exact kernels: the "fail list" is 0 .. cq_count-1
        hipLaunchKernelGGL(kz_iota_kernel, dim3((unsigned)((ch.cq_count + 255) / 256)), dim3(256), 0, ctx->stream, ps.fail_list, (int)ch.cq_count);
        KZ_HIP(hipGetLastError());
    } else if (tier == KZ_TIER_H && dual) {
        cp.qpack = dual->qpack;
        cp.ypack = dual->ypack;
        cp.ybias = dual->ybias;
        cp.theta = dual->theta;
        cp.qnbias = dual->qnbias;
        cp.qfloor = dual->qfloor;
        cp.log_keys = dual->log_keys;
        cp.log_meta = dual->log_meta;
        cp.log_cnt = dual->log_cnt;
        cp.log_cap = dual->log_cap;
        rc = kz_sweep_launch(ctx, kern, cp, W);
    } else if (tier == KZ_TIER_H && boot && ps.W0 > 0 && ps.W0 < W) {
        // range 0 of every query tile, the floor off its lists, then the other ranges
        rc = kz_sweep_launch(ctx, kern, cp, ps.W0);
        if (rc != KZ_OK) return rc;
        const int64_t n_pad = (int64_t)query->n_tiles * KZ_TILE;
        rc = boot_floor.alloc(ctx, (size_t)n_pad * 4);   // (a buffer of this chunk: escalated sub-searches boot too)
        if (rc != KZ_OK) return rc;
        hipLaunchKernelGGL(kz_boot_floor_kernel, dim3((unsigned)((ch.cq_count + 255) / 256)), dim3(256), 0, ctx->stream, ps.out_key, ps.out_idx, ps.lay,
                           KP, ch.cq_begin - (int64_t)ch.qt0 * KZ_TILE, ch.cq_begin, ch.cq_count, cp.qfloor, boot_floor.get());
        KZ_HIP(hipGetLastError());
        cp.qfloor = boot_floor.get();
        cp.work = ps.d_work + ps.W0;
        rc = kz_sweep_launch(ctx, kern, cp, W - ps.W0);
    } else if (tier == KZ_TIER_H && !q64) {
        if ((ctx->abl & 2) && getenv("KZ_STAMP_FILE")) {   // (diagnostic: a -DKZ_ABL_STAMP build of the fp16 units fills it)
            rc = stamp_buf.alloc(ctx, (size_t)W * (16 + 1024));
            if (rc != KZ_OK) return rc;
            KZ_HIP(hipMemsetAsync(stamp_buf.get(), 0, (size_t)W * (16 + 1024), ctx->stream));
            cp.log_meta = stamp_buf.get();
            cp.log_keys = stamp_buf.get() + 2 * (size_t)W;
        }
        rc = kz_sweep_launch(ctx, kern, cp, W);
        cp.log_meta = nullptr;
        cp.log_keys = nullptr;
        if (rc == KZ_OK && (ctx->abl & 1) && !short_ord && ps.lay.n_regions == 1 && ps.lay.pieces[0] == 1) {
            // DIAGNOSTIC ("abl_refloor", profiles/r06_event_ablation.md): the same sweep AGAIN with every list starting at the
            // threshold it ENDED on (the K'-th best key of the first sweep's list): K' insertions per query instead of
            // K' (1 + ln(n / K')) -- the time any seeding of the lists could at best reach.  The second sweep is the one timed.
            const int64_t n_pad = (int64_t)query->n_tiles * KZ_TILE;
            rc = boot_floor.alloc(ctx, (size_t)n_pad * 4);
            if (rc != KZ_OK) return rc;
            hipLaunchKernelGGL(kz_boot_floor_kernel, dim3((unsigned)((ch.cq_count + 255) / 256)), dim3(256), 0, ctx->stream, ps.out_key, ps.out_idx,
                               ps.lay, KP, ch.cq_begin - (int64_t)ch.qt0 * KZ_TILE, ch.cq_begin, ch.cq_count, cp.qfloor, boot_floor.get());
            // (one ulp below: entries equal to the threshold must get in again)
            hipLaunchKernelGGL(kz_floor_nudge_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, ctx->stream, boot_floor.get(), n_pad);
            KZ_HIP(hipGetLastError());
            cp.qfloor = boot_floor.get();
            KZ_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
            rc = kz_sweep_launch(ctx, kern, cp, W);
        }
    } else   // (the 64-query kernel, the split-bf16 and the float32 operands: one plain launch)
        rc = kz_sweep_launch(ctx, kern, cp, W);
    return rc;
}

// The finalize kernel's parameters that every launch fills the same way: the two matrices and -- fp16 tier: qi / ii, the images the
// lists were swept on; nullptr on the other tiers -- the terms of that tier's certification bound.  The lists, the rows and the
// outputs are the caller's.
static KnnFinParams kz_fin_params(const kz_ctx* ctx, const kz_matrix* query, const kz_matrix* index, const kz_himage* qi, const kz_himage* ii, int k) {
    KnnFinParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.qraw = query->raw;
    fp.yraw = index->raw;
    fp.qsqn = query->sqn;
    fp.ysqn = index->sqn;
    fp.n_i = index->n;
    fp.d = (int)index->d;
    fp.metric = index->metric;
    fp.k = k;
    fp.ystats = index->d_stats;
    fp.tier_h = qi ? 1 : 0;
    if (fp.tier_h) {
        fp.eps_mult = ctx->eps_scale;
        fp.gamma_acc = kz_gamma_acc_h(index->kg);
        fp.q_rowq = qi->rowq;
        fp.y_hmax = ii->d_max;
        fp.hscale = ii->center->d_scale;
    }
    return fp;
}

// The chunk's finalize launch (none for an exact-only call or a raw-list pass) and the parameters it ran with, which the stages behind
// it read (*fp: where results go, the fail list).  c0: first row of the chunk in the call; gamma: the tier's a-priori bound factor;
// list_floor: what the lists of an ordinary fp16 sweep started at (range-0 floor, else the population floor, else nullptr).
static int kz_chunk_finalize(const KzCall& c, const KzRoute& route, const KzChunk& ch, const KzPass& ps, int64_t c0, double gamma,
                             const float* list_floor, KnnFinParams* out) {
    kz_ctx* ctx = c.ctx;
    kz_matrix *query = c.query, *index = c.index;
    const KzDualPass* dual = c.dual;
    const int tier = route.tier, KP = route.cur.KP;
    KnnFinParams fp = kz_fin_params(ctx, query, index, tier == KZ_TIER_H ? query->himg : nullptr, tier == KZ_TIER_H ? index->himg : nullptr, c.k);
    fp.in_key = ps.out_key;
    fp.in_idx = ps.out_idx;
    fp.lay = ps.lay;
    fp.KP = KP;
    fp.KSEL = route.cur.KSEL;
    fp.list_row0 = ch.cq_begin - (int64_t)ch.qt0 * KZ_TILE;
    fp.q_begin = ch.cq_begin;
    fp.q_count = ch.cq_count;
    fp.exclude_self = c.exclude_self ? 1 : 0;
    fp.self_ids = c.d_self_ids;
    fp.gamma = gamma;
    fp.out_dist = c.d_dist + c0 * (int64_t)c.k;
    fp.out_ind = c.d_ind + c0 * (int64_t)c.k;
    if (tier == KZ_TIER_H && route.short_ord) fp.idx_map = index->himg->dealt_perm;   // the lists hold rows of the dealt index image
    if (tier == KZ_TIER_H && !dual) fp.list_floor = list_floor;
    if (tier == KZ_TIER_H && dual) {
        fp.idx_map = dual->perm;      // the lists hold rows of the sorted index image
        fp.row_map = dual->row_map;   // the chunk is a range of IMAGE rows: results and failures go by matrix row
        fp.list_floor = dual->qfloor;
        fp.out_dist = c.d_dist;
        fp.out_ind = c.d_ind;
    }
    fp.fail_count = ctx->d_counters + 8;
    fp.fail_list = ps.fail_list;
    fp.fail_tau = ps.fail_tau;
    fp.err_ratio_bits = (unsigned long long*)(ctx->d_counters + 10);
    if (fp.tier_h && index->metric == KZ_COSINE && (fp.KSEL > 0 ? fp.KSEL : KP) > 160 && !(dual && dual->raw_lists)) {
        // (hundreds of re-ranked candidates per query: the normalised float64 rows of the index, built once -- kz_pack.hip)
        const int rc = kz_matrix_norm64(index);
        if (rc != KZ_OK) return rc;
        fp.ynorm64 = index->norm64;
    }
    *out = fp;
    if (!route.exact_only && !(dual && dual->raw_lists))   // (raw lists: the caller's hook has read them; nothing is finalized)
        return kz_launch_finalize(ctx, *out, ps.lay, KP, ch.cq_count, index->dtype);
    return KZ_OK;
}

// Test hook (kiez_amd.h; tests/test_gpu_finalize_direct.py): the finalize launch of a pass on lists the caller wrote.  Parameters by
// kz_fin_params, launch by kz_launch_finalize, as kz_chunk_finalize above; everything the kernels index with is checked here first.
extern "C" int kz_selftest_finalize(kz_ctx* ctx, kz_matrix* query, kz_matrix* index, kz_selftest_fin* t) {
    KZ_REQUIRE(ctx && query && index && t && query->ctx == ctx && index->ctx == ctx, "kz_selftest_finalize: null argument / foreign matrix");
    for (const kz_matrix* x : {(const kz_matrix*)query, (const kz_matrix*)index}) {
        KZ_REFUSE_PRECOMPUTED("kz_selftest_finalize", x);
        KZ_REQUIRE(!x->raw_only && x->metric <= KZ_COSINE, "kz_selftest_finalize: searchable matrices of the euclidean family or cosine only");
    }
    KZ_REQUIRE(query->d == index->d && query->metric == index->metric && query->dtype == index->dtype,
               "kz_selftest_finalize: the matrices must share width, metric and element type");
    KZ_REQUIRE(t->h_key && t->h_idx && t->h_out_dist && t->h_out_ind && t->h_fail_list && t->h_fail_tau, "kz_selftest_finalize: null array");
    const int KP = t->KP, k_eff = t->k + (t->exclude_self ? 1 : 0), KS = t->KSEL > 0 ? t->KSEL : KP;
    KZ_REQUIRE(KP == 16 || KP == 32 || KP == 64 || KP == 128, "kz_selftest_finalize: lists of %d entries", KP);
    KZ_REQUIRE(t->k >= 1 && k_eff <= KZ_EXACT_MAX_K && t->KSEL >= 0 && t->KSEL <= KZ_FIN_MAXM && KS >= k_eff,
               "kz_selftest_finalize: k=%d (+ self) against %d selected candidates", t->k, KS);
    KZ_REQUIRE(t->tier == KZ_TIER_F32 || t->tier == KZ_TIER_H, "kz_selftest_finalize: tier %d", t->tier);
    KZ_REQUIRE(t->tier == KZ_TIER_H || (t->gamma >= 0.0 && t->gamma < INFINITY), "kz_selftest_finalize: gamma must be finite and non-negative");
    KZ_REQUIRE(t->tier != KZ_TIER_H || (t->contig == 1 && kz_h_slices_ok(index->kg)),
               "kz_selftest_finalize: the fp16 tier needs contiguous lists and a width with an fp16 image (d=%lld)", (long long)index->d);
    KZ_REQUIRE((t->contig == 0 || t->contig == 1) && (t->halves == 1 || t->halves == 2) && t->n_regions >= 1 && t->n_regions <= KZ_MAX_REGIONS,
               "kz_selftest_finalize: layout with %d regions, %d halves, contig=%d", t->n_regions, t->halves, t->contig);
    // ---- the layout, its bases as kz_plan_pass lays them out ----
    KzListLayout lay;
    memset(&lay, 0, sizeof(lay));
    lay.n_regions = t->n_regions;
    lay.halves = t->halves;
    lay.contig = t->contig;
    const int entries_per_list = t->contig ? KP : 2 * KP;
    KZ_REQUIRE(t->contig == 0 || t->halves == 1, "kz_selftest_finalize: contiguous lists have one list per query and range");
    int64_t list_elems = 0;
    int max_m = 0;
    for (int r = 0; r < t->n_regions; ++r) {
        const int t0 = r > 0 ? t->qt_end[r - 1] : 0;
        KZ_REQUIRE(t->qt_end[r] > t0 && t->qt_end[r] <= (1 << 16) && t->pieces[r] >= 1 && t->pieces[r] <= KZ_FIN_MAXM,
                   "kz_selftest_finalize: region %d ends at tile %d with %d pieces", r, t->qt_end[r], t->pieces[r]);
        const int m = t->pieces[r] * t->halves * KP;
        KZ_REQUIRE(m <= KZ_FIN_MAXM, "kz_selftest_finalize: %d list entries per query (at most %d)", m, KZ_FIN_MAXM);
        if (m > max_m) max_m = m;
        lay.qt_end[r] = t->qt_end[r];
        lay.pieces[r] = t->pieces[r];
        lay.base[r] = (long long)list_elems;
        list_elems += (int64_t)(t->qt_end[r] - t0) * KZ_TILE * (int64_t)t->pieces[r] * entries_per_list;
    }
    KZ_REQUIRE(t->n_list == list_elems && list_elems < ((int64_t)1 << 28), "kz_selftest_finalize: the layout holds %lld entries, the arrays %lld",
               (long long)list_elems, (long long)t->n_list);
    KZ_REQUIRE(t->q_count >= 1 && t->q_begin >= 0 && t->q_begin + t->q_count <= query->n && t->list_row0 >= 0 &&
                   t->list_row0 + t->q_count <= (int64_t)t->qt_end[t->n_regions - 1] * KZ_TILE,
               "kz_selftest_finalize: rows [%lld, +%lld) at list row %lld", (long long)t->q_begin, (long long)t->q_count, (long long)t->list_row0);
    // ---- every index the kernels read through ----
    // (the wave-interleaved gather stores the list's ids as they are: a map there would be checked here and never applied)
    KZ_REQUIRE(!t->h_idx_map || t->contig == 1, "kz_selftest_finalize: idx_map needs contiguous lists");
    // (the reverse direction's bound is excl_floor and the cut of its ONE list of KP entries: kz_finalize_query counts neither
    //  list_floor nor an evicting list's minimum beside it)
    KZ_REQUIRE(!t->h_excl_floor || (!t->h_list_floor && KS == KP && t->halves == 1 && max_m == KP),
               "kz_selftest_finalize: excl_floor goes with one list of KP entries, all selected, and no list_floor");
    KZ_REQUIRE(!t->h_idx_map || t->n_idx_map >= 1, "kz_selftest_finalize: empty idx_map");
    const int64_t id_end = t->h_idx_map ? (int64_t)t->n_idx_map : index->n;
    for (int64_t e = 0; e < t->n_list; ++e)
        KZ_REQUIRE(t->h_idx[e] >= -1 && t->h_idx[e] < id_end, "kz_selftest_finalize: list entry %lld holds id %d", (long long)e, t->h_idx[e]);
    if (t->h_idx_map)
        for (int i = 0; i < t->n_idx_map; ++i)
            KZ_REQUIRE(t->h_idx_map[i] >= -1 && t->h_idx_map[i] < index->n, "kz_selftest_finalize: idx_map[%d] = %d is no index row", i, t->h_idx_map[i]);
    if (t->h_row_map)
        for (int64_t i = 0; i < query->n; ++i)
            KZ_REQUIRE(t->h_row_map[i] >= 0 && t->h_row_map[i] < query->n, "kz_selftest_finalize: row_map[%lld] = %d is no query row", (long long)i,
                       t->h_row_map[i]);
    if (t->h_self_ids)
        for (int64_t i = 0; i < t->q_count; ++i)
            KZ_REQUIRE(t->h_self_ids[i] >= 0 && t->h_self_ids[i] < index->n, "kz_selftest_finalize: self_ids[%lld] is no index row", (long long)i);
    KZ_HIP(hipSetDevice(ctx->device));
    int rc = kz_matrix_check(query);
    if (rc == KZ_OK) rc = kz_matrix_check(index);
    if (rc != KZ_OK) return rc;
    if (t->tier == KZ_TIER_H) {
        rc = kz_himage_ensure(query, index);
        if (rc != KZ_OK) return rc;
    }
    KnnFinParams fp = kz_fin_params(ctx, query, index, t->tier == KZ_TIER_H ? query->himg : nullptr, t->tier == KZ_TIER_H ? index->himg : nullptr, t->k);
    // (the kernel's build, and with it the LDS a wave needs, follows from the parameters filled so far plus these three)
    fp.KP = KP;
    fp.KSEL = t->KSEL;
    KzPoolBuf<float> d_efloor;
    if (t->h_excl_floor && d_efloor.alloc(ctx, (size_t)query->n * 4) != KZ_OK) {
        kz_set_error("kz_selftest_finalize: out of device memory");
        return KZ_ERR_NOMEM;
    }
    fp.excl_floor = d_efloor.get();   // (kz_fin_build reads whether there is one; filled with the other copies below)
    const int build = kz_fin_build(fp, KP, index->dtype);
    const int wave_bytes = build == KZ_FIN_BUILD_WIDE ? kz_fin_wide_wave_bytes(max_m, KS) : kz_fin_wave_bytes(max_m, KS);
    KZ_REQUIRE(4 * wave_bytes <= KZ_FIN_LDS_BYTES, "kz_selftest_finalize: %d entries, %d selected: %d bytes of LDS", max_m, KS, 4 * wave_bytes);
    // ---- device copies ----
    const int64_t out_rows = t->h_row_map ? query->n : t->q_count;
    const size_t out_n = (size_t)out_rows * (size_t)t->k;
    KzPoolBuf<float> d_key, d_lfloor;
    KzPoolBuf<int> d_idx, d_imap, d_rmap, d_fail;
    KzPoolBuf<int64_t> d_self, d_oind;
    KzPoolBuf<double> d_odist, d_tau;
    bool ok = d_key.alloc(ctx, (size_t)t->n_list * 4) == KZ_OK && d_idx.alloc(ctx, (size_t)t->n_list * 4) == KZ_OK &&
              d_fail.alloc(ctx, (size_t)t->q_count * 4) == KZ_OK && d_tau.alloc(ctx, (size_t)t->q_count * 8) == KZ_OK &&
              d_odist.alloc(ctx, out_n * 8) == KZ_OK && d_oind.alloc(ctx, out_n * 8) == KZ_OK;
    ok = ok && (!t->h_list_floor || d_lfloor.alloc(ctx, (size_t)query->n * 4) == KZ_OK) &&
         (!t->h_idx_map || d_imap.alloc(ctx, (size_t)t->n_idx_map * 4) == KZ_OK) && (!t->h_row_map || d_rmap.alloc(ctx, (size_t)query->n * 4) == KZ_OK) &&
         (!t->h_self_ids || d_self.alloc(ctx, (size_t)t->q_count * 8) == KZ_OK);
    if (!ok) {
        kz_set_error("kz_selftest_finalize: out of device memory");
        return KZ_ERR_NOMEM;
    }
    const hipStream_t st = ctx->stream;
    KZ_HIP(hipMemcpyAsync(d_key.get(), t->h_key, (size_t)t->n_list * 4, hipMemcpyHostToDevice, st));
    KZ_HIP(hipMemcpyAsync(d_idx.get(), t->h_idx, (size_t)t->n_list * 4, hipMemcpyHostToDevice, st));
    if (t->h_list_floor) KZ_HIP(hipMemcpyAsync(d_lfloor.get(), t->h_list_floor, (size_t)query->n * 4, hipMemcpyHostToDevice, st));
    if (t->h_excl_floor) KZ_HIP(hipMemcpyAsync(d_efloor.get(), t->h_excl_floor, (size_t)query->n * 4, hipMemcpyHostToDevice, st));
    if (t->h_idx_map) KZ_HIP(hipMemcpyAsync(d_imap.get(), t->h_idx_map, (size_t)t->n_idx_map * 4, hipMemcpyHostToDevice, st));
    if (t->h_row_map) KZ_HIP(hipMemcpyAsync(d_rmap.get(), t->h_row_map, (size_t)query->n * 4, hipMemcpyHostToDevice, st));
    if (t->h_self_ids) KZ_HIP(hipMemcpyAsync(d_self.get(), t->h_self_ids, (size_t)t->q_count * 8, hipMemcpyHostToDevice, st));
    // (all-ones bytes: a NaN distance, id -1, row -1, a NaN tau wherever the kernels write nothing)
    KZ_HIP(hipMemsetAsync(d_odist.get(), 0xFF, out_n * 8, st));
    KZ_HIP(hipMemsetAsync(d_oind.get(), 0xFF, out_n * 8, st));
    KZ_HIP(hipMemsetAsync(d_fail.get(), 0xFF, (size_t)t->q_count * 4, st));
    KZ_HIP(hipMemsetAsync(d_tau.get(), 0xFF, (size_t)t->q_count * 8, st));
    int* fail_count = ctx->d_counters + 8;
    KZ_HIP(hipMemsetAsync(fail_count, 0, 4 * sizeof(int), st));   // fail counter, (unused), error-ratio bits
    KZ_HIP(hipStreamSynchronize(st));   // (the host arrays are the caller's pageable buffers)
    // ---- the rest of the parameters, field by field as kz_chunk_finalize fills them ----
    fp.in_key = d_key.get();
    fp.in_idx = d_idx.get();
    fp.lay = lay;
    fp.list_row0 = t->list_row0;
    fp.q_begin = t->q_begin;
    fp.q_count = t->q_count;
    fp.exclude_self = t->exclude_self ? 1 : 0;
    fp.self_ids = d_self.get();
    fp.gamma = t->gamma;
    fp.out_dist = d_odist.get();
    fp.out_ind = d_oind.get();
    fp.idx_map = d_imap.get();
    fp.row_map = d_rmap.get();
    fp.list_floor = d_lfloor.get();
    fp.excl_floor = d_efloor.get();
    fp.dual_col = t->dual_col ? 1 : 0;
    fp.fail_count = fail_count;
    fp.fail_list = d_fail.get();
    fp.fail_tau = d_tau.get();
    fp.err_ratio_bits = (unsigned long long*)(ctx->d_counters + 10);
    if (fp.tier_h && index->metric == KZ_COSINE && KS > 160) {   // (kz_chunk_finalize's condition)
        rc = kz_matrix_norm64(index);
        if (rc != KZ_OK) return rc;
        fp.ynorm64 = index->norm64;
    }
    rc = kz_launch_finalize(ctx, fp, lay, KP, t->q_count, index->dtype);
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipMemcpyAsync(ctx->h_counters + 8, fail_count, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(t->h_out_dist, d_odist.get(), out_n * 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(t->h_out_ind, d_oind.get(), out_n * 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(t->h_fail_list, d_fail.get(), (size_t)t->q_count * 4, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(t->h_fail_tau, d_tau.get(), (size_t)t->q_count * 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipStreamSynchronize(st));
    t->n_fail = ctx->h_counters[8];
    memcpy(&t->err_ratio, ctx->h_counters + 10, 8);
    t->build = build;
    return KZ_OK;
}

// Test hook (kiez_amd.h; tests/test_gpu_sweep_direct.py): one sweep launch of one table entry, its lists and event log as they lie on
// the device.  The stages are kz_knn_impl's own, called in its order with a route filled in by hand (tier, list length and the number
// of index ranges are the caller's choice here, not kz_route.h's): kz_himage_ensure / kz_tier_images, kz_sweep_kernel, kz_chunk_plan,
// kz_prepare_pass, kz_chunk_sweep -- and nothing behind them.  The dual builds get a KzDualPass on the PLAIN images, as
// kz_range_sweep_rows fills one.
extern "C" int kz_selftest_sweep(kz_ctx* ctx, kz_matrix* query, kz_matrix* index, kz_selftest_swp* t) {
    KZ_REQUIRE(ctx && query && index && t && query->ctx == ctx && index->ctx == ctx, "kz_selftest_sweep: null argument / foreign matrix");
    for (const kz_matrix* x : {(const kz_matrix*)query, (const kz_matrix*)index}) {
        KZ_REFUSE_PRECOMPUTED("kz_selftest_sweep", x);
        KZ_REQUIRE(!x->raw_only && x->metric <= KZ_COSINE, "kz_selftest_sweep: searchable matrices of the euclidean family or cosine only");
    }
    KZ_REQUIRE(query->d == index->d && query->metric == index->metric && query->dtype == index->dtype,
               "kz_selftest_sweep: the matrices must share width, metric and element type");
    const int tier = t->tier, KP = t->KP;
    const bool dual = t->dual != 0, q64 = t->q64 != 0;
    KZ_REQUIRE(tier == KZ_TIER_F32 || tier == KZ_TIER_BF || tier == KZ_TIER_H, "kz_selftest_sweep: tier %d", tier);
    KZ_REQUIRE(KP == 16 || KP == 32 || KP == 64 || KP == 128, "kz_selftest_sweep: lists of %d entries", KP);
    KZ_REQUIRE(t->n_ranges >= 1 && t->n_ranges <= KZ_MAX_PIECES, "kz_selftest_sweep: %d index ranges", t->n_ranges);
    KZ_REQUIRE(t->q_count >= 1 && t->q_begin >= 0 && t->q_begin + t->q_count <= query->n, "kz_selftest_sweep: query rows [%lld, +%lld)",
               (long long)t->q_begin, (long long)t->q_count);
    KZ_REQUIRE(!t->h_qfloor || tier == KZ_TIER_H, "kz_selftest_sweep: seeded lists exist on the fp16 tier only");
    KZ_REQUIRE(!dual || (t->h_theta && t->h_qnbias && t->log_cap >= 1 && t->log_cap < ((int64_t)1 << 26) && t->h_log_keys && t->h_log_meta),
               "kz_selftest_sweep: a dual build needs h_theta, h_qnbias, log_cap >= 1 and the two log arrays");
    KZ_REQUIRE(!t->h_out_key || (t->h_out_idx && t->list_capacity >= 1), "kz_selftest_sweep: h_out_key without h_out_idx / list_capacity");
    // ---- the entry: a combination without a build is refused here, before any image is built ----
    const int n_slices = kz_h_nsr(index->kg);
    if ((dual || q64) && tier != KZ_TIER_H) {
        kz_set_error("kz_selftest_sweep: the dual-pass and 64-query builds exist on the fp16 tier only");
        return KZ_ERR_UNSUPPORTED;
    }
    if ((tier == KZ_TIER_H && !kz_h_slices_ok(index->kg)) || (tier == KZ_TIER_BF && !(index->kg / 4 >= 2 && index->kg / 4 <= 24)) ||
        (tier != KZ_TIER_F32 && query->kg != index->kg)) {
        kz_set_error("kz_selftest_sweep: tier %d has no kernel for d=%lld", tier, (long long)index->d);
        return KZ_ERR_UNSUPPORTED;
    }
    KzSweepKernel kern;
    int rc = kz_sweep_kernel(tier, dual, q64, KP, n_slices, &kern);
    if (rc != KZ_OK) return rc;
    KZ_REQUIRE(t->q_count <= kz_rows_per_chunk(ctx, KP, false), "kz_selftest_sweep: %lld rows are more than one launch takes", (long long)t->q_count);
    KZ_HIP(hipSetDevice(ctx->device));
    // ---- route and call as the stages read them ----
    KzRoute route;
    route.tier = tier;
    route.cur.KP = KP;
    route.cur.pieces = t->n_ranges;
    route.lng = route.cur;
    route.KP_class = KP;
    KzDualPass dp;
    memset(&dp, 0, sizeof(dp));
    dp.raw_lists = 1;
    dp.no_q64 = q64 ? 0 : 1;
    const KzCall c = {ctx, query, t->q_begin, t->q_count, index, 1, 0, nullptr, nullptr, nullptr, dual ? &dp : nullptr};
    int blocks_per_cu = 1;
    rc = kz_sweep_occupancy(ctx, kern, &blocks_per_cu);
    if (rc != KZ_OK) return rc;
    const int slots = kz_h_slots(kern.wg_per_item, blocks_per_cu, ctx->n_cus);
    const int tpw_h = q64 ? 2 : 1, n_ytiles = (int)index->n_tiles;
    int64_t max_rows = kz_rows_per_chunk(ctx, KP, false);
    KzChunk ch;
    kz_chunk_plan(c, route, slots, tpw_h, n_ytiles, 0, &max_rows, &ch);
    KZ_REQUIRE(ch.cq_count == t->q_count && ch.pl.list_elems < ((size_t)1 << 28), "kz_selftest_sweep: the rows do not fit one launch (%zu list entries)",
               ch.pl.list_elems);
    const KzListLayout& lay = ch.pl.lay;
    t->n_list = (int64_t)ch.pl.list_elems;
    t->n_regions = lay.n_regions;
    t->halves = lay.halves;
    t->contig = lay.contig;
    t->qt0 = ch.qt0;
    for (int r = 0; r < KZ_MAX_REGIONS; ++r) {
        t->qt_end[r] = r < lay.n_regions ? lay.qt_end[r] : 0;
        t->pieces[r] = r < lay.n_regions ? lay.pieces[r] : 0;
        t->base[r] = r < lay.n_regions ? lay.base[r] : 0;
    }
    t->wg_per_item = kern.wg_per_item;
    t->tiles_per_item = kern.tiles_per_item;
    t->n_slices = kern.n_slices;
    t->entry_KP = kern.KP;
    t->n_items = ch.pl.W;
    t->log_count = 0;
    if (!t->h_out_key) return KZ_OK;   // (the geometry only: the caller sizes its arrays)
    KZ_REQUIRE(t->list_capacity >= t->n_list, "kz_selftest_sweep: the lists hold %lld entries, the arrays %lld", (long long)t->n_list,
               (long long)t->list_capacity);
    rc = kz_matrix_check(query);
    if (rc == KZ_OK) rc = kz_matrix_check(index);
    if (rc != KZ_OK) return rc;
    // ---- the operand images, as kz_knn_impl builds them ----
    if (tier == KZ_TIER_H) {
        rc = kz_himage_ensure(query, index);
        if (rc != KZ_OK) return rc;
    }
    rc = kz_tier_images(c, KzResearch(), route);
    if (rc != KZ_OK) return rc;
    // ---- device copies of the caller's arrays ----
    const size_t q_pad = (size_t)query->n_tiles * KZ_TILE, y_pad = (size_t)n_ytiles * KZ_TILE;
    KzPoolBuf<float> d_floor, d_theta, d_qnbias;
    KzPoolBuf<void> d_lkeys, d_lmeta;
    KzPoolBuf<unsigned long long> d_lcnt;
    bool ok = !t->h_qfloor || d_floor.alloc(ctx, q_pad * 4) == KZ_OK;
    if (dual)
        ok = ok && d_theta.alloc(ctx, y_pad * 4) == KZ_OK && d_qnbias.alloc(ctx, q_pad * 4) == KZ_OK && d_lkeys.alloc(ctx, (size_t)t->log_cap * 16) == KZ_OK &&
             d_lmeta.alloc(ctx, (size_t)t->log_cap * 8) == KZ_OK && d_lcnt.alloc(ctx, 8) == KZ_OK;
    if (!ok) {
        kz_set_error("kz_selftest_sweep: out of device memory");
        return KZ_ERR_NOMEM;
    }
    const hipStream_t st = ctx->stream;
    if (t->h_qfloor) KZ_HIP(hipMemcpyAsync(d_floor.get(), t->h_qfloor, q_pad * 4, hipMemcpyHostToDevice, st));
    if (dual) {
        KZ_HIP(hipMemcpyAsync(d_theta.get(), t->h_theta, y_pad * 4, hipMemcpyHostToDevice, st));
        KZ_HIP(hipMemcpyAsync(d_qnbias.get(), t->h_qnbias, q_pad * 4, hipMemcpyHostToDevice, st));
        KZ_HIP(hipMemsetAsync(d_lkeys.get(), 0xFF, (size_t)t->log_cap * 16, st));
        KZ_HIP(hipMemsetAsync(d_lmeta.get(), 0xFF, (size_t)t->log_cap * 8, st));
        KZ_HIP(hipMemsetAsync(d_lcnt.get(), 0, 8, st));
        dp.probed = 1;
        dp.qpack = (const float*)query->himg->packed;
        dp.ypack = (const float*)index->himg->packed;
        dp.ybias = index->himg->bias;
        dp.theta = d_theta.get();
        dp.qnbias = d_qnbias.get();
        dp.qfloor = d_floor.get();
        dp.log_keys = d_lkeys.get();
        dp.log_meta = d_lmeta.get();
        dp.log_cnt = d_lcnt.get();
        dp.log_cap = t->log_cap;
    }
    KZ_HIP(hipStreamSynchronize(st));   // (the host arrays are the caller's pageable buffers)
    // ---- scratch, work table, launch ----
    KzPass ps;
    rc = kz_prepare_pass(ctx, ch.pl, n_ytiles, slots, tier, ch.cq_count, &ps, tier == KZ_TIER_H ? tpw_h : 1, false);
    if (rc != KZ_OK) return rc;
    // (all-ones bytes: a NaN key, id -1 wherever the kernel writes nothing)
    KZ_HIP(hipMemsetAsync(ps.out_key, 0xFF, (size_t)t->n_list * 4, st));
    KZ_HIP(hipMemsetAsync(ps.out_idx, 0xFF, (size_t)t->n_list * 4, st));
    KzPoolBuf<float> boot_floor;
    KzPoolBuf<unsigned long long> stamp_buf;
    rc = kz_chunk_sweep(c, route, kern, ch, ps, q64, false, d_floor.get(), n_ytiles, boot_floor, stamp_buf);
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipMemcpyAsync(t->h_out_key, ps.out_key, (size_t)t->n_list * 4, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipMemcpyAsync(t->h_out_idx, ps.out_idx, (size_t)t->n_list * 4, hipMemcpyDeviceToHost, st));
    unsigned long long h_cnt = 0;
    if (dual) KZ_HIP(hipMemcpyAsync(&h_cnt, d_lcnt.get(), 8, hipMemcpyDeviceToHost, st));
    KZ_HIP(hipStreamSynchronize(st));
    if (dual) {
        t->log_count = h_cnt;
        const size_t n_log = h_cnt < (unsigned long long)t->log_cap ? (size_t)h_cnt : (size_t)t->log_cap;
        if (n_log > 0) {
            KZ_HIP(hipMemcpyAsync(t->h_log_keys, d_lkeys.get(), n_log * 16, hipMemcpyDeviceToHost, st));
            KZ_HIP(hipMemcpyAsync(t->h_log_meta, d_lmeta.get(), n_log * 8, hipMemcpyDeviceToHost, st));
            KZ_HIP(hipStreamSynchronize(st));
        }
    }
    return KZ_OK;
}

// Behind the finalize kernel: the speculative rescue, the read-back of the fail counter (and of the matrices' deferred finiteness
// verdicts), the synchronisation; *spec_R = rows the speculative launches covered.
static int kz_chunk_readback(const KzCall& c, const KzRoute& route, const KzChunk& ch, const KzPass& ps, const KnnFinParams& fp, int k_eff,
                             int n_ytiles, int n_slices, KzPoolBuf<unsigned long long>& stamp_buf, int* spec_R) {
    kz_ctx* ctx = c.ctx;
    kz_matrix *query = c.query, *index = c.index;
    const KzDualPass* dual = c.dual;
    const int W = ps.W;
    int* fail_count = ctx->d_counters + 8;
    // matrices created from device rows have not had their finiteness verdict read yet (kz_matrix_create waits for
    // nothing): it rides on this call's read-back
    kz_matrix* unchecked[2] = {query->checked ? nullptr : query, (index->checked || index == query) ? nullptr : index};
    *spec_R = 0;
    hipError_t es;
    {
        // SPECULATIVE RESCUE (above kz_escalate_rows): the exact kernels for up to R uncertified rows, before the count is known
        KzSpec spec;   // (its buffers go right after the read-back -- stream-ordered: the launches that used them are on the stream)
        if (!route.exact_only && !(dual && dual->raw_lists) && route.tier != KZ_TIER_F32) {
            const int R = kz_spec_rows(ctx, index, k_eff);
            if (R > 0) {
                const int rc = kz_spec_rescue(ctx, spec, R, query, fp.row_map ? 0 : ch.cq_begin, ps.fail_list, fail_count, index, c.k, c.exclude_self,
                                              c.d_self_ids, fp.out_dist, fp.out_ind);
                if (rc != KZ_OK) return rc;
                if (spec.R > 0) KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
            }
        }
        KZ_HIP(hipMemcpyAsync(ctx->h_counters + 8, fail_count, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        for (int u = 0; u < 2; ++u)
            if (unchecked[u])
                KZ_HIP(hipMemcpyAsync(ctx->h_counters + 44 + 10 * u, unchecked[u]->d_stats, 40, hipMemcpyDeviceToHost, ctx->stream));
        es = hipStreamSynchronize(ctx->stream);
        *spec_R = spec.R;
    }
    KZ_HIP(es);
    if (stamp_buf.get()) {   // (diagnostic: start / end of every workgroup of the sweep, in work-table order, appended to the file)
        std::vector<unsigned long long> hs((size_t)W * 130);
        KZ_HIP(hipMemcpy(hs.data(), stamp_buf.get(), (size_t)W * (16 + 1024), hipMemcpyDeviceToHost));
        stamp_buf.reset();
        if (FILE* f = fopen(getenv("KZ_STAMP_FILE"), "a")) {
            fprintf(f, "# launch W=%d n_qtiles=%d n_ytiles=%d slices=%d\n", W, ch.n_qtiles, n_ytiles, n_slices);
            for (int w = 0; w < W; ++w) {
                fprintf(f, "%d %llu %llu", w, hs[2 * (size_t)w], hs[2 * (size_t)w + 1]);
                if (w < 8 || w % 97 == 0)   // (per-tile stamps of a few workgroups: the first 64 tiles, then every 16th)
                    for (int t = 0; t < 128; ++t) fprintf(f, " %llu", hs[2 * (size_t)W + (size_t)w * 128 + t]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
    }
    for (int u = 0; u < 2; ++u) {
        if (!unchecked[u]) continue;
        if (ctx->h_counters[44 + 10 * u + 8] != 0) {
            kz_set_error(KZ_MSG_NONFINITE);
            return KZ_ERR_NONFINITE;
        }
        memcpy(&unchecked[u]->max_norm, ctx->h_counters + 44 + 10 * u, 8);
        unchecked[u]->checked = true;
    }
    return KZ_OK;
}

// EARLY RANGE RE-SEARCH (kz_route.h: kz_after_pass has said early_range): the grouped ranges are tried on the *n_fail rows of
// ps.fail_list; the rows they leave are in early_left (*esc_list, *n_fail) -- or, with no room for the lists, everything as it was.
static int kz_early_range(const KzCall& c, const KzPass& ps, const KnnFinParams& fp, int64_t cq_begin, int* n_fail, KzPoolBuf<int>& early_left,
                          const int** esc_list, KzTally* tally) {
    kz_ctx* ctx = c.ctx;
    KzPoolBuf<int> fl0;
    KzPoolBuf<double> tau0;
    int rc = fl0.alloc(ctx, (size_t)*n_fail * sizeof(int));
    if (rc == KZ_OK) rc = tau0.alloc(ctx, (size_t)*n_fail * 8);
    if (rc == KZ_OK) rc = early_left.alloc(ctx, (size_t)*n_fail * sizeof(int));
    if (rc == KZ_OK && (hipMemcpyAsync(fl0.get(), ps.fail_list, (size_t)*n_fail * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess ||
                        hipMemcpyAsync(tau0.get(), ps.fail_tau, (size_t)*n_fail * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)) {
        kz_set_error("kz_knn: copying the uncertified rows failed");
        rc = KZ_ERR_HIP;
    }
    int n_after = *n_fail;
    long long pairs = 0, grouped = 0;
    const bool no_mem = rc == KZ_ERR_NOMEM;   // (no room for the lists: the next tier as before -- the step is an optimisation)
    if (rc == KZ_OK) {
        KZ_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
        rc = kz_range_rescue(ctx, c.query, fp.row_map ? 0 : cq_begin, fl0.get(), tau0.get(), *n_fail, c.index, c.k, c.exclude_self, c.d_self_ids,
                             fp.out_dist, fp.out_ind, early_left.get(), &n_after, &pairs, &grouped, true, KZ_RANGE_EARLY_PER_ROW);
    }
    fl0.reset();
    tau0.reset();
    if (no_mem) {
        early_left.reset();
        return KZ_OK;
    }
    if (rc != KZ_OK) return rc;
    KZ_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]));
    tally->fb_ms += ms;
    tally->n_range += *n_fail - n_after;
    tally->n_range_group += grouped;
    tally->n_range_pairs += pairs;
    tally->n_fail_total += *n_fail - n_after;   // (answered by the exact kernels)
    *n_fail = n_after;
    *esc_list = early_left.get();
    return KZ_OK;
}

static int kz_knn_impl(kz_ctx* ctx, kz_matrix* query, int64_t q_begin, int64_t q_count, kz_matrix* index, int k,
                       int exclude_self, const int64_t* d_self_ids, KzResearch rs, double* d_dist,
                       int64_t* d_ind, kz_knn_stats* stats, KzDualPass* dual) {
    // (before kz_require_pair reads a precomputed matrix' deferred verdict: a refusal waits for nothing)
    KZ_REQUIRE(!(exclude_self && query && query->pre),
               "kz_knn: exclude_self has no meaning for a precomputed distance matrix (two-sided data: mask the diagonal in the matrix)");
    {
        const int rcp = kz_require_pair("kz_knn", ctx, query, q_begin, q_count, index, d_dist, d_ind);
        if (rcp != KZ_OK) return rcp;
    }
    KZ_REQUIRE(k >= 1, "kz_knn: Expected k > 0. Got %d", k);
    const int k_eff = k + (exclude_self ? 1 : 0);
    KZ_REQUIRE((int64_t)k_eff <= index->n, "kz_knn: Expected n_neighbors %s n_samples_fit, but n_neighbors = %d, n_samples_fit = %lld",
               exclude_self ? "<" : "<=", k, (long long)index->n);
    if (index->metric == KZ_PRECOMPUTED) return kz_knn_precomputed(ctx, query, q_begin, q_count, index, k, d_dist, d_ind, stats);
    if (exclude_self && !d_self_ids)
        KZ_REQUIRE(query->n == index->n, "kz_knn: exclude_self needs query and index of equal length");
    const KzCall c = {ctx, query, q_begin, q_count, index, k, exclude_self, d_self_ids, d_dist, d_ind, dual};
    const KzRouteIn in = kz_route_in(c, k_eff);

    // ---- the lists of this call (kz_route.h: long-k route, the dual pass' short lists, exact-only, what a re-search raises) ----------
    KzRoute route;
    if (!kz_route_lists(in, rs, &route)) {
        kz_set_error("kz_knn: k=%d exceeds the supported maximum of %d neighbours per query", k_eff, KZ_EXACT_MAX_K);
        return KZ_ERR_UNSUPPORTED;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (q_count == 0) return KZ_OK;
    KZ_HIP(hipSetDevice(ctx->device));

    const int n_ytiles = (dual && dual->n_ytiles > 0) ? dual->n_ytiles : (int)index->n_tiles;
    const int n_slices = in.n_slices;
    // rounding bound factors.  float32 operands: (d_pad + 16) 2^-24 covers the d+1 step fma chain, the float32 rounding of
    // the bias and (float64 inputs) of the operands; 1e-12 covers the float64 re-rank's own rounding.  fp16 operands: the
    // float32 accumulation of d_pad exact products + bias in an unspecified order, (n + 16) u doubled to allow for
    // truncating internal adds (the operand rounding is measured per row, kz_pack.hip): kz_gamma_acc_h, kz_fin_params.
    const double gamma_f32 = ((double)(index->kg * 4 + 16) * 5.9604644775390625e-08 + 1e-12) * ctx->eps_scale;
    const double gamma_bf = kz_bf16_gamma(index->kg_bf * 4) * ctx->eps_scale;

    // ---- tier of this call, and the routes of lists of 16 on the row-dealt image (kz_route.h) ---------------------------------------
    kz_route_tier(in, rs, &route);
    if (route.tier == KZ_TIER_H) {
        const int rc = kz_himage_ensure(query, index);
        if (rc != KZ_OK) return rc;
    }
    {   // SHORT-LIST ROUTE of the ordinary kernel
        int P = 0, sel = 0;
        if (kz_route_short_geometry(in, rs, route, &P, &sel)) {
            const int rc = kz_himage_dealt(index, P);
            if (rc == KZ_OK)
                kz_route_take_dealt(&route, P, sel, false);
            else if (rc != KZ_ERR_NOMEM)
                return rc;   // (no memory for the second image: the long list)
        }
    }
    if (rs.wide_lists > 0) {   // WIDE ROUTE, asked for by the caller
        const int rc = kz_take_wide(index, in, &route, rs.wide_lists);
        if (rc != KZ_OK && rc != KZ_ERR_UNSUPPORTED && rc != KZ_ERR_NOMEM) return rc;   // (not available: this call's ordinary route)
    }
    // ---- tier probe: may move the call to the wide route or down a tier, or seed its lists ------------------------------------------
    KzTally tally;
    float* qfloor_ord = nullptr;   // seeded lists of an ordinary search (the context's buffer: nothing to release)
    bool probed = false;           // the tier probe has run: its verdict stands (no ladder after the fact)
    if (kz_probe_wanted(in, rs, route, q_count)) {
        const int rc = kz_tier_probe(c, in, &route, &qfloor_ord, &tally.probe_ms);
        if (rc != KZ_OK) return rc;
        probed = true;
    }
    bool q64 = false;   // the 64-queries-per-wave build of the fp16 kernel for this call
    {
        const int rc = kz_q64_wanted(c, route, n_slices, &q64);
        if (rc != KZ_OK) return rc;
    }
    const int tpw_h = q64 ? 2 : 1;   // query tiles per workgroup of the fp16 kernel this call runs
    // The sweep kernel of the call's tier and the work items a round of it may hold: resolved (and its occupancy queried) once, and
    // again only when the call goes down a tier (after kz_route_next_tier: the list length may have changed with it).  The one choice
    // of kernel: every launch below starts `kern`.
    KzSweepKernel kern;
    int kern_tier = -1, kern_slots = 0;
    auto kernel_for = [&](int t) -> int {
        if (kern_tier == t && kern.KP == route.cur.KP) return KZ_OK;
        int rc0 = kz_sweep_kernel(t, dual != nullptr, q64, route.cur.KP, n_slices, &kern);
        if (rc0 != KZ_OK) return rc0;
        int blocks_per_cu = 1;
        rc0 = kz_sweep_occupancy(ctx, kern, &blocks_per_cu);
        if (rc0 != KZ_OK) return rc0;
        kern_slots = kz_h_slots(kern.wg_per_item, blocks_per_cu, ctx->n_cus);
        kern_tier = t;
        return KZ_OK;
    };
    // query rows are processed in chunks so that the candidate lists stay below ~1 GiB: 524288 rows for K' >= 64, up to four
    // times as many for shorter lists (1 M x 250 k, K' = 16: one launch instead of two -- one tail round, one read-back, one
    // re-search of the uncertified rows)
    // (taken after the probe has possibly changed the route, like first_tier)
    const int KP_mem = route.KP_class > route.cur.KP ? route.KP_class : route.cur.KP;   // (short-list route: several lists of 16 -- the chunk of the replaced list length)
    // (the wide route keeps 32 lists of 16 per query -- 4 KiB: 524288 rows)
    int64_t max_rows_per_chunk = kz_rows_per_chunk(ctx, KP_mem, route.wide_route);   // (halved by kz_chunk_plan where a chunk's lists would pass 2^32 entries)
    if (dual && dual->raw_lists && q_count > max_rows_per_chunk) {
        kz_set_error("kz_knn: internal: a raw-list pass must be one launch");
        return KZ_ERR_INVALID;
    }
    const int first_tier = route.tier;
    for (int64_t c0 = 0; c0 < q_count;) {
        int rc = kz_tier_images(c, rs, route);
        if (rc != KZ_OK) return rc;
        rc = kernel_for(route.tier);
        if (rc != KZ_OK) return rc;
        const int tier = route.tier, KP = route.cur.KP, slots = kern_slots;
        KzChunk ch;
        kz_chunk_plan(c, route, slots, tpw_h, n_ytiles, c0, &max_rows_per_chunk, &ch);
        KzPass ps;
        // (range-0 bootstrap: the short-list routes of the ordinary 32-query kernel, from four ranges on)
        const bool boot = tier == KZ_TIER_H && route.short_ord && !dual && !q64 && ch.force_pieces >= 4;
        rc = kz_prepare_pass(ctx, ch.pl, n_ytiles, slots, tier, ch.cq_count, &ps, tier == KZ_TIER_H ? tpw_h : 1, boot);
        if (rc != KZ_OK) return rc;
        int* fail_count = ctx->d_counters + 8;
        KZ_HIP(hipMemsetAsync(fail_count, 0, 4 * sizeof(int), ctx->stream));  // fail counter, (unused), error-ratio bits
        KzPoolBuf<float> boot_floor;   // (this chunk's range-0 floor, if any: the finalize kernel must know it)
        KzPoolBuf<unsigned long long> stamp_buf;   // (diagnostic "abl_stamp")
        rc = kz_chunk_sweep(c, route, kern, ch, ps, q64, boot, qfloor_ord, n_ytiles, boot_floor, stamp_buf);
        if (rc != KZ_OK) return rc;
        if (dual && tier != KZ_TIER_H) dual->broken = 1;   // this chunk's pairs were not scanned for events
        KZ_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
        if (dual) {
            dual->lists_key = ps.out_key;
            dual->lists_idx = ps.out_idx;
            dual->lists_lay = ps.lay;
            dual->lists_KP = KP;
        }
        if (dual && dual->post_sweep && !dual->broken && c0 + ch.cq_count >= q_count) {
            dual->post_called = 1;
            rc = dual->post_sweep(dual->post_user);
            if (rc != KZ_OK) return rc;
        }

        // ---- finalize: select, re-rank in float64, certify ---------------------------------------------------------------------------
        KnnFinParams fp;
        rc = kz_chunk_finalize(c, route, ch, ps, c0, tier == KZ_TIER_BF ? gamma_bf : gamma_f32, boot_floor.get() ? boot_floor.get() : qfloor_ord, &fp);
        if (rc != KZ_OK) return rc;
        boot_floor.reset();   // (stream-ordered: the launches above have it)
        KZ_HIP(hipGetLastError());
        KZ_HIP(hipEventRecord(ctx->ev[2], ctx->stream));

        // ---- read-back: how many rows are left, and where they go (kz_route.h: kz_after_pass) ----------------------------------------
        int spec_R = 0;   // rows the speculative launches covered
        rc = kz_chunk_readback(c, route, ch, ps, fp, k_eff, n_ytiles, n_slices, stamp_buf, &spec_R);
        if (rc != KZ_OK) return rc;
        int n_fail = route.exact_only ? (int)ch.cq_count : ctx->h_counters[8];
        tally.n_first_fail += n_fail;
        {
            double ratio;
            memcpy(&ratio, ctx->h_counters + 10, 8);
            if (ratio > tally.max_err_ratio) tally.max_err_ratio = ratio;
        }
        float ms = 0;
        KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        tally.main_ms += ms;
        KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        tally.fin_ms += ms;
        tally.last_splits = ps.lay.pieces[0];
        tally.last_blocks = ps.W;
        const KzAfterPass ap = kz_after_pass(in, rs, route, probed, n_fail, ch.cq_count, spec_R);
        if (ap.rescued) {
            KZ_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
            tally.fb_ms += ms;
            tally.n_spec += n_fail;
        }
        if (ap.escalate) {
            // the uncertified rows again, as a dense block, with what ap.next asks for; the rest of the call at ap.tier_next
            KzPoolBuf<int> early_left;
            const int* esc_list = ps.fail_list;
            if (ap.early_range) {
                rc = kz_early_range(c, ps, fp, ch.cq_begin, &n_fail, early_left, &esc_list, &tally);
                if (rc != KZ_OK) return rc;
            }
            kz_knn_stats st2;
            memset(&st2, 0, sizeof(st2));
            ms = 0;
            if (n_fail == 0) {
            } else if (ap.ladder)
                rc = kz_escalate_ladder(ctx, query, fp.row_map ? 0 : ch.cq_begin, esc_list, n_fail, index, k, exclude_self, d_self_ids, ap.next,
                                        fp.out_dist, fp.out_ind, &st2, &ms);
            else
                rc = kz_escalate_rows(ctx, query, fp.row_map ? 0 : ch.cq_begin, esc_list, n_fail, index, k, exclude_self, d_self_ids, ap.next,
                                      fp.out_dist, fp.out_ind, &st2, &ms);
            early_left.reset();
            if (rc != KZ_OK) return rc;
            tally.fb_ms += ms;
            tally.n_escalated += n_fail;
            tally.add(st2);
            c0 += max_rows_per_chunk;
            kz_route_next_tier(&route, ap.tier_next);   // (kernel_for re-resolves at the top of the next chunk)
            continue;
        }
        tally.n_fail_total += n_fail;

        if (n_fail > 0 && !ap.rescued) {
            // exact brute force against the whole index (kz_exact.h), behind the range re-search where that applies
            KzExactTaken taken;
            rc = kz_exact_whole_index(ctx, query, ch.cq_begin, ps.fail_list, ps.fail_tau, n_fail, ap.range_first, index, k, exclude_self, d_self_ids,
                                      fp.out_dist, fp.out_ind, &taken);
            if (rc != KZ_OK) return rc;
            tally.n_range += taken.range_rows;
            tally.n_range_pairs += taken.range_pairs;
            tally.n_range_group += taken.range_group_rows;
            tally.fb_ms += taken.ms;
        }
        c0 += max_rows_per_chunk;
    }
    if (stats) {
        tally.write(stats);
        stats->list_len = route.cur.KP;
        stats->first_pass = first_tier;
        stats->wide_lists = route.wide_route ? route.cur.pieces : 0;
    }
    return KZ_OK;
}


extern "C" int kz_knn(kz_ctx* ctx, const kz_matrix* query, int64_t q_begin, int64_t q_count, const kz_matrix* index, int k,
                      int exclude_self, double* d_dist, int64_t* d_ind, kz_knn_stats* stats) {
    // (the matrices are logically const for the caller: kz_knn only attaches lazily built operand images to them)
    return kz_knn_impl(ctx, const_cast<kz_matrix*>(query), q_begin, q_count, const_cast<kz_matrix*>(index), k, exclude_self, nullptr,
                       KzResearch(), d_dist, d_ind, stats, nullptr);
}

#include "kz_gold_ranks.h"
#include "kz_knn_reduced.h"
#include "kz_radius.h"
#include "kz_pairs.h"
#include "kz_softmin.h"
#include "kz_knn_dual.h"
