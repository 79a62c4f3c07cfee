// OPTIMAL ONE-TO-ONE ASSIGNMENT: Bertsekas' forward auction (Jacobi form) over neighbour lists.
// Entry (i, c) of dist / ind [n_q, k] is a PAIR when 0 <= ind < n_index, w = (double)dist is finite and w <= u (the price of staying
// unmatched); any other entry is no pair.  Target prices start at 0.0 and every row FREE.  In a round every FREE row i computes
// v_c = (-w_c) - price[t_c] over its pair columns; best = the first column with the largest v (v1), v2 = the largest v of its other
// pair columns taken together with -u.  Not v1 > -u: the row stays unmatched for good (prices only rise).  Otherwise it bids
// (price[t] + (v1 - v2)) + eps on its best target.  A target takes the largest bid, among equal bids the smallest row: the bid becomes
// the price, the winner the owner, the previous owner FREE again.  The run ends when no row is FREE.  The rule is synchronous per
// round: the arrays that come out depend neither on thread order nor on how the rounds are spread over launches.  float64 add,
// subtract and compare only (-ffp-contract=off); cost <= optimum + n_q eps.
//
// TWO PHASES, one rule:
//   wide: three grid-wide launches per round (one thread per row, grid-stride), while more than tail_rows rows are FREE:
//         bid (64-bit atomicMax of the bid's order key into the target's word), tie (atomicMin of the row among the bidders whose
//         key is the word), resolve (the bidder that finds its key and row takes the target).  KZ_ASSIGN_WIDE_ROUNDS rounds are queued
//         per read of the FREE counts;
//   tail: ONE workgroup, one bidder per thread.  It gathers the FREE rows into an LDS queue and runs up to KZ_ASSIGN_TAIL_ROUNDS
//         rounds inside the launch, workgroup barriers between bid, tie and resolve; winners push the row they displaced, losers
//         themselves, into the next round's queue (queue order cannot change a synchronous round).  Price, owner and bid words that
//         another wave of the workgroup may have written earlier in the launch are read and written as relaxed agent-scope atomics,
//         and every wave waits for its memory operations before each barrier.
// No kernel waits for another workgroup; every loop in a kernel is bounded.
#include "kz_common.h"
#include "kz_order_key.h"
#include "kz_pool_buf.h"

// rounds queued between two reads of the FREE counts (wide) and rounds run inside one tail launch (profiles/assignment.md;
// -DKZ_ASSIGN_WIDE_ROUNDS=n / -DKZ_ASSIGN_TAIL_ROUNDS=n build the variants measured there)
#ifndef KZ_ASSIGN_WIDE_ROUNDS
#define KZ_ASSIGN_WIDE_ROUNDS 8
#endif
#ifndef KZ_ASSIGN_TAIL_ROUNDS
#define KZ_ASSIGN_TAIL_ROUNDS 1024
#endif
constexpr int KZ_ASSIGN_BLOCKS = 256;        // of 256 threads: one grid covers 65 536 rows, more rows take the grid-stride loop
constexpr int KZ_ASSIGN_TAIL_MAX = 1024;     // the workgroup limit: one bidder per thread
constexpr int KZ_ASSIGN_CHUNK = 8;           // columns of a list whose loads are in flight together

enum { KZ_ASSIGN_FREE = 0, KZ_ASSIGN_BIDDING = 1, KZ_ASSIGN_OWNER = 2, KZ_ASSIGN_OUT = 3 };
constexpr int KZ_ASSIGN_NO_ROW = 0x7fffffff;          // the second bid word of a target nobody bids on
constexpr unsigned long long KZ_ASSIGN_NO_BID = 0ull; // the first: below the key of every double

int kz_match_require(const char* who, kz_ctx* ctx, const void* d_dist, int dist_dtype, int64_t n_q, int k);   // kz_match.hip

// working arrays (the context's scoped scratch)
struct KzAssignState {
    unsigned long long* price;     // [n_index] the price as the bits of a double (d_price, or scratch)
    int* owner;                    // [n_index] the row that holds the target (-1: none)
    unsigned long long* bid_key;   // [n_index] largest key bid this round (KZ_ASSIGN_NO_BID: none)
    int* bid_row;                  // [n_index] smallest row among the bidders with that key (KZ_ASSIGN_NO_ROW: none)
    int* state;                    // [n_q] KZ_ASSIGN_*
    int* bid_col;                  // [n_q] wide rounds: the column a BIDDING row bids on
    double* bid_val;               // [n_q] wide rounds: its bid
};

#define KZ_RLX_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define KZ_RLX_STORE(p, x) __hip_atomic_store((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// The bid of FREE row i under the current prices -> false: no pair column is strictly better than staying out.
// SHARED: prices may have been written by another wave earlier in this launch (the tail kernel).
template <typename T, bool SHARED>
__device__ __forceinline__ bool kz_assign_bid(const KzAssignState& s, const T* __restrict__ dist, const int64_t* __restrict__ ind, int64_t i,
                                              int k, int64_t n_index, double u, double eps, int& c_best, int64_t& t_best, double& bid) {
    double v1 = -INFINITY, v2 = -u, p_best = 0.0;
    c_best = -1;
    t_best = -1;
    // KZ_ASSIGN_CHUNK columns at a time: their ids and values, then their prices, are loads that do not wait for each other; the
    // compares run in column order (a column past the end, or no pair, has t = -1 and reads the price of target 0 for nothing)
    for (int c0 = 0; c0 < k; c0 += KZ_ASSIGN_CHUNK) {
        int64_t t[KZ_ASSIGN_CHUNK];
        double w[KZ_ASSIGN_CHUNK], p[KZ_ASSIGN_CHUNK];
#pragma unroll
        for (int j = 0; j < KZ_ASSIGN_CHUNK; ++j) {
            const bool in = c0 + j < k;
            const int64_t e = i * k + (in ? c0 + j : c0);
            t[j] = ind[e];
            w[j] = (double)dist[e];
            if (!in) t[j] = -1;
        }
#pragma unroll
        for (int j = 0; j < KZ_ASSIGN_CHUNK; ++j) {
            // NaN, +-inf, above the threshold, an id out of range: no pair
            const bool ok = t[j] >= 0 && t[j] < n_index && fabs(w[j]) <= 1.7976931348623157e308 && w[j] <= u;
            if (!ok) t[j] = -1;
            const unsigned long long* pp = s.price + (ok ? t[j] : 0);
            p[j] = __longlong_as_double((long long)(SHARED ? KZ_RLX_LOAD(pp) : *pp));
        }
#pragma unroll
        for (int j = 0; j < KZ_ASSIGN_CHUNK; ++j) {
            if (t[j] < 0) continue;
            const double v = (-w[j]) - p[j];
            if (v > v1) {
                if (v1 > v2) v2 = v1;
                v1 = v;
                c_best = c0 + j;
                t_best = t[j];
                p_best = p[j];
            } else if (v > v2) {
                v2 = v;
            }
        }
    }
    if (!(v1 > -u)) return false;
    bid = (p_best + (v1 - v2)) + eps;
    return true;
}

__global__ __launch_bounds__(256) void kz_assign_init_kernel(KzAssignState s, int n_q, int n_index, int64_t* __restrict__ match,
                                                             int64_t* __restrict__ col) {
    const int stride = gridDim.x * blockDim.x;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t t = tid; t < n_index; t += stride) {
        s.price[t] = 0ull;   // +0.0
        s.owner[t] = -1;
        s.bid_key[t] = KZ_ASSIGN_NO_BID;
        s.bid_row[t] = KZ_ASSIGN_NO_ROW;
    }
    for (int64_t i = tid; i < n_q; i += stride) {
        s.state[i] = KZ_ASSIGN_FREE;
        match[i] = -1;
        col[i] = -1;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void kz_assign_bid_kernel(KzAssignState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                            int n_q, int k, int64_t n_index, double u, double eps) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_FREE) continue;
        int c;
        int64_t t;
        double bid;
        if (!kz_assign_bid<T, false>(s, dist, ind, i, k, n_index, u, eps, c, t, bid)) {
            s.state[i] = KZ_ASSIGN_OUT;
            continue;
        }
        atomicMax(s.bid_key + t, kz_knnr_key(bid));
        s.bid_col[i] = c;
        s.bid_val[i] = bid;
        s.state[i] = KZ_ASSIGN_BIDDING;
    }
}

__global__ __launch_bounds__(256) void kz_assign_tie_kernel(KzAssignState s, const int64_t* __restrict__ ind, int n_q, int k) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_BIDDING) continue;
        const int64_t t = ind[i * k + s.bid_col[i]];
        if (s.bid_key[t] == kz_knnr_key(s.bid_val[i])) atomicMin(s.bid_row + t, (int)i);
    }
}

// The winner resets the bid words that the other bidders of its target read in this launch: they are read and written as relaxed
// agent-scope atomics, and a bidder that is not the winner finds "not mine" in either version -- no bidder has the key
// KZ_ASSIGN_NO_BID.  The displaced row is an owner, so no bidder; only the winner of its target writes its state.
// free_after: the rows FREE once the round is over (losers and displaced owners).
__global__ __launch_bounds__(256) void kz_assign_resolve_kernel(KzAssignState s, const int64_t* __restrict__ ind, int n_q, int k,
                                                                int64_t* __restrict__ match, int64_t* __restrict__ col,
                                                                unsigned* __restrict__ free_after) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_BIDDING) continue;
        const int c = s.bid_col[i];
        const int64_t t = ind[i * k + c];
        const double bid = s.bid_val[i];
        const bool won = KZ_RLX_LOAD(s.bid_key + t) == kz_knnr_key(bid) && KZ_RLX_LOAD(s.bid_row + t) == (int)i;
        if (!won) {
            s.state[i] = KZ_ASSIGN_FREE;
            atomicAdd(free_after, 1u);
            continue;
        }
        KZ_RLX_STORE(s.bid_key + t, KZ_ASSIGN_NO_BID);
        KZ_RLX_STORE(s.bid_row + t, KZ_ASSIGN_NO_ROW);
        const int old = s.owner[t];
        s.price[t] = (unsigned long long)__double_as_longlong(bid);
        s.owner[t] = (int)i;
        s.state[i] = KZ_ASSIGN_OWNER;
        match[i] = t;
        col[i] = c;
        if (old >= 0) {
            s.state[old] = KZ_ASSIGN_FREE;
            match[old] = -1;
            col[old] = -1;
            atomicAdd(free_after, 1u);
        }
    }
}

// every memory operation of this wave has completed (stores and atomics are acknowledged by the L2) before it joins the barrier
__device__ __forceinline__ void kz_assign_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// out[0] = rounds run, out[1] = rows still FREE, out[2] = 1 if more rows were FREE than the workgroup has threads (nothing was done)
template <typename T>
__global__ __launch_bounds__(KZ_ASSIGN_TAIL_MAX) void kz_assign_tail_kernel(KzAssignState s, const T* __restrict__ dist,
                                                                            const int64_t* __restrict__ ind, int n_q, int k, int64_t n_index,
                                                                            double u, double eps, int round_limit, int64_t* match,
                                                                            int64_t* col, int* __restrict__ out) {
    __shared__ int queue[2][KZ_ASSIGN_TAIL_MAX];
    __shared__ int queue_n[2];
    const int tid = threadIdx.x;
    if (tid == 0) queue_n[0] = queue_n[1] = 0;
    __syncthreads();
    for (int i = tid; i < n_q; i += blockDim.x) {
        if (s.state[i] != KZ_ASSIGN_FREE) continue;
        const int slot = atomicAdd(&queue_n[0], 1);
        if (slot < KZ_ASSIGN_TAIL_MAX) queue[0][slot] = i;
    }
    __syncthreads();
    int n_cur = queue_n[0];
    if (n_cur > (int)blockDim.x) {   // (uniform) the host launches a thread per FREE row
        if (tid == 0) {
            out[0] = 0;
            out[1] = n_cur;
            out[2] = 1;
        }
        return;
    }
    int cur = 0, r = 0;
    for (; r < round_limit && n_cur > 0; ++r) {
        const int nxt = cur ^ 1;
        if (tid == 0) queue_n[nxt] = 0;
        bool bidding = false;
        int i = -1, c = -1;
        int64_t t = -1;
        double bid = 0.0;
        unsigned long long key = 0ull;
        if (tid < n_cur) {
            i = queue[cur][tid];
            bidding = kz_assign_bid<T, true>(s, dist, ind, i, k, n_index, u, eps, c, t, bid);
            if (bidding) {
                key = kz_knnr_key(bid);
                atomicMax(s.bid_key + t, key);
            } else {
                s.state[i] = KZ_ASSIGN_OUT;
            }
        }
        kz_assign_barrier();
        if (bidding && KZ_RLX_LOAD(s.bid_key + t) == key) atomicMin(s.bid_row + t, i);
        kz_assign_barrier();
        if (bidding) {
            const bool won = KZ_RLX_LOAD(s.bid_key + t) == key && KZ_RLX_LOAD(s.bid_row + t) == i;
            if (!won) {
                const int slot = atomicAdd(&queue_n[nxt], 1);   // (at most one push per bidder: never more than n_cur)
                if (slot < KZ_ASSIGN_TAIL_MAX) queue[nxt][slot] = i;
            } else {
                KZ_RLX_STORE(s.bid_key + t, KZ_ASSIGN_NO_BID);
                KZ_RLX_STORE(s.bid_row + t, KZ_ASSIGN_NO_ROW);
                const int old = KZ_RLX_LOAD(s.owner + t);
                KZ_RLX_STORE(s.price + t, (unsigned long long)__double_as_longlong(bid));
                KZ_RLX_STORE(s.owner + t, i);
                s.state[i] = KZ_ASSIGN_OWNER;
                match[i] = t;
                col[i] = c;
                if (old >= 0) {
                    s.state[old] = KZ_ASSIGN_FREE;
                    match[old] = -1;
                    col[old] = -1;
                    const int slot = atomicAdd(&queue_n[nxt], 1);
                    if (slot < KZ_ASSIGN_TAIL_MAX) queue[nxt][slot] = old;
                }
            }
        }
        kz_assign_barrier();
        cur = nxt;
        n_cur = queue_n[cur];
    }
    if (tid == 0) {
        out[0] = r;
        out[1] = n_cur;
        out[2] = 0;
    }
}

static int kz_assign_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : b < KZ_ASSIGN_BLOCKS ? b : KZ_ASSIGN_BLOCKS);
}

template <typename T>
static int kz_assign_lists_impl(kz_ctx* ctx, const T* d_dist, const int64_t* d_ind, int n_q, int k, int64_t n_index, double u, double eps,
                                int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col, double* d_price, int64_t* h_rounds,
                                int* h_converged) {
    // (released when the function returns, behind its last synchronise)
    KzPoolBuf<unsigned long long> price, bid_key;
    KzPoolBuf<int> owner, bid_row, state, bid_col, tail_out;
    KzPoolBuf<double> bid_val;
    KzPoolBuf<unsigned> counts;
    int rc = KZ_OK;
    if (!d_price) rc = price.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = bid_key.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = owner.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = bid_row.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = state.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = bid_col.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = bid_val.alloc(ctx, (size_t)n_q * 8);
    if (rc == KZ_OK) rc = counts.alloc(ctx, KZ_ASSIGN_WIDE_ROUNDS * sizeof(unsigned));
    if (rc == KZ_OK) rc = tail_out.alloc(ctx, 3 * sizeof(int));
    if (rc != KZ_OK) return rc;
    const KzAssignState s{d_price ? (unsigned long long*)d_price : price.get(), owner.get(), bid_key.get(), bid_row.get(), state.get(),
                          bid_col.get(), bid_val.get()};
    const dim3 grid(kz_assign_blocks(n_q)), block(256);
    hipLaunchKernelGGL(kz_assign_init_kernel, dim3(kz_assign_blocks(n_q > n_index ? n_q : n_index)), block, 0, ctx->stream, s, n_q,
                       (int)n_index, d_match, d_col);
    KZ_HIP(hipGetLastError());
    int64_t rounds = 0, n_free = n_q;   // n_free: the rows FREE now (exact after every read)
    while (n_free > 0 && rounds < max_rounds) {
        const int64_t left = max_rounds - rounds;
        if (tail_rows >= 0 && n_free <= tail_rows) {
            const int limit = (int)(left < KZ_ASSIGN_TAIL_ROUNDS ? left : KZ_ASSIGN_TAIL_ROUNDS);
            int threads = (int)((n_free + 63) / 64 * 64);
            threads = threads < 256 ? 256 : threads;   // (the gather of the FREE rows walks all n_q states)
            hipLaunchKernelGGL(kz_assign_tail_kernel<T>, dim3(1), dim3(threads), 0, ctx->stream, s, d_dist, d_ind, n_q, k, n_index, u, eps, limit,
                               d_match, d_col, tail_out.get());
            KZ_HIP(hipGetLastError());
            int h_out[3];
            KZ_HIP(hipMemcpyAsync(h_out, tail_out.get(), sizeof(h_out), hipMemcpyDeviceToHost, ctx->stream));
            KZ_HIP(hipStreamSynchronize(ctx->stream));
            if (h_out[2] != 0 || h_out[1] > n_free || (h_out[0] == 0 && h_out[1] != 0)) {
                kz_set_error("kz_assign_lists: the tail kernel found %d FREE rows where at most %lld were expected", h_out[1], (long long)n_free);
                return KZ_ERR_HIP;
            }
            rounds += h_out[0];
            n_free = h_out[1];
            continue;
        }
        const int nr = (int)(left < KZ_ASSIGN_WIDE_ROUNDS ? left : KZ_ASSIGN_WIDE_ROUNDS);
        KZ_HIP(hipMemsetAsync(counts.get(), 0, KZ_ASSIGN_WIDE_ROUNDS * sizeof(unsigned), ctx->stream));
        for (int r = 0; r < nr; ++r) {
            hipLaunchKernelGGL(kz_assign_bid_kernel<T>, grid, block, 0, ctx->stream, s, d_dist, d_ind, n_q, k, n_index, u, eps);
            hipLaunchKernelGGL(kz_assign_tie_kernel, grid, block, 0, ctx->stream, s, d_ind, n_q, k);
            hipLaunchKernelGGL(kz_assign_resolve_kernel, grid, block, 0, ctx->stream, s, d_ind, n_q, k, d_match, d_col, counts.get() + r);
        }
        KZ_HIP(hipGetLastError());
        unsigned h_counts[KZ_ASSIGN_WIDE_ROUNDS];
        KZ_HIP(hipMemcpyAsync(h_counts, counts.get(), sizeof(h_counts), hipMemcpyDeviceToHost, ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < nr && n_free > 0; ++r) {   // (a round counts when a row was FREE at its start)
            rounds += 1;
            n_free = h_counts[r];
        }
    }
    if (h_rounds) *h_rounds = rounds;
    if (h_converged) *h_converged = n_free == 0;
    return KZ_OK;
}

extern "C" int kz_assign_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                               double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col,
                               double* d_price, int64_t* h_rounds, int* h_converged) {
    const int rcq = kz_match_require("kz_assign_lists", ctx, d_dist, dist_dtype, n_q, k);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_assign_lists: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    KZ_REQUIRE(fabs(unmatched_cost) <= 1.7976931348623157e308, "kz_assign_lists: unmatched_cost must be finite, got %g", unmatched_cost);
    KZ_REQUIRE(eps > 0.0 && eps <= 1.7976931348623157e308, "kz_assign_lists: eps must be positive and finite, got %g", eps);
    KZ_REQUIRE(max_rounds >= 0, "kz_assign_lists: max_rounds = %lld is negative", (long long)max_rounds);
    KZ_REQUIRE(tail_rows <= KZ_ASSIGN_TAIL_MAX, "kz_assign_lists: tail_rows = %d is above %d, the rows one workgroup takes", tail_rows,
               KZ_ASSIGN_TAIL_MAX);
    if (h_rounds) *h_rounds = 0;
    if (h_converged) *h_converged = 1;
    KZ_HIP(hipSetDevice(ctx->device));
    if (d_price && n_q == 0) KZ_HIP(hipMemsetAsync(d_price, 0, (size_t)n_index * sizeof(double), ctx->stream));
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_ind && d_match && d_col, "kz_assign_lists: null argument");
    if (tail_rows == 0) tail_rows = KZ_ASSIGN_TAIL_MAX;
    if (dist_dtype == KZ_F32)
        return kz_assign_lists_impl(ctx, (const float*)d_dist, d_ind, (int)n_q, k, n_index, unmatched_cost, eps, max_rounds, tail_rows, d_match,
                                    d_col, d_price, h_rounds, h_converged);
    return kz_assign_lists_impl(ctx, (const double*)d_dist, d_ind, (int)n_q, k, n_index, unmatched_cost, eps, max_rounds, tail_rows, d_match,
                                d_col, d_price, h_rounds, h_converged);
}

// ---- the range of the listed values: what the defaults of unmatched_cost and eps are made of -----------------------------------
// keys[0] = the smallest, keys[1] = the largest order key over the entries with 0 <= ind < n_index and a finite value
template <typename T>
__global__ __launch_bounds__(256) void kz_assign_range_kernel(const T* __restrict__ dist, const int64_t* __restrict__ ind, int64_t count,
                                                              int64_t n_index, unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long sh[2];
    if (threadIdx.x == 0) {
        sh[0] = ~0ull;
        sh[1] = 0ull;
    }
    __syncthreads();
    unsigned long long lo = ~0ull, hi = 0ull;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
        const int64_t t = ind[e];
        const double w = (double)dist[e];
        if (t < 0 || t >= n_index || !(fabs(w) <= 1.7976931348623157e308)) continue;
        const unsigned long long key = kz_knnr_key(w);
        lo = key < lo ? key : lo;
        hi = key > hi ? key : hi;
    }
    if (lo <= hi) {
        atomicMin(&sh[0], lo);
        atomicMax(&sh[1], hi);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sh[0] <= sh[1]) {
        atomicMin(keys, sh[0]);
        atomicMax(keys + 1, sh[1]);
    }
}

static double kz_assign_unkey(unsigned long long key) {
    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    double w;
    memcpy(&w, &b, sizeof(w));
    return w;
}

extern "C" int kz_assign_range(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                               double* h_min, double* h_max, int* h_any) {
    const int rcq = kz_match_require("kz_assign_range", ctx, d_dist, dist_dtype, n_q, k);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_assign_range: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    KZ_REQUIRE(h_min && h_max && h_any, "kz_assign_range: null argument");
    *h_min = *h_max = 0.0;
    *h_any = 0;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_ind != nullptr, "kz_assign_range: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    KzPoolBuf<unsigned long long> keys;
    const int rc = keys.alloc(ctx, 2 * sizeof(unsigned long long));
    if (rc != KZ_OK) return rc;
    unsigned long long h_keys[2] = {~0ull, 0ull};
    KZ_HIP(hipMemcpyAsync(keys.get(), h_keys, sizeof(h_keys), hipMemcpyHostToDevice, ctx->stream));
    const int64_t count = n_q * k;
    const dim3 grid(kz_assign_blocks(count)), block(256);
    if (dist_dtype == KZ_F32)
        hipLaunchKernelGGL(kz_assign_range_kernel<float>, grid, block, 0, ctx->stream, (const float*)d_dist, d_ind, count, n_index, keys.get());
    else
        hipLaunchKernelGGL(kz_assign_range_kernel<double>, grid, block, 0, ctx->stream, (const double*)d_dist, d_ind, count, n_index, keys.get());
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipMemcpyAsync(h_keys, keys.get(), sizeof(h_keys), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (h_keys[0] <= h_keys[1]) {
        *h_min = kz_assign_unkey(h_keys[0]);
        *h_max = kz_assign_unkey(h_keys[1]);
        *h_any = 1;
    }
    return KZ_OK;
}
