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
#include "kz_rows.h"   // KzRowsFixed, KzRowsCsr: the row-walking kernels are instantiated for both
#include <type_traits>

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

// One pass over the columns c = first, first + STEP, ... < k of the row that starts at entry e0, in ascending order: v1 = the largest
// v, c_best = the first column with it (t_best, p_best: its target and price), v2 = the largest v of the other columns visited taken
// together with -u.  STEP 1 is a whole row on one lane; STEP 64 one lane's share of a row that a wave takes (kz_assign_wave_merge).
// SHARED: prices may have been written by another wave earlier in this launch (the tail kernel).
template <typename T, bool SHARED, int STEP>
__device__ __forceinline__ void kz_assign_scan(const KzAssignState& s, const T* __restrict__ dist, const int64_t* __restrict__ ind, int64_t e0,
                                               int first, int k, int64_t n_index, double u, double& v1, double& v2, int& c_best,
                                               int64_t& t_best, double& p_best) {
    v1 = -INFINITY;
    v2 = -u;
    p_best = 0.0;
    c_best = -1;
    t_best = -1;
    // KZ_ASSIGN_CHUNK columns at a time: their ids and values, then their prices, are loads that do not wait for each other; the
    // compares run in column order (a column past the end, or no pair, has t = -1 and reads the price of target 0 for nothing)
    for (int c0 = first; c0 < k; c0 += KZ_ASSIGN_CHUNK * STEP) {
        int64_t t[KZ_ASSIGN_CHUNK];
        double w[KZ_ASSIGN_CHUNK], p[KZ_ASSIGN_CHUNK];
#pragma unroll
        for (int j = 0; j < KZ_ASSIGN_CHUNK; ++j) {
            const bool in = c0 + j * STEP < k;
            const int64_t e = e0 + (in ? c0 + j * STEP : c0);
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
                c_best = c0 + j * STEP;
                t_best = t[j];
                p_best = p[j];
            } else if (v > v2) {
                v2 = v;
            }
        }
    }
}

// The bid of a FREE row (its entries: e0 .. e0 + k - 1) under the current prices -> false: no pair column is strictly better than
// staying out.
template <typename T, bool SHARED>
__device__ __forceinline__ bool kz_assign_bid(const KzAssignState& s, const T* __restrict__ dist, const int64_t* __restrict__ ind, int64_t e0,
                                              int k, int64_t n_index, double u, double eps, int& c_best, int64_t& t_best, double& bid) {
    double v1, v2, p_best;
    kz_assign_scan<T, SHARED, 1>(s, dist, ind, e0, 0, k, n_index, u, v1, v2, c_best, t_best, p_best);
    if (!(v1 > -u)) return false;
    bid = (p_best + (v1 - v2)) + eps;
    return true;
}

// The 64 lanes' scans of one row (lane l: the columns l, l + 64, ...) merged into the scan of the whole row, in every lane.  Two
// partial scans A and B of disjoint column sets merge EXACTLY, by compares alone: the larger v1 wins, equal v1 the smaller column
// (a lane without a pair column has v1 = -inf and c = INT_MAX), and v2 = the largest of both v2 and the LOSING v1 -- the largest v of
// every column but the winner's.  That is what the one-lane scan computes, so the bid made of it has the same bits.  The rule is
// symmetric: both partners of an exchange end with the same triple.
__device__ __forceinline__ void kz_assign_wave_merge(double& v1, int& c, double& v2) {
    if (c < 0) c = 0x7fffffff;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const double o1 = __shfl_xor(v1, sh, 64), o2 = __shfl_xor(v2, sh, 64);
        const int oc = __shfl_xor(c, sh, 64);
        const bool other = o1 > v1 || (o1 == v1 && oc < c);
        const double lose = other ? v1 : o1;
        double m2 = o2 > v2 ? o2 : v2;
        m2 = lose > m2 ? lose : m2;
        v1 = other ? o1 : v1;
        c = other ? oc : c;
        v2 = m2;
    }
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

// (a row the layout calls long is left to kz_assign_bid_long_kernel, queued behind this kernel in the same round)
template <typename T, typename L>
__global__ __launch_bounds__(256) void kz_assign_bid_kernel(KzAssignState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                            int n_q, L rows, int64_t n_index, double u, double eps) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_FREE || rows.is_long(i)) continue;
        int c;
        int64_t t;
        double bid;
        if (!kz_assign_bid<T, false>(s, dist, ind, rows.start(i), rows.len(i), n_index, u, eps, c, t, bid)) {
            s.state[i] = KZ_ASSIGN_OUT;
            continue;
        }
        atomicMax(s.bid_key + t, kz_knnr_key(bid));
        s.bid_col[i] = c;
        s.bid_val[i] = bid;
        s.state[i] = KZ_ASSIGN_BIDDING;
    }
}

// THE LONG ROWS of a CSR (more than KZ_CSR_LONG_ROW entries): one wave per row, four rows per workgroup, wave r the row
// long_rows[r] -- indexed by rank in the ordered list kz_assign_long_rows_kernel wrote, so nothing here depends on an order of
// arrival.  Lane l scans the columns l, l + 64, ... with KZ_ASSIGN_CHUNK loads in flight, the butterfly merges the 64 scans, and
// lane 0 bids as the thread of kz_assign_bid_kernel does.  No price is written in a bid launch: re-reading the best target's
// price gives the value the scan used.
template <typename T>
__global__ __launch_bounds__(256) void kz_assign_bid_long_kernel(KzAssignState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                                 KzRowsCsr rows, const int* __restrict__ long_rows, int n_long, int64_t n_index,
                                                                 double u, double eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_long) return;   // (wave-uniform, as the next)
    const int i = long_rows[r];
    if (s.state[i] != KZ_ASSIGN_FREE) return;
    const int64_t e0 = rows.start(i);
    double v1, v2, p_best;
    int c;
    int64_t t;
    kz_assign_scan<T, false, 64>(s, dist, ind, e0, lane, rows.len(i), n_index, u, v1, v2, c, t, p_best);
    kz_assign_wave_merge(v1, c, v2);
    if (lane != 0) return;
    if (!(v1 > -u)) {
        s.state[i] = KZ_ASSIGN_OUT;
        return;
    }
    t = ind[e0 + c];
    const double bid = (__longlong_as_double((long long)s.price[t]) + (v1 - v2)) + eps;
    atomicMax(s.bid_key + t, kz_knnr_key(bid));
    s.bid_col[i] = c;
    s.bid_val[i] = bid;
    s.state[i] = KZ_ASSIGN_BIDDING;
}

// long_rows[0 .. *n_long) = the long rows in ASCENDING row order, by ONE workgroup: 1024 rows per step, a row's place = the long
// rows of the earlier steps + those of the earlier waves of its step + those of the lower lanes of its wave (ballot and popcount).
// No atomic: the list is the same in every run.  capacity: the places long_rows has (the host sizes it by nnz / (KZ_CSR_LONG_ROW + 1)).
__global__ __launch_bounds__(1024) void kz_assign_long_rows_kernel(KzRowsCsr rows, int n_q, int capacity, int* __restrict__ long_rows,
                                                                   int* __restrict__ n_long) {
    __shared__ int wave_n[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int64_t i0 = 0; i0 < n_q; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const bool is = i < n_q && rows.is_long(i);
        const unsigned long long mask = __ballot(is);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wave_n[w] : 0;
            total += wave_n[w];
        }
        const int slot = base + before + __popcll(mask & ((1ull << lane) - 1ull));
        if (is && slot < capacity) long_rows[slot] = (int)i;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_long = base;
}

template <typename L>
__global__ __launch_bounds__(256) void kz_assign_tie_kernel(KzAssignState s, const int64_t* __restrict__ ind, int n_q, L rows) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_BIDDING) continue;
        const int64_t t = ind[rows.start(i) + s.bid_col[i]];
        if (s.bid_key[t] == kz_knnr_key(s.bid_val[i])) atomicMin(s.bid_row + t, (int)i);
    }
}

// The winner resets the bid words that the other bidders of its target read in this launch: they are read and written as relaxed
// agent-scope atomics, and a bidder that is not the winner finds "not mine" in either version -- no bidder has the key
// KZ_ASSIGN_NO_BID.  The displaced row is an owner, so no bidder; only the winner of its target writes its state.
// free_after[0]: the rows FREE once the round is over (losers and displaced owners); free_after[1]: the long ones among them (a
// layout without long rows never touches it).
template <typename L>
__global__ __launch_bounds__(256) void kz_assign_resolve_kernel(KzAssignState s, const int64_t* __restrict__ ind, int n_q, L rows,
                                                                int64_t* __restrict__ match, int64_t* __restrict__ col,
                                                                unsigned* __restrict__ free_after) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_ASSIGN_BIDDING) continue;
        const int c = s.bid_col[i];
        const int64_t t = ind[rows.start(i) + c];
        const double bid = s.bid_val[i];
        const bool won = KZ_RLX_LOAD(s.bid_key + t) == kz_knnr_key(bid) && KZ_RLX_LOAD(s.bid_row + t) == (int)i;
        if (!won) {
            s.state[i] = KZ_ASSIGN_FREE;
            atomicAdd(free_after, 1u);
            if (rows.is_long(i)) atomicAdd(free_after + 1, 1u);
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
            if (rows.is_long(old)) atomicAdd(free_after + 1, 1u);
        }
    }
}

// every memory operation of this wave has completed (stores and atomics are acknowledged by the L2) before it joins the barrier
__device__ __forceinline__ void kz_assign_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// out[0] = rounds run, out[1] = rows still FREE, out[2] = 1 if more rows were FREE than the workgroup has threads (nothing was done),
// out[3] = the long rows among out[1].  A bidder here is ONE LANE, so the launch ends after the round that frees a long row (a short
// row's bid displaced it): the host goes back to grid-wide rounds, where the row bids with a wave, until no long row is FREE.  The
// rounds are the same rounds either way.
template <typename T, typename L>
__global__ __launch_bounds__(KZ_ASSIGN_TAIL_MAX) void kz_assign_tail_kernel(KzAssignState s, const T* __restrict__ dist,
                                                                            const int64_t* __restrict__ ind, int n_q, L rows, int64_t n_index,
                                                                            double u, double eps, int round_limit, int64_t* match,
                                                                            int64_t* col, int* __restrict__ out) {
    __shared__ int queue[2][KZ_ASSIGN_TAIL_MAX];
    __shared__ int queue_n[2];
    __shared__ int queue_long[2];   // the long rows pushed into queue[x]
    const int tid = threadIdx.x;
    if (tid == 0) queue_n[0] = queue_n[1] = queue_long[0] = queue_long[1] = 0;
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
            out[3] = 0;
        }
        return;
    }
    int cur = 0, r = 0, n_long_cur = 0;
    for (; r < round_limit && n_cur > 0 && n_long_cur == 0; ++r) {
        const int nxt = cur ^ 1;
        if (tid == 0) queue_n[nxt] = queue_long[nxt] = 0;
        bool bidding = false;
        int i = -1, c = -1;
        int64_t t = -1;
        double bid = 0.0;
        unsigned long long key = 0ull;
        if (tid < n_cur) {
            i = queue[cur][tid];
            bidding = kz_assign_bid<T, true>(s, dist, ind, rows.start(i), rows.len(i), n_index, u, eps, c, t, bid);
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
                if (rows.is_long(i)) atomicAdd(&queue_long[nxt], 1);
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
                    if (rows.is_long(old)) atomicAdd(&queue_long[nxt], 1);
                }
            }
        }
        kz_assign_barrier();
        cur = nxt;
        n_cur = queue_n[cur];
        n_long_cur = queue_long[cur];
    }
    if (tid == 0) {
        out[0] = r;
        out[1] = n_cur;
        out[2] = 0;
        out[3] = n_long_cur;
    }
}

// nnz: the entries of a CSR (sizes the list of its long rows); unused for the fixed layout
template <typename T, typename L>
static int kz_assign_lists_impl(const char* who, kz_ctx* ctx, const T* d_dist, const int64_t* d_ind, int n_q, L rows, int64_t nnz,
                                int64_t n_index, double u, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col,
                                double* d_price, int64_t* h_rounds, int* h_converged) {
    constexpr bool CSR = std::is_same<L, KzRowsCsr>::value;
    // (released when the function returns, behind its last synchronise)
    KzPoolBuf<unsigned long long> price, bid_key;
    KzPoolBuf<int> owner, bid_row, state, bid_col, tail_out, long_rows;
    KzPoolBuf<double> bid_val;
    KzPoolBuf<unsigned> counts;
    // (at most nnz / (KZ_CSR_LONG_ROW + 1) rows are long; the last place holds their number)
    const int64_t long_cap64 = CSR ? nnz / ((int64_t)KZ_CSR_LONG_ROW + 1) : 0;
    const int long_cap = (int)(long_cap64 < n_q ? long_cap64 : n_q);
    int rc = KZ_OK;
    if (!d_price) rc = price.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = bid_key.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = owner.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = bid_row.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = state.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = bid_col.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = bid_val.alloc(ctx, (size_t)n_q * 8);
    if (rc == KZ_OK) rc = counts.alloc(ctx, 2 * KZ_ASSIGN_WIDE_ROUNDS * sizeof(unsigned));
    if (rc == KZ_OK) rc = tail_out.alloc(ctx, 4 * sizeof(int));
    if (rc == KZ_OK && long_cap > 0) rc = long_rows.alloc(ctx, ((size_t)long_cap + 1) * sizeof(int));
    if (rc != KZ_OK) return rc;
    const KzAssignState s{d_price ? (unsigned long long*)d_price : price.get(), owner.get(), bid_key.get(), bid_row.get(), state.get(),
                          bid_col.get(), bid_val.get()};
    const dim3 grid(kz_blocks(n_q, KZ_ASSIGN_BLOCKS)), block(256);
    hipLaunchKernelGGL(kz_assign_init_kernel, dim3(kz_blocks(n_q > n_index ? n_q : n_index, KZ_ASSIGN_BLOCKS)), block, 0, ctx->stream, s, n_q,
                       (int)n_index, d_match, d_col);
    KZ_HIP(hipGetLastError());
    int n_long = 0;   // the long rows of the call, found once: every row starts FREE, so they are the long rows FREE now
    if constexpr (CSR) {
        if (long_cap > 0) {
            hipLaunchKernelGGL(kz_assign_long_rows_kernel, dim3(1), dim3(1024), 0, ctx->stream, rows, n_q, long_cap, long_rows.get(),
                               long_rows.get() + long_cap);
            KZ_HIP(hipGetLastError());
            KZ_HIP(hipMemcpyAsync(&n_long, long_rows.get() + long_cap, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            KZ_HIP(hipStreamSynchronize(ctx->stream));
            if (n_long < 0 || n_long > long_cap) {
                kz_set_error("%s: %d long rows where at most %d fit the entries", who, n_long, long_cap);
                return KZ_ERR_HIP;
            }
        }
    }
    int64_t rounds = 0, n_free = n_q, n_long_free = n_long;   // the rows FREE now, and the long ones among them (exact after every read)
    while (n_free > 0 && rounds < max_rounds) {
        const int64_t left = max_rounds - rounds;
        if (tail_rows >= 0 && n_free <= tail_rows && n_long_free == 0) {
            const int limit = (int)(left < KZ_ASSIGN_TAIL_ROUNDS ? left : KZ_ASSIGN_TAIL_ROUNDS);
            int threads = (int)((n_free + 63) / 64 * 64);
            threads = threads < 256 ? 256 : threads;   // (the gather of the FREE rows walks all n_q states)
            hipLaunchKernelGGL((kz_assign_tail_kernel<T, L>), dim3(1), dim3(threads), 0, ctx->stream, s, d_dist, d_ind, n_q, rows, n_index, u, eps,
                               limit, d_match, d_col, tail_out.get());
            KZ_HIP(hipGetLastError());
            int h_out[4];
            KZ_HIP(hipMemcpyAsync(h_out, tail_out.get(), sizeof(h_out), hipMemcpyDeviceToHost, ctx->stream));
            KZ_HIP(hipStreamSynchronize(ctx->stream));
            if (h_out[2] != 0 || h_out[1] > n_free || (h_out[0] == 0 && h_out[1] != 0)) {
                kz_set_error("%s: the tail kernel found %d FREE rows where at most %lld were expected", who, h_out[1], (long long)n_free);
                return KZ_ERR_HIP;
            }
            rounds += h_out[0];
            n_free = h_out[1];
            n_long_free = h_out[3];
            continue;
        }
        const int nr = (int)(left < KZ_ASSIGN_WIDE_ROUNDS ? left : KZ_ASSIGN_WIDE_ROUNDS);
        KZ_HIP(hipMemsetAsync(counts.get(), 0, 2 * KZ_ASSIGN_WIDE_ROUNDS * sizeof(unsigned), ctx->stream));
        for (int r = 0; r < nr; ++r) {
            hipLaunchKernelGGL((kz_assign_bid_kernel<T, L>), grid, block, 0, ctx->stream, s, d_dist, d_ind, n_q, rows, n_index, u, eps);
            if constexpr (CSR) {
                if (n_long > 0)
                    hipLaunchKernelGGL(kz_assign_bid_long_kernel<T>, dim3((unsigned)((n_long + 3) / 4)), block, 0, ctx->stream, s, d_dist, d_ind, rows,
                                       (const int*)long_rows.get(), n_long, n_index, u, eps);
            }
            hipLaunchKernelGGL(kz_assign_tie_kernel<L>, grid, block, 0, ctx->stream, s, d_ind, n_q, rows);
            hipLaunchKernelGGL(kz_assign_resolve_kernel<L>, grid, block, 0, ctx->stream, s, d_ind, n_q, rows, d_match, d_col, counts.get() + 2 * r);
        }
        KZ_HIP(hipGetLastError());
        unsigned h_counts[2 * KZ_ASSIGN_WIDE_ROUNDS];
        KZ_HIP(hipMemcpyAsync(h_counts, counts.get(), sizeof(h_counts), hipMemcpyDeviceToHost, ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < nr && n_free > 0; ++r) {   // (a round counts when a row was FREE at its start)
            rounds += 1;
            n_free = h_counts[2 * r];
            n_long_free = h_counts[2 * r + 1];
        }
    }
    if (h_rounds) *h_rounds = rounds;
    if (h_converged) *h_converged = n_free == 0;
    return KZ_OK;
}

// the option checks kz_assign_lists and kz_assign_csr share
static int kz_assign_require_options(const char* who, double unmatched_cost, double eps, int64_t max_rounds, int tail_rows) {
    KZ_REQUIRE(fabs(unmatched_cost) <= 1.7976931348623157e308, "%s: unmatched_cost must be finite, got %g", who, unmatched_cost);
    KZ_REQUIRE(eps > 0.0 && eps <= 1.7976931348623157e308, "%s: eps must be positive and finite, got %g", who, eps);
    KZ_REQUIRE(max_rounds >= 0, "%s: max_rounds = %lld is negative", who, (long long)max_rounds);
    KZ_REQUIRE(tail_rows <= KZ_ASSIGN_TAIL_MAX, "%s: tail_rows = %d is above %d, the rows one workgroup takes", who, tail_rows, KZ_ASSIGN_TAIL_MAX);
    return KZ_OK;
}

extern "C" int kz_assign_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                               double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col,
                               double* d_price, int64_t* h_rounds, int* h_converged) {
    const int rcq = kz_match_require("kz_assign_lists", ctx, d_dist, dist_dtype, n_q, k);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_assign_lists: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    const int rco = kz_assign_require_options("kz_assign_lists", unmatched_cost, eps, max_rounds, tail_rows);
    if (rco != KZ_OK) return rco;
    if (h_rounds) *h_rounds = 0;
    if (h_converged) *h_converged = 1;
    KZ_HIP(hipSetDevice(ctx->device));
    if (d_price && n_q == 0) KZ_HIP(hipMemsetAsync(d_price, 0, (size_t)n_index * sizeof(double), ctx->stream));
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_ind && d_match && d_col, "kz_assign_lists: null argument");
    if (tail_rows == 0) tail_rows = KZ_ASSIGN_TAIL_MAX;
    return kz_with_values(dist_dtype, d_dist, [&](auto* dist) {
        return kz_assign_lists_impl("kz_assign_lists", ctx, dist, d_ind, (int)n_q, KzRowsFixed{k}, 0, n_index, unmatched_cost, eps, max_rounds,
                                    tail_rows, d_match, d_col, d_price, h_rounds, h_converged);
    });
}

extern "C" int kz_assign_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                             int64_t nnz, int64_t n_index, double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match,
                             int64_t* d_col, double* d_price, int64_t* h_rounds, int* h_converged) {
    const int rcq = kz_csr_require("kz_assign_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "kz_assign_csr: dist_dtype must be KZ_F32 or KZ_F64, got %d", dist_dtype);
    const int rco = kz_assign_require_options("kz_assign_csr", unmatched_cost, eps, max_rounds, tail_rows);
    if (rco != KZ_OK) return rco;
    if (h_rounds) *h_rounds = 0;
    if (h_converged) *h_converged = 1;
    KZ_HIP(hipSetDevice(ctx->device));
    if (d_price && n_q == 0) KZ_HIP(hipMemsetAsync(d_price, 0, (size_t)n_index * sizeof(double), ctx->stream));
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_match && d_col && (nnz == 0 || (d_ind && d_dist)), "kz_assign_csr: null argument");
    const int rcv = kz_csr_validate("kz_assign_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    if (tail_rows == 0) tail_rows = KZ_ASSIGN_TAIL_MAX;
    return kz_with_values(dist_dtype, d_dist, [&](auto* dist) {
        return kz_assign_lists_impl("kz_assign_csr", ctx, dist, d_ind, (int)n_q, KzRowsCsr{d_indptr}, nnz, n_index, unmatched_cost, eps, max_rounds,
                                    tail_rows, d_match, d_col, d_price, h_rounds, h_converged);
    });
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

// the range kernel over `count` entries and its read-out
static int kz_assign_range_impl(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t count, int64_t n_index,
                                double* h_min, double* h_max, int* h_any) {
    KzPoolBuf<unsigned long long> keys;
    const int rc = keys.alloc(ctx, 2 * sizeof(unsigned long long));
    if (rc != KZ_OK) return rc;
    unsigned long long h_keys[2] = {~0ull, 0ull};
    KZ_HIP(hipMemcpyAsync(keys.get(), h_keys, sizeof(h_keys), hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid(kz_blocks(count, KZ_ASSIGN_BLOCKS)), block(256);
    kz_with_values(dist_dtype, d_dist, [&](auto* dist) {   // (the kernel's T follows from the pointer)
        hipLaunchKernelGGL(kz_assign_range_kernel, grid, block, 0, ctx->stream, dist, d_ind, count, n_index, keys.get());
    });
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
    return kz_assign_range_impl(ctx, d_dist, dist_dtype, d_ind, n_q * k, n_index, h_min, h_max, h_any);
}

// (reads dist / ind as flat arrays of nnz entries: indptr takes no part, the signature keeps the CSR calls alike)
extern "C" int kz_assign_range_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                                   int64_t nnz, int64_t n_index, double* h_min, double* h_max, int* h_any) {
    const int rcq = kz_csr_require("kz_assign_range_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "kz_assign_range_csr: dist_dtype must be KZ_F32 or KZ_F64, got %d", dist_dtype);
    KZ_REQUIRE(h_min && h_max && h_any, "kz_assign_range_csr: null argument");
    *h_min = *h_max = 0.0;
    *h_any = 0;
    if (nnz == 0) return KZ_OK;
    KZ_REQUIRE(d_ind && d_dist, "kz_assign_range_csr: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_assign_range_impl(ctx, d_dist, dist_dtype, d_ind, nnz, n_index, h_min, h_max, h_any);
}
