// ONE-TO-ONE ALIGNMENT: the source-proposing stable matching (deferred acceptance) over neighbour lists.
// Entry (i, c) of dist / ind [n_q, k] with 0 <= ind < n_index is a pair of source row i and target row ind[i, c] with value
// w = dist[i, c]; any other entry (the INT_MAX padding of kz_knn_reduced, a -1) is no pair.  A source row prefers its pairs by
// column, a target row the sources that list it by (kz_knnr_key(w), source row), smaller first.  For fixed preferences the
// source-optimal stable matching is unique: the result does not depend on the order proposals are processed in, and where every row
// is non-decreasing in key order it is the greedy assignment over all pairs sorted by (key, source row, column).
//
// ROUNDS of three launches over the source rows (one thread per row, grid-stride), on the context's stream:
//   1. propose: every free row steps over the columns whose target already holds a pair that beats its own (key, row) -- held pairs
//      only ever improve, so those proposals would lose now and in every later round -- and, if a column is left, atomicMin's its key
//      into the target's proposal word;
//   2. tie:     the proposers whose key is the word atomicMin their row into the target's second word;
//   3. resolve: the one proposer per target that finds (its key, its row) in the two words takes the target: it beat the held pair when
//      it looked in step 1, and nothing has written a held pair since.  It writes the held pair, its own match / col, frees the source
//      it displaced one column on, and resets the two words.  Every other proposer is free again, one column on.
// Integer compares and integer atomics only; no kernel waits for another workgroup; the same arrays come out of every run.
// A round with a proposer advances a column pointer or fills an empty target: at most n_q k + n_index rounds.  A round without one
// changes nothing, so KZ_MATCH_ROUNDS_PER_READ rounds are queued before the host reads the per-round proposer counts.
#include "kz_common.h"
#include "kz_order_key.h"
#include "kz_pool_buf.h"
#include "kz_rows.h"   // KzRowsFixed, KzRowsCsr: the kernels below are instantiated for both (the CSR calls are at the end of the file)

// rounds queued between two reads of the proposer counts: a read costs a stream synchronise, a surplus round three empty launches
// (profiles/one_to_one.md; -DKZ_MATCH_ROUNDS=n builds the variants measured there)
#ifndef KZ_MATCH_ROUNDS
#define KZ_MATCH_ROUNDS 8
#endif
constexpr int KZ_MATCH_ROUNDS_PER_READ = KZ_MATCH_ROUNDS;
constexpr int KZ_MATCH_BLOCKS = 256;   // of 256 threads: one grid covers 65 536 rows, more rows take the grid-stride loop

enum { KZ_MATCH_FREE = 0, KZ_MATCH_PROPOSING = 1, KZ_MATCH_ENGAGED = 2 };
constexpr int KZ_MATCH_NO_ROW = 0x7fffffff;   // the second proposal word of a target nobody proposes to

// working arrays (the context's scoped scratch): per target the held pair and the round's best proposal, per source the next
// column and the state
struct KzMatchState {
    unsigned long long* held_key;   // [n_index] key of the pair the target holds (KZ_KNNR_PAD: none)
    int* held_row;                  // [n_index] its source row (-1: none)
    unsigned long long* prop_key;   // [n_index] smallest key proposed this round (KZ_KNNR_PAD: none)
    int* prop_row;                  // [n_index] smallest row among the proposers with that key (KZ_MATCH_NO_ROW: none)
    int* next;                      // [n_q] the column the row proposes to next (k: the list is used up)
    int* state;                     // [n_q] KZ_MATCH_*
};

__global__ __launch_bounds__(256) void kz_match_init_kernel(KzMatchState s, int n_q, int n_index, int64_t* __restrict__ match,
                                                            int64_t* __restrict__ col) {
    const int stride = gridDim.x * blockDim.x;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t t = tid; t < n_index; t += stride) {
        s.held_key[t] = KZ_KNNR_PAD;
        s.held_row[t] = -1;
        s.prop_key[t] = KZ_KNNR_PAD;
        s.prop_row[t] = KZ_MATCH_NO_ROW;
    }
    for (int64_t i = tid; i < n_q; i += stride) {
        s.next[i] = 0;
        s.state[i] = KZ_MATCH_FREE;
        match[i] = -1;
        col[i] = -1;
    }
}

template <typename T, typename L>
__global__ __launch_bounds__(256) void kz_match_propose_kernel(KzMatchState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                               int n_q, L rows, int64_t n_index, unsigned* __restrict__ n_proposers) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_MATCH_FREE) continue;
        int c = s.next[i];
        const int k = rows.len(i);
        if (c >= k) continue;
        const int64_t e0 = rows.start(i);
        for (; c < k; ++c) {
            const int64_t t = ind[e0 + c];
            if (t < 0 || t >= n_index) continue;   // no pair
            const unsigned long long key = kz_knnr_key((double)dist[e0 + c]);
            const unsigned long long hk = s.held_key[t];
            if (hk < key || (hk == key && s.held_row[t] < (int)i)) continue;   // the target holds a pair that beats this one for good
            atomicMin(s.prop_key + t, key);
            atomicAdd(n_proposers, 1u);
            s.state[i] = KZ_MATCH_PROPOSING;
            break;
        }
        s.next[i] = c;
    }
}

template <typename T, typename L>
__global__ __launch_bounds__(256) void kz_match_tie_kernel(KzMatchState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                           int n_q, L rows) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_MATCH_PROPOSING) continue;
        const int64_t e = rows.start(i) + s.next[i];
        const int64_t t = ind[e];
        if (s.prop_key[t] == kz_knnr_key((double)dist[e])) atomicMin(s.prop_row + t, (int)i);
    }
}

// The winner resets the proposal words that the other proposers of its target read in this launch: they are read and written as
// relaxed agent-scope atomics, and a proposer that is not the winner finds "not mine" in either version -- no proposer has the key
// KZ_KNNR_PAD.  The displaced source is engaged, so no proposer: its own thread reads its state and does nothing, whichever version
// it sees; only the winner writes it.
template <typename T, typename L>
__global__ __launch_bounds__(256) void kz_match_resolve_kernel(KzMatchState s, const T* __restrict__ dist, const int64_t* __restrict__ ind,
                                                               int n_q, L rows, int64_t* __restrict__ match, int64_t* __restrict__ col) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        if (s.state[i] != KZ_MATCH_PROPOSING) continue;
        const int c = s.next[i];
        const int64_t e = rows.start(i) + c;
        const int64_t t = ind[e];
        const unsigned long long key = kz_knnr_key((double)dist[e]);
        const bool won = __hip_atomic_load(s.prop_key + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key &&
                         __hip_atomic_load(s.prop_row + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)i;
        if (!won) {
            s.state[i] = KZ_MATCH_FREE;
            s.next[i] = c + 1;
            continue;
        }
        __hip_atomic_store(s.prop_key + t, KZ_KNNR_PAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(s.prop_row + t, KZ_MATCH_NO_ROW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int old = s.held_row[t];
        s.held_key[t] = key;
        s.held_row[t] = (int)i;
        s.state[i] = KZ_MATCH_ENGAGED;
        match[i] = t;
        col[i] = c;
        if (old >= 0) {   // (next[old] is the column it held the target at)
            s.state[old] = KZ_MATCH_FREE;
            s.next[old] += 1;
            match[old] = -1;
            col[old] = -1;
        }
    }
}

// d_out[i] = d_dist[i, d_col[i]], NaN where d_col[i] < 0
template <typename T, typename L>
__global__ __launch_bounds__(256) void kz_match_values_kernel(const T* __restrict__ dist, const int64_t* __restrict__ col, int n_q, L rows,
                                                              T* __restrict__ out) {
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += stride) {
        const int64_t c = col[i];
        out[i] = c >= 0 && c < rows.len(i) ? dist[rows.start(i) + c] : (T)NAN;
    }
}

// max_rounds: every round with a proposer advances a column pointer or fills an empty target -- entries + n_index
template <typename T, typename L>
static int kz_match_lists_impl(const char* who, kz_ctx* ctx, const T* d_dist, const int64_t* d_ind, int n_q, L rows, int64_t max_rounds,
                               int64_t n_index, int64_t* d_match, int64_t* d_col, int64_t* h_rounds) {
    // (released when the function returns, behind its last synchronise)
    KzPoolBuf<unsigned long long> held_key, prop_key;
    KzPoolBuf<int> held_row, prop_row, next, state;
    KzPoolBuf<unsigned> counts;
    int rc = held_key.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = prop_key.alloc(ctx, (size_t)n_index * 8);
    if (rc == KZ_OK) rc = held_row.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = prop_row.alloc(ctx, (size_t)n_index * 4);
    if (rc == KZ_OK) rc = next.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = state.alloc(ctx, (size_t)n_q * 4);
    if (rc == KZ_OK) rc = counts.alloc(ctx, KZ_MATCH_ROUNDS_PER_READ * sizeof(unsigned));
    if (rc != KZ_OK) return rc;
    const KzMatchState s{held_key.get(), held_row.get(), prop_key.get(), prop_row.get(), next.get(), state.get()};
    const dim3 grid(kz_blocks(n_q, KZ_MATCH_BLOCKS)), block(256);
    hipLaunchKernelGGL(kz_match_init_kernel, dim3(kz_blocks(n_q > n_index ? n_q : n_index, KZ_MATCH_BLOCKS)), block, 0, ctx->stream, s, n_q,
                       (int)n_index, d_match, d_col);
    int64_t rounds = 0, queued = 0;
    for (bool busy = true; busy;) {
        if (queued > max_rounds) {
            kz_set_error("%s: %lld rounds and still a proposer (the bound is %lld)", who, (long long)queued, (long long)max_rounds);
            return KZ_ERR_HIP;
        }
        KZ_HIP(hipMemsetAsync(counts.get(), 0, KZ_MATCH_ROUNDS_PER_READ * sizeof(unsigned), ctx->stream));
        for (int r = 0; r < KZ_MATCH_ROUNDS_PER_READ; ++r) {
            hipLaunchKernelGGL((kz_match_propose_kernel<T, L>), grid, block, 0, ctx->stream, s, d_dist, d_ind, n_q, rows, n_index, counts.get() + r);
            hipLaunchKernelGGL((kz_match_tie_kernel<T, L>), grid, block, 0, ctx->stream, s, d_dist, d_ind, n_q, rows);
            hipLaunchKernelGGL((kz_match_resolve_kernel<T, L>), grid, block, 0, ctx->stream, s, d_dist, d_ind, n_q, rows, d_match, d_col);
        }
        KZ_HIP(hipGetLastError());
        queued += KZ_MATCH_ROUNDS_PER_READ;
        unsigned h_counts[KZ_MATCH_ROUNDS_PER_READ];
        KZ_HIP(hipMemcpyAsync(h_counts, counts.get(), sizeof(h_counts), hipMemcpyDeviceToHost, ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < KZ_MATCH_ROUNDS_PER_READ; ++r) rounds += h_counts[r] != 0;
        busy = h_counts[KZ_MATCH_ROUNDS_PER_READ - 1] != 0;   // (no proposer in a round: none in any later one)
    }
    if (h_rounds) *h_rounds = rounds;
    return KZ_OK;
}

// the launch of kz_match_values_kernel for either layout and value type
template <typename L>
static int kz_match_values_launch(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_col, int64_t n_q, L rows, void* d_out) {
    kz_with_values(dist_dtype, d_dist, [&](auto* dist) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(dist)>>;
        hipLaunchKernelGGL((kz_match_values_kernel<T, L>), dim3(kz_blocks(n_q, KZ_MATCH_BLOCKS)), dim3(256), 0, ctx->stream, dist, d_col, (int)n_q,
                           rows, (T*)d_out);
    });
    KZ_HIP(hipGetLastError());
    return KZ_OK;
}

extern "C" int kz_match_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                              int64_t* d_match, int64_t* d_col, int64_t* h_rounds) {
    const int rcq = kz_match_require("kz_match_lists", ctx, d_dist, dist_dtype, n_q, k);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_match_lists: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    if (h_rounds) *h_rounds = 0;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_ind && d_match && d_col, "kz_match_lists: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_with_values(dist_dtype, d_dist, [&](auto* dist) {
        return kz_match_lists_impl("kz_match_lists", ctx, dist, d_ind, (int)n_q, KzRowsFixed{k}, n_q * k + n_index, n_index, d_match, d_col, h_rounds);
    });
}

extern "C" int kz_match_values(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_col, int64_t n_q, int k, void* d_out) {
    const int rcq = kz_match_require("kz_match_values", ctx, d_dist, dist_dtype, n_q, k);
    if (rcq != KZ_OK) return rcq;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_col && d_out, "kz_match_values: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_match_values_launch(ctx, d_dist, dist_dtype, d_col, n_q, KzRowsFixed{k}, d_out);
}

// ---- the CSR layout --------------------------------------------------------------------------------------------------------------

extern "C" int kz_match_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q,
                            int64_t nnz, int64_t n_index, int64_t* d_match, int64_t* d_col, int64_t* h_rounds) {
    const int rcq = kz_csr_require("kz_match_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "kz_match_csr: dist_dtype must be KZ_F32 or KZ_F64, got %d", dist_dtype);
    if (h_rounds) *h_rounds = 0;
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_match && d_col && (nnz == 0 || (d_ind && d_dist)), "kz_match_csr: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_match_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    return kz_with_values(dist_dtype, d_dist, [&](auto* dist) {
        return kz_match_lists_impl("kz_match_csr", ctx, dist, d_ind, (int)n_q, KzRowsCsr{d_indptr}, nnz + n_index, n_index, d_match, d_col, h_rounds);
    });
}

extern "C" int kz_match_values_csr(kz_ctx* ctx, const int64_t* d_indptr, const void* d_dist, int dist_dtype, const int64_t* d_col, int64_t n_q,
                                   int64_t nnz, void* d_out) {
    const int rcq = kz_csr_require("kz_match_values_csr", ctx, n_q, nnz, 1);
    if (rcq != KZ_OK) return rcq;
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "kz_match_values_csr: dist_dtype must be KZ_F32 or KZ_F64, got %d", dist_dtype);
    if (n_q == 0) return KZ_OK;
    KZ_REQUIRE(d_col && d_out && (nnz == 0 || d_dist), "kz_match_values_csr: null argument");
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_match_values_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    return kz_match_values_launch(ctx, d_dist, dist_dtype, d_col, n_q, KzRowsCsr{d_indptr}, d_out);
}
