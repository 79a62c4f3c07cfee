// THE SINGLE-LINKAGE HIERARCHY OF A PAIR LIST: the minimum spanning forest of the weighted pair graph.  The
// components of the pairs with value <= t, for EVERY t, are the components of the forest edges with value <= t: one loose join plus
// one forest answers every tighter threshold with a components call on at most n_q + n_index - 1 edges (kz_components_edges).
// The graph is kz_components.hip's -- source row i is node i, target row j node n_q + j -- with one more rule: an entry is an edge
// when 0 <= ind[p] < n_index AND its value is not NaN (NaN is <= no threshold).  Edge p comes before p' when
// (kz_knnr_key(w_p), p) < (kz_knnr_key(w_p'), p'), p the entry's flat position: a strict total order, so the forest is unique -- the
// one Kruskal's algorithm builds taking the edges in that order -- and the answer does not depend on the order anything ran in.
//
// BORUVKA IN ROUNDS, one thread per ENTRY (a hub row of 10^5 entries costs what 10^5 entries of short rows cost).  comp[v] is the root
// of v's component at the start of a round, flat (comp[comp[v]] == comp[v]).  A round is five launches:
//   1. reset    best_key[v] = ~0, best_p[v] = INT_MAX;
//   2. offer    every live entry whose ends lie in different components offers its 64-bit key to both with an unsigned atomicMin --
//               behind a relaxed agent-scope load that skips the atomic when the key is not smaller (the word only ever decreases in
//               this launch: a stale read costs an atomic, never correctness; the boundary of a giant component does not send every
//               lane of the chip to one address).  An entry with both ends in one component is dead for good: src[p] <- -1;
//   3. tie      every live entry whose key IS its component's best offers its position p with an int atomicMin, behind the same
//               kind of load.  Two passes because (key, p) does not fit one atomic word; both ends use the SAME (key, p) order, which
//               rules out cycles longer than two among the picks;
//   4. pick     per root with a pick p: mark[p] = 1 (an idempotent store: both ends may pick p), and the root hooks under the other
//               end's root in a SECOND array next[] (comp is only read) -- unless the pick is mutual and this root is the smaller
//               one, which stays; a hook sets the round's flag;
//   5. flatten  comp[v] = the root above v in next[], with path halving (agent-scope loads and stores; a stale parent is still an
//               ancestor, roots are not written: at most n_nodes steps, counted).
// The host READS THE FLAG BACK after every round and stops at the first round that hooked nothing: every round at least halves the
// components that have an edge left, so at most ceil(log2(nodes)) <= 31 rounds hook (32 are run at most); real pair lists need far
// fewer, and a read-back per round costs less than queueing 31 x 5 launches that return at once.
// Then: the exclusive scan of mark[] (kz_scan_flags, kz_pairs.hip's) compacts the forest entries in ascending p -- (widened value, p)
// -- the one-row CSR (value, p) goes through kz_csr_sort_rows (stable by key, ties by p), and (source, target) are read off p.
// Integer atomics and integer arithmetic only; no float atomics; no kernel waits for another workgroup; every loop is bounded.
// TRANSIENT DEVICE MEMORY: 20 bytes per node (comp, next, best_key, best_p) and 12 bytes per entry (src, mark, place), plus the
// sort's second copy (16 bytes per forest edge) when the forest has more than 4096 edges.
#include "kz_common.h"
#include "kz_order_key.h"
#include "kz_pool_buf.h"
#include "kz_rows.h"   // KzRowsFixed, KzRowsCsr, kz_csr_row_of, kz_csr_require, kz_csr_validate, kz_scan_flags

namespace {

constexpr int KZ_FOREST_MAX_ROUNDS = 32;   // 31 rounds that hook at the most, and the one that finds nothing left

__device__ __forceinline__ int64_t kz_fo_row_of(const KzRowsFixed& rows, int64_t, int64_t e) { return e / rows.k; }
__device__ __forceinline__ int64_t kz_fo_row_of(const KzRowsCsr& rows, int64_t n_q, int64_t e) { return kz_csr_row_of(rows.indptr, n_q, e); }

// src[e] = the source row of entry e when it is an edge, else -1; mark[e] = 0; and (the grid covers the nodes too) comp[v] = v
template <typename L, typename T>
__global__ __launch_bounds__(256) void kz_fo_prepare_kernel(const int64_t* __restrict__ ind, const T* __restrict__ dist, L rows, int64_t n_q,
                                                            int64_t n_entries, int64_t n_index, int n_nodes, int* __restrict__ src,
                                                            int* __restrict__ mark, int* __restrict__ comp) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t e = first; e < n_entries; e += stride) {
        const int64_t t = ind[e];
        const T w = dist[e];
        src[e] = (t >= 0 && t < n_index && w == w) ? (int)kz_fo_row_of(rows, n_q, e) : -1;
        mark[e] = 0;
    }
    for (int64_t v = first; v < n_nodes; v += stride) comp[v] = (int)v;
}

__global__ __launch_bounds__(256) void kz_fo_reset_kernel(unsigned long long* __restrict__ best_key, int* __restrict__ best_p, int n_nodes,
                                                          int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t v = first; v < n_nodes; v += stride) {
        best_key[v] = ~0ull;
        best_p[v] = 0x7fffffff;
    }
    if (first == 0) *flag = 0;
}

// Words other workgroups lower in the same launch: relaxed agent-scope loads, served by the L2 (kz_components.hip's rule)
__device__ __forceinline__ void kz_fo_offer_key(unsigned long long* word, unsigned long long key) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(word, key);
}
__device__ __forceinline__ void kz_fo_offer_p(int* word, int p) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) atomicMin(word, p);
}

template <typename T>
__global__ __launch_bounds__(256) void kz_fo_offer_kernel(const int64_t* __restrict__ ind, const T* __restrict__ dist, int64_t n_q, int64_t n_entries,
                                                          const int* __restrict__ comp, int* __restrict__ src,
                                                          unsigned long long* __restrict__ best_key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += stride) {
        const int s = src[e];
        if (s < 0) continue;   // no edge, or inside one component since an earlier round
        const int a = comp[s], b = comp[n_q + ind[e]];
        if (a == b) {
            src[e] = -1;   // (this thread's own word: no other thread reads it in this launch)
            continue;
        }
        const unsigned long long key = kz_knnr_key((double)dist[e]);
        kz_fo_offer_key(best_key + a, key);
        kz_fo_offer_key(best_key + b, key);
    }
}

// (best_key is final: written by the launch before this one)
template <typename T>
__global__ __launch_bounds__(256) void kz_fo_tie_kernel(const int64_t* __restrict__ ind, const T* __restrict__ dist, int64_t n_q, int64_t n_entries,
                                                        const int* __restrict__ comp, const int* __restrict__ src,
                                                        const unsigned long long* __restrict__ best_key, int* __restrict__ best_p) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += stride) {
        const int s = src[e];
        if (s < 0) continue;
        const int a = comp[s], b = comp[n_q + ind[e]];   // (a != b: the offer launch has retired the others)
        const unsigned long long key = kz_knnr_key((double)dist[e]);
        if (best_key[a] == key) kz_fo_offer_p(best_p + a, (int)e);
        if (best_key[b] == key) kz_fo_offer_p(best_p + b, (int)e);
    }
}

// next[v] = where v points after this round: a non-root at its root, a root at itself or, hooked, at the root of its pick's other end.
// Reads comp / best_p / src / ind, writes next / mark / flag: no word is read and written in one launch.
__global__ __launch_bounds__(256) void kz_fo_pick_kernel(const int64_t* __restrict__ ind, int64_t n_q, int n_nodes, const int* __restrict__ comp,
                                                         const int* __restrict__ src, const int* __restrict__ best_p, int* __restrict__ next,
                                                         int* __restrict__ mark, int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += stride) {
        const int c = comp[v];
        int to = c;
        if (c == (int)v) {
            const int p = best_p[v];
            if (p != 0x7fffffff) {
                // mark[p] and *flag are words several workgroups may store to in this launch -- both ends of a mutual pick mark p, every
                // hooking root raises the flag.  Every writer stores the same value 1 and nobody reads either word before the next
                // launch (the flag: before the host's read-back): whichever store lands last, the word is 1.  Relaxed agent-scope
                // stores, as every other word of this file that more than one workgroup touches.
                __hip_atomic_store(mark + p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int u = comp[src[p]], w = comp[n_q + ind[p]];
                const int other = u == c ? w : u;
                const bool stays = best_p[other] == p && c < other;   // a mutual pick: the smaller root stays root
                if (!stays) {
                    to = other;
                    __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        next[v] = to;
    }
}

// comp[v] = the root above v in next[].  Halving stores replace a parent by a higher ancestor of the same tree and never touch a
// root, so whichever version of a word a thread reads names an ancestor; the walk goes strictly up a forest of depth < n_nodes.
__global__ __launch_bounds__(256) void kz_fo_flatten_kernel(int* next, int* __restrict__ comp, int n_nodes) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v0 < n_nodes; v0 += stride) {
        int v = (int)v0, r = v;
        for (int step = 0; step < n_nodes; ++step) {
            const int p = __hip_atomic_load(next + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r = p;
            if (p == v) break;
            const int g = __hip_atomic_load(next + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r = g;
            if (g == p) break;
            __hip_atomic_store(next + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v = g;
        }
        comp[v0] = r;
    }
}

// the marked entries, ascending in p: (widened value, p) at their place; and the one-row indptr of the sort
template <typename T>
__global__ __launch_bounds__(256) void kz_fo_compact_kernel(const T* __restrict__ dist, int64_t n_entries, const int* __restrict__ mark,
                                                            const int* __restrict__ place, int64_t n_edges, double* __restrict__ value,
                                                            int64_t* __restrict__ entry, int64_t* __restrict__ row_ptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t e = first; e < n_entries; e += stride) {
        if (!mark[e]) continue;
        const int at = place[e];   // (< n_edges = place[n_entries], which the host has checked against the room)
        value[at] = (double)dist[e];
        entry[at] = e;
    }
    if (first == 0) {
        row_ptr[0] = 0;
        row_ptr[1] = n_edges;
    }
}

// behind the sort: the two ends of every forest edge from its position
template <typename L>
__global__ __launch_bounds__(256) void kz_fo_ends_kernel(const int64_t* __restrict__ ind, L rows, int64_t n_q, const int64_t* __restrict__ entry,
                                                         int64_t n_edges, int64_t* __restrict__ source, int64_t* __restrict__ target) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_edges; i += stride) {
        const int64_t p = entry[i];
        source[i] = kz_fo_row_of(rows, n_q, p);
        target[i] = ind[p];
    }
}

template <typename L, typename T>
int kz_forest_impl(kz_ctx* ctx, const int64_t* d_ind, const T* d_dist, L rows, int64_t n_q, int64_t n_entries, int64_t n_index, int64_t* d_source,
                   int64_t* d_target, double* d_value, int64_t* d_entry, int64_t* h_n_edges, int64_t* h_n_components, int* h_rounds) {
    const int n_nodes = (int)(n_q + n_index);
    *h_n_edges = 0;
    *h_n_components = n_nodes;
    if (h_rounds) *h_rounds = 0;
    if (n_entries == 0) return KZ_OK;   // every node a component of its own
    const int total = (int)n_entries, n_tiles = (total + 255) / 256;
    // (released when the function returns, behind its last synchronise)
    KzPoolBuf<int> comp, next, best_p, src, mark, place, tile, flag;
    KzPoolBuf<unsigned long long> best_key;
    KzPoolBuf<int64_t> row_ptr;
    int rc = comp.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = next.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = best_p.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = best_key.alloc(ctx, (size_t)n_nodes * 8);
    if (rc == KZ_OK) rc = src.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = mark.alloc(ctx, (size_t)total * 4);
    if (rc == KZ_OK) rc = place.alloc(ctx, ((size_t)total + 1) * 4);
    if (rc == KZ_OK) rc = tile.alloc(ctx, (size_t)n_tiles * 4);
    if (rc == KZ_OK) rc = flag.alloc(ctx, 16);
    if (rc == KZ_OK) rc = row_ptr.alloc(ctx, 16);
    if (rc != KZ_OK) return rc;
    const dim3 nodes(kz_blocks(n_nodes, 4096)), entries(kz_blocks(n_entries, 4096)), both(kz_blocks(n_entries > n_nodes ? n_entries : n_nodes, 4096)),
        wg(256);
    hipLaunchKernelGGL((kz_fo_prepare_kernel<L, T>), both, wg, 0, ctx->stream, d_ind, d_dist, rows, n_q, n_entries, n_index, n_nodes, src.get(),
                       mark.get(), comp.get());
    int rounds = 0;
    for (int round = 0; round < KZ_FOREST_MAX_ROUNDS; ++round) {
        hipLaunchKernelGGL(kz_fo_reset_kernel, nodes, wg, 0, ctx->stream, best_key.get(), best_p.get(), n_nodes, flag.get());
        hipLaunchKernelGGL((kz_fo_offer_kernel<T>), entries, wg, 0, ctx->stream, d_ind, d_dist, n_q, n_entries, (const int*)comp.get(), src.get(),
                           best_key.get());
        hipLaunchKernelGGL((kz_fo_tie_kernel<T>), entries, wg, 0, ctx->stream, d_ind, d_dist, n_q, n_entries, (const int*)comp.get(),
                           (const int*)src.get(), (const unsigned long long*)best_key.get(), best_p.get());
        hipLaunchKernelGGL(kz_fo_pick_kernel, nodes, wg, 0, ctx->stream, d_ind, n_q, n_nodes, (const int*)comp.get(), (const int*)src.get(),
                           (const int*)best_p.get(), next.get(), mark.get(), flag.get());
        hipLaunchKernelGGL(kz_fo_flatten_kernel, nodes, wg, 0, ctx->stream, next.get(), comp.get(), n_nodes);
        KZ_HIP(hipGetLastError());
        int h_flag = 0;
        KZ_HIP(hipMemcpyAsync(&h_flag, flag.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        KZ_HIP(hipStreamSynchronize(ctx->stream));
        if (!h_flag) break;
        ++rounds;
    }
    if (h_rounds) *h_rounds = rounds;
    kz_scan_flags(ctx, mark.get(), total, tile.get(), place.get());
    KZ_HIP(hipGetLastError());
    int h_edges = 0;
    KZ_HIP(hipMemcpyAsync(&h_edges, place.get() + total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    if (h_edges < 0 || h_edges >= n_nodes) {   // (a forest has fewer edges than nodes: nothing is written behind the caller's room)
        kz_set_error("kz_forest: %d marked entries for %d nodes -- not a forest (internal error)", h_edges, n_nodes);
        return KZ_ERR_HIP;
    }
    *h_n_edges = h_edges;
    *h_n_components = (int64_t)n_nodes - h_edges;
    if (h_edges == 0) return KZ_OK;
    hipLaunchKernelGGL((kz_fo_compact_kernel<T>), entries, wg, 0, ctx->stream, d_dist, n_entries, (const int*)mark.get(), (const int*)place.get(),
                       (int64_t)h_edges, d_value, d_entry, row_ptr.get());
    KZ_HIP(hipGetLastError());
    // one row of h_edges entries, ascending by (key, p): positions are below 2^31 - 1 as the sort's ids must be
    rc = kz_csr_sort_rows(ctx, row_ptr.get(), 1, h_edges, 0x7ffffffeLL, d_entry, d_value);
    if (rc != KZ_OK) return rc;
    hipLaunchKernelGGL((kz_fo_ends_kernel<L>), dim3(kz_blocks(h_edges, 4096)), wg, 0, ctx->stream, d_ind, rows, n_q, (const int64_t*)d_entry,
                       (int64_t)h_edges, d_source, d_target);
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

// the checks both layouts share, all before anything is launched
int kz_fo_require(const char* who, int dist_dtype, int64_t n_q, int64_t n_entries, int64_t n_index, const void* d_ind, const void* d_dist,
                  const void* d_source, const void* d_target, const void* d_value, const void* d_entry, const void* h_n_edges,
                  const void* h_n_components) {
    KZ_REQUIRE(dist_dtype == KZ_F32 || dist_dtype == KZ_F64, "%s: dist_dtype must be KZ_F32 or KZ_F64, got %d", who, dist_dtype);
    if (n_q + n_index >= 0x7fffffffLL) {
        kz_set_error("%s: n_q + n_index = %lld nodes, the limit is 2^31 - 2 (node ids are int32)", who, (long long)(n_q + n_index));
        return KZ_ERR_UNSUPPORTED;
    }
    KZ_REQUIRE(h_n_edges && h_n_components && d_source && d_target && d_value && d_entry, "%s: null argument", who);
    KZ_REQUIRE(n_entries == 0 || (d_ind && d_dist), "%s: null argument", who);
    return KZ_OK;
}

}  // namespace

extern "C" int kz_forest_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, const void* d_dist, int dist_dtype, int64_t n_q, int64_t nnz,
                             int64_t n_index, int64_t* d_source, int64_t* d_target, double* d_value, int64_t* d_entry, int64_t* h_n_edges,
                             int64_t* h_n_components, int* h_rounds) {
    const int rcq = kz_csr_require("kz_forest_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    const int rcf = kz_fo_require("kz_forest_csr", dist_dtype, n_q, nnz, n_index, d_ind, d_dist, d_source, d_target, d_value, d_entry, h_n_edges,
                                  h_n_components);
    if (rcf != KZ_OK) return rcf;
    *h_n_edges = 0;
    *h_n_components = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_forest_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    return kz_with_values(dist_dtype, d_dist, [&](auto dist) {
        return kz_forest_impl(ctx, d_ind, dist, KzRowsCsr{d_indptr}, n_q, nnz, n_index, d_source, d_target, d_value, d_entry, h_n_edges,
                              h_n_components, h_rounds);
    });
}

extern "C" int kz_forest_lists(kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index,
                               int64_t* d_source, int64_t* d_target, double* d_value, int64_t* d_entry, int64_t* h_n_edges,
                               int64_t* h_n_components, int* h_rounds) {
    KZ_REQUIRE(ctx != nullptr, "kz_forest_lists: null context");
    KZ_REQUIRE(k >= 1, "kz_forest_lists: lists of at least one column, got k = %d", k);
    KZ_REQUIRE(n_q >= 0 && n_q < 0x7fffffffLL, "kz_forest_lists: n_q = %lld is outside [0, 2^31 - 1)", (long long)n_q);
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_forest_lists: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    const int64_t n_entries = n_q * (int64_t)k;   // (< 2^62)
    if (n_entries >= 0x7fffffffLL) {
        kz_set_error("kz_forest_lists: %lld list entries, the limit is 2^31 - 2", (long long)n_entries);
        return KZ_ERR_UNSUPPORTED;
    }
    const int rcf = kz_fo_require("kz_forest_lists", dist_dtype, n_q, n_entries, n_index, d_ind, d_dist, d_source, d_target, d_value, d_entry,
                                  h_n_edges, h_n_components);
    if (rcf != KZ_OK) return rcf;
    *h_n_edges = 0;
    *h_n_components = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_with_values(dist_dtype, d_dist, [&](auto dist) {
        return kz_forest_impl(ctx, d_ind, dist, KzRowsFixed{k}, n_q, n_entries, n_index, d_source, d_target, d_value, d_entry, h_n_edges,
                              h_n_components, h_rounds);
    });
}
