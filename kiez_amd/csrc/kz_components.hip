// ENTITY CLUSTERS: the connected components of a pair list -- the transitive closure of the pairs that
// kz_radius_neighbors, kz_lists_combine or anything else produced, beside the one-to-one steps (kz_match.hip, kz_assign.hip) and the
// soft one (kz_softmin_lists.hip).  The graph is bipartite: source row i is node i, target row j is node n_q + j, and entry (i, t) of
// the list with 0 <= t < n_index is an edge; any other entry is no pair (kz_match_lists' rule).  Every node gets the number of its
// component, components counted 0 .. C - 1 in the order of their smallest node; every component its number of source and of target
// rows.  Three front ends feed the same stages: a CSR, fixed-width lists, and an edge array (kz_components_edges: what labels a cut
// of kz_forest.hip's forest).
//
// UNION-FIND ON int32 PARENT WORDS WITH parent[v] <= v, ALWAYS.  The invariant makes every tree acyclic and every walk a sequence of
// strictly decreasing node ids, and the root of a finished tree the smallest node of its component: the answer does not depend on
// the order anything ran in.  Five stages, each a launch (or three) on the context's stream:
//   1. init     parent[v] = v;
//   2. hook     one thread per ENTRY (the row of an entry by binary search in indptr, or e / k: a hub row of 10^5 entries costs what
//               10^5 entries of short rows cost): find the two roots with path halving, compare-and-swap the parent word of the
//               LARGER root from itself to the smaller one; on failure go on from the value the swap read;
//   3. flatten  root[v] = the root of v, into a second array (parent is only read: no word is read and written in one launch);
//   4. ids      the exclusive prefix sum of the flags root[v] == v over all nodes (tile sums, one workgroup over the tile totals, the
//               tile again: kz_pairs.hip's scheme), label[v] = that prefix at root[v], C = the total;
//   5. sizes    (when asked) integer adds into size_q[label] / size_t[label], pre-aggregated per wave.
// Integer arithmetic and integer atomics only; no kernel waits for another workgroup; every loop is bounded (each stage says by
// what).  Integer adds commute: two calls give identical bytes.
#include "kz_common.h"
#include "kz_pool_buf.h"
#include "kz_rows.h"   // KzRowsFixed, KzRowsCsr, kz_csr_row_of, kz_csr_require, kz_csr_validate

namespace {

// (uniform) the row that holds entry e, per layout
__device__ __forceinline__ int64_t kz_cc_row_of(const KzRowsFixed& rows, int64_t, int64_t e) { return e / rows.k; }
__device__ __forceinline__ int64_t kz_cc_row_of(const KzRowsCsr& rows, int64_t n_q, int64_t e) { return kz_csr_row_of(rows.indptr, n_q, e); }

// Parent words are written by other workgroups in the same launch: relaxed agent-scope atomics, served by the L2 and never by a
// stale L1 line (DESIGN.md section 3.1h has the same rule for the auction's price words).
__device__ __forceinline__ int kz_cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void kz_cc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above v, with path halving: parent[v] <- its grandparent on the way.  Every step goes to a strictly smaller node or
// returns: at most v steps.  The halving store never touches a root (p != v: only a root's word is ever compare-and-swapped, and
// only from v to something else, once), and what it writes is an ancestor of v below v in id -- whichever of two racing stores
// lands last, parent[v] <= v holds and parent[v] is an ancestor of v.
__device__ __forceinline__ int kz_cc_find(int* parent, int v) {
    for (;;) {
        const int p = kz_cc_load(parent + v);
        if (p == v) return v;
        const int g = kz_cc_load(parent + p);
        if (g == p) return p;
        kz_cc_store(parent + v, g);
        v = g;
    }
}

__global__ __launch_bounds__(256) void kz_cc_init_kernel(int* __restrict__ parent, int n_nodes) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += stride) parent[v] = (int)v;
}

// A STALE PARENT IS STILL AN ANCESTOR.  Links only ever hang a root under a smaller node and halving only replaces a parent by a
// higher ancestor, so whatever version of a word a thread reads names a node that is (and stays) above it in its tree: a stale read
// costs steps, never correctness.  The one write that decides anything, the link, is a compare-and-swap that succeeds only while
// the word still says "root".
// The link loop: (a, b) are two nodes of the two trees, a != b.  hi = max, lo = min; the swap hangs hi under lo while hi is a root.
// When it fails, hi had a parent `seen` < hi already: go on with (root above seen, lo) -- both below hi, so the larger of the pair
// strictly decreases: at most max(a, b) rounds.  lo may have stopped being a root meanwhile: the link is then to an inner node,
// which keeps parent[v] <= v and joins the two trees all the same.
__device__ __forceinline__ void kz_cc_link(int* parent, int a, int b) {
    a = kz_cc_find(parent, a);
    b = kz_cc_find(parent, b);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        a = kz_cc_find(parent, seen);   // (seen < hi: parent[hi] <= hi and it is not hi)
        b = lo;
    }
}

template <typename L>
__global__ __launch_bounds__(256) void kz_cc_hook_kernel(int* parent, const int64_t* __restrict__ ind, L rows, int64_t n_q, int64_t n_entries,
                                                         int64_t n_index) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += stride) {
        const int64_t t = ind[e];
        if (t < 0 || t >= n_index) continue;   // no pair
        kz_cc_link(parent, (int)kz_cc_row_of(rows, n_q, e), (int)(n_q + t));
    }
}

// The EDGE-ARRAY front end (kz_components_edges): edge e joins source row source[e] and target row target[e]; an edge with either id
// out of range is no pair (the rule above, for both ends: nothing vouches for the source ids of a free-standing edge array).
__global__ __launch_bounds__(256) void kz_cc_hook_edges_kernel(int* parent, const int64_t* __restrict__ source, const int64_t* __restrict__ target,
                                                               int64_t n_q, int64_t n_edges, int64_t n_index) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
        const int64_t i = source[e], t = target[e];
        if (i < 0 || i >= n_q || t < 0 || t >= n_index) continue;   // no pair
        kz_cc_link(parent, (int)i, (int)(n_q + t));
    }
}

// root[v] = the root above v.  Nothing writes parent in this launch: plain loads.  A walk goes to strictly smaller nodes: at most v
// steps (path halving has kept the trees shallow).
__global__ __launch_bounds__(256) void kz_cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ root, int n_nodes) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += stride) {
        int r = (int)v;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;
        root[v] = r;
    }
}

// The exclusive prefix of v over the workgroup's 256 threads and their total, to every thread (kz_pc_tile_scan's scheme, kz_pairs.hip:
// a shuffle scan per wave, the four wave totals through LDS; s_w is free again when the call returns).
__device__ __forceinline__ int kz_cc_tile_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return before + incl - v;
}

// scan, level 1: tile_sum[t] = the roots among nodes 256 t .. 256 t + 255
__global__ __launch_bounds__(256) void kz_cc_tile_sums_kernel(const int* __restrict__ root, int n_nodes, int* __restrict__ tile_sum) {
    __shared__ int s_w[4];
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int sum;
    (void)kz_cc_tile_scan(v < n_nodes && root[v] == (int)v ? 1 : 0, s_w, sum);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;
}

// scan, level 2 (ONE workgroup): tile_sum[t] <- the roots in front of tile t, 256 tiles a round with a running base; *n_components =
// the number of roots
__global__ __launch_bounds__(256) void kz_cc_tile_bases_kernel(int* __restrict__ tile_sum, int n_tiles, int64_t* __restrict__ n_components) {
    __shared__ int s_w[4];
    int base = 0;   // (uniform)
    for (int t0 = 0; t0 < n_tiles; t0 += 256) {   // (uniform)
        const int t = t0 + (int)threadIdx.x;
        int sum;
        const int before = kz_cc_tile_scan(t < n_tiles ? tile_sum[t] : 0, s_w, sum);
        if (t < n_tiles) tile_sum[t] = base + before;
        base += sum;
    }
    if (threadIdx.x == 0) *n_components = base;
}

// scan, level 3: rank[v] = the roots in front of node v (read at the roots only)
__global__ __launch_bounds__(256) void kz_cc_ranks_kernel(const int* __restrict__ root, int n_nodes, const int* __restrict__ tile_base,
                                                          int* __restrict__ rank) {
    __shared__ int s_w[4];
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int sum;
    const int before = kz_cc_tile_scan(v < n_nodes && root[v] == (int)v ? 1 : 0, s_w, sum);
    if (v < n_nodes) rank[v] = tile_base[blockIdx.x] + before;
}

// the first *n_components entries of both size arrays <- 0 (the count lies on the device: no second synchronise)
__global__ __launch_bounds__(256) void kz_cc_zero_sizes_kernel(const int64_t* __restrict__ n_components, int64_t* __restrict__ size_q,
                                                               int64_t* __restrict__ size_t_) {
    const int64_t n = *n_components, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += stride) {
        size_q[c] = 0;
        size_t_[c] = 0;
    }
}

// label[v] = rank[root[v]], split into the two outputs; with sizes: one add per DISTINCT label of a wave and side.  A giant component
// would send every add of the chip to one address: the lanes that hold the label of the first lane still waiting are counted with
// two ballots and that lane adds the counts; the loop runs over the distinct labels of the wave, at most 64 times.  (The grid
// covers the nodes in whole waves: every lane of a wave runs every round of the loop.)
__global__ __launch_bounds__(256) void kz_cc_labels_kernel(const int* __restrict__ root, const int* __restrict__ rank, int n_nodes, int n_q,
                                                           int64_t* __restrict__ label_q, int64_t* __restrict__ label_t,
                                                           unsigned long long* __restrict__ size_q, unsigned long long* __restrict__ size_t_) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_round = ((int64_t)n_nodes + 63) / 64 * 64;   // (whole waves)
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_round; v += stride) {
        const bool live = v < n_nodes, is_q = v < n_q;
        int label = -1;
        if (live) {
            label = rank[root[v]];
            if (is_q)
                label_q[v] = label;
            else
                label_t[v - n_q] = label;
        }
        if (!size_q) continue;   // (uniform)
        bool waiting = live;
        for (unsigned long long todo = __ballot(waiting); todo != 0; todo = __ballot(waiting)) {   // (wave-uniform)
            const int first = __ffsll((long long)todo) - 1;
            const int l0 = __shfl(label, first, 64);
            const bool mine = waiting && label == l0;
            const int cnt_q = __popcll(__ballot(mine && is_q)), cnt_t = __popcll(__ballot(mine && !is_q));
            if (lane == first) {
                if (cnt_q) atomicAdd(size_q + l0, (unsigned long long)cnt_q);
                if (cnt_t) atomicAdd(size_t_ + l0, (unsigned long long)cnt_t);
            }
            waiting = waiting && !mine;
        }
    }
}

// the checks both layouts share beyond kz_csr_require's, all before anything is launched
int kz_cc_require(const char* who, int64_t n_q, int64_t n_index, const int64_t* d_label_q, const int64_t* d_label_t, const int64_t* d_size_q,
                  const int64_t* d_size_t, const int64_t* h_n_components) {
    if (n_q + n_index >= 0x7fffffffLL) {
        kz_set_error("%s: n_q + n_index = %lld nodes, the limit is 2^31 - 2 (node ids are int32)", who, (long long)(n_q + n_index));
        return KZ_ERR_UNSUPPORTED;
    }
    KZ_REQUIRE(h_n_components && d_label_t && (n_q == 0 || d_label_q), "%s: null argument", who);
    KZ_REQUIRE((d_size_q == nullptr) == (d_size_t == nullptr), "%s: d_size_q and d_size_t are both null or both given", who);
    return KZ_OK;
}

// `hook(parent)` queues the front end's hook launch (none when there is no entry): the one stage that reads the pairs
template <typename H>
int kz_components_impl(kz_ctx* ctx, H&& hook, int64_t n_q, int64_t n_index, int64_t* d_label_q, int64_t* d_label_t, int64_t* d_size_q,
                       int64_t* d_size_t, int64_t* h_n_components) {
    const int n_nodes = (int)(n_q + n_index), n_tiles = (int)((n_q + n_index + 255) / 256);
    // (released when the function returns, behind its synchronise)
    KzPoolBuf<int> parent, root, rank, tile;
    KzPoolBuf<int64_t> count;
    int rc = parent.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = root.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = rank.alloc(ctx, (size_t)n_nodes * 4);
    if (rc == KZ_OK) rc = tile.alloc(ctx, (size_t)n_tiles * 4);
    if (rc == KZ_OK) rc = count.alloc(ctx, 16);
    if (rc != KZ_OK) return rc;
    const dim3 nodes(kz_blocks(n_nodes, 4096)), wg(256);
    hipLaunchKernelGGL(kz_cc_init_kernel, nodes, wg, 0, ctx->stream, parent.get(), n_nodes);
    hook(parent.get());
    hipLaunchKernelGGL(kz_cc_flatten_kernel, nodes, wg, 0, ctx->stream, (const int*)parent.get(), root.get(), n_nodes);
    hipLaunchKernelGGL(kz_cc_tile_sums_kernel, dim3(n_tiles), wg, 0, ctx->stream, (const int*)root.get(), n_nodes, tile.get());
    hipLaunchKernelGGL(kz_cc_tile_bases_kernel, dim3(1), wg, 0, ctx->stream, tile.get(), n_tiles, count.get());
    hipLaunchKernelGGL(kz_cc_ranks_kernel, dim3(n_tiles), wg, 0, ctx->stream, (const int*)root.get(), n_nodes, (const int*)tile.get(), rank.get());
    if (d_size_q)
        hipLaunchKernelGGL(kz_cc_zero_sizes_kernel, nodes, wg, 0, ctx->stream, (const int64_t*)count.get(), d_size_q, d_size_t);
    hipLaunchKernelGGL(kz_cc_labels_kernel, nodes, wg, 0, ctx->stream, (const int*)root.get(), (const int*)rank.get(), n_nodes, (int)n_q, d_label_q,
                       d_label_t, reinterpret_cast<unsigned long long*>(d_size_q), reinterpret_cast<unsigned long long*>(d_size_t));
    KZ_HIP(hipGetLastError());
    KZ_HIP(hipMemcpyAsync(h_n_components, count.get(), sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipStreamSynchronize(ctx->stream));
    return KZ_OK;
}

// the hook launch of the two list layouts
template <typename L>
auto kz_cc_list_hook(kz_ctx* ctx, const int64_t* d_ind, L rows, int64_t n_q, int64_t n_entries, int64_t n_index) {
    return [=](int* parent) {
        if (n_entries > 0)
            hipLaunchKernelGGL((kz_cc_hook_kernel<L>), dim3(kz_blocks(n_entries, 4096)), dim3(256), 0, ctx->stream, parent, d_ind, rows, n_q,
                               n_entries, n_index);
    };
}

}  // namespace

extern "C" int kz_components_csr(kz_ctx* ctx, const int64_t* d_indptr, const int64_t* d_ind, int64_t n_q, int64_t nnz, int64_t n_index,
                                 int64_t* d_label_q, int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components) {
    const int rcq = kz_csr_require("kz_components_csr", ctx, n_q, nnz, n_index);
    if (rcq != KZ_OK) return rcq;
    const int rcc = kz_cc_require("kz_components_csr", n_q, n_index, d_label_q, d_label_t, d_size_q, d_size_t, h_n_components);
    if (rcc != KZ_OK) return rcc;
    KZ_REQUIRE(nnz == 0 || d_ind, "kz_components_csr: null argument");
    *h_n_components = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    const int rcv = kz_csr_validate("kz_components_csr", ctx, d_indptr, n_q, nnz);
    if (rcv != KZ_OK) return rcv;
    return kz_components_impl(ctx, kz_cc_list_hook(ctx, d_ind, KzRowsCsr{d_indptr}, n_q, nnz, n_index), n_q, n_index, d_label_q, d_label_t, d_size_q,
                              d_size_t, h_n_components);
}

extern "C" int kz_components_lists(kz_ctx* ctx, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, int64_t* d_label_q,
                                   int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components) {
    KZ_REQUIRE(ctx != nullptr, "kz_components_lists: null context");
    KZ_REQUIRE(k >= 1, "kz_components_lists: lists of at least one column, got k = %d", k);
    KZ_REQUIRE(n_q >= 0 && n_q < 0x7fffffffLL, "kz_components_lists: n_q = %lld is outside [0, 2^31 - 1)", (long long)n_q);
    KZ_REQUIRE(n_index >= 1 && n_index < 0x7fffffffLL, "kz_components_lists: n_index = %lld is outside [1, 2^31 - 1)", (long long)n_index);
    const int64_t n_entries = n_q * (int64_t)k;   // (< 2^62)
    if (n_entries >= 0x7fffffffLL) {
        kz_set_error("kz_components_lists: %lld list entries, the limit is 2^31 - 2", (long long)n_entries);
        return KZ_ERR_UNSUPPORTED;
    }
    const int rcc = kz_cc_require("kz_components_lists", n_q, n_index, d_label_q, d_label_t, d_size_q, d_size_t, h_n_components);
    if (rcc != KZ_OK) return rcc;
    KZ_REQUIRE(n_q == 0 || d_ind, "kz_components_lists: null argument");
    *h_n_components = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    return kz_components_impl(ctx, kz_cc_list_hook(ctx, d_ind, KzRowsFixed{k}, n_q, n_entries, n_index), n_q, n_index, d_label_q, d_label_t, d_size_q,
                              d_size_t, h_n_components);
}

// The same five stages behind an EDGE ARRAY (source[e], target[e]), e < count, in any order, edges repeated or not: what a cut of
// kz_forest_*'s forest is labelled with.  One thread per edge.
extern "C" int kz_components_edges(kz_ctx* ctx, const int64_t* d_source, const int64_t* d_target, int64_t count, int64_t n_q, int64_t n_index,
                                   int64_t* d_label_q, int64_t* d_label_t, int64_t* d_size_q, int64_t* d_size_t, int64_t* h_n_components) {
    const int rcq = kz_csr_require("kz_components_edges", ctx, n_q, count, n_index);   // (the limits of a CSR of `count` entries)
    if (rcq != KZ_OK) return rcq;
    const int rcc = kz_cc_require("kz_components_edges", n_q, n_index, d_label_q, d_label_t, d_size_q, d_size_t, h_n_components);
    if (rcc != KZ_OK) return rcc;
    KZ_REQUIRE(count == 0 || (d_source && d_target), "kz_components_edges: null argument");
    *h_n_components = 0;
    KZ_HIP(hipSetDevice(ctx->device));
    auto hook = [=](int* parent) {
        if (count > 0)
            hipLaunchKernelGGL(kz_cc_hook_edges_kernel, dim3(kz_blocks(count, 4096)), dim3(256), 0, ctx->stream, parent, d_source, d_target, n_q,
                               count, n_index);
    };
    return kz_components_impl(ctx, hook, n_q, n_index, d_label_q, d_label_t, d_size_q, d_size_t, h_n_components);
}
