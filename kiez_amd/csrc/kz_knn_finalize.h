// Stage 2 of kz_knn (kz_knn.hip): the finalize kernels -- merge a query's candidate lists, certify them, re-rank in float64 -- and
// their launcher.  Included by kz_knn.hip behind the first-pass kernels; kz_knn_fin_wide.h holds the build for many candidates.
#pragma once

// ---------------------------------------------------------------------------------------------------
// Stage 2: merge + certify + float64 re-rank
// ---------------------------------------------------------------------------------------------------

struct KnnFinParams {
    const float* in_key;  // [rows][M]
    const int* in_idx;
    KzListLayout lay;     // list layout (kz_list_base)
    int max_m;            // largest entry count of a query in this launch (sizes the dynamic LDS)
    int fast_div;         // cosine re-rank: y_k / |y| as kz_div_shared (one reciprocal per candidate row; same bits as the division)
    int64_t q_first, q_last;  // local query range [q_first, q_last) handled by this launch
    int KP;               // entries per list (per query and index range)
    int KSEL;             // candidates the finalize kernel selects from a query's lists and re-ranks (0: = KP).  Larger than KP on the
                          // long-k route (more than 110 neighbours: lists of 128 over many index ranges, kz_knn_impl)
    int64_t list_row0;    // list row of local query 0  (= q_begin - qt0*128)
    int64_t q_begin;      // global query row of local query 0
    int64_t q_count;
    const void* qraw;     // raw query rows (global row indexing)
    const void* yraw;     // raw index rows
    const double* ynorm64; // cosine, float32 rows: the index rows normalised in float64 (kz_matrix_norm64), or NULL
    const double* qsqn;
    const double* ysqn;
    int64_t n_i;
    int d;
    int metric;
    int k;                // neighbours to return
    int exclude_self;
    const int64_t* self_ids;  // optional: index row to strip per local query (escalated subsets); NULL = q_begin + q
    double gamma;         // rounding-bound factor (already multiplied by eps_scale)
    const double* ystats; // index matrix: [0] max row norm (device)
    // fp16 first pass (kz_knn_h16.h): keys are in centred, scaled units; the bound uses the measured operand residuals
    int tier_h;
    double eps_mult;      // eps_scale (test knob)
    double gamma_acc;     // float32 accumulation part of the bound
    const double* q_rowq; // query image: [n][3] = |x_c|^2, |x_h|, |x_c - x_h|
    const double* y_hmax; // index image: max |y_h|, max |y_c - y_h|, max |y_c|^2
    const double* hscale; // {S, 1 / S^2}
    // dual pass, reverse direction (kz_knn_dual.h): the list holds the K' best EVENTS of the row; rows outside the events
    // have an approximate key below excl_floor[q] (+inf: the row's events are incomplete, it must fail)
    const float* excl_floor;
    // seeded lists (KnnCandParams::qfloor): [q_begin + q] the key the query's lists started from -- rows that never entered a list
    // have an approximate key at or below it
    const float* list_floor;
    int dual_col;
    const int* idx_map;   // dual pass, forward direction: list entry r stands for index row idx_map[r] (NULL: identity)
    const int* row_map;   // dual pass, forward direction: the query image is permuted too -- image row r is matrix row row_map[r];
                          // raw row, norms, residuals, the output position and the fail-list entry all go by the MATRIX row
    double* out_dist;     // [q_count][k]
    int64_t* out_ind;
    int* fail_count;
    int* fail_list;
    double* fail_tau;     // optional, beside fail_list: the exact value of the row's k-th best CANDIDATE (+inf: fewer than k candidates) -- an
                          // upper bound of its k-th neighbour's value whatever the tier: what the range re-search starts from (kz_range.h)
    unsigned long long* err_ratio_bits;  // max over certified candidates of |key~ - key| / eps (bits of a non-negative double)
};

// (kz_exact_value: kz_common.h -- shared with kz_pair_values, which must reproduce the re-rank's values bit for bit)
template <typename T>
__device__ __forceinline__ double kz_output_distance(double v, int metric, double p = 2.0) {
    // (Minkowski family: the ranking value is the reduced distance; scikit-learn converts at the end,
    //  MinkowskiDistance._rdist_to_dist: rdist ** (1 / p), rounded to the input dtype -- measured on scikit-learn 1.7.2)
    if (metric == KZ_MINKOWSKI) return kz_f32_rows<T> ? (double)(float)pow(v, 1.0 / p) : pow(v, 1.0 / p);
    // (seuclidean: SEuclideanDistance._rdist_to_dist, sqrt of the ranking value -- already rounded to the input dtype -- rounded
    //  again; correlation: the constant row's NaN, ranked as +inf (kz_family_finish), is NaN again)
    if (metric == KZ_SEUCLIDEAN) return kz_f32_rows<T> ? (double)(float)sqrt(v) : sqrt(v);
    if ((metric == KZ_CORRELATION || metric == KZ_DICE || metric == KZ_SOKALSNEATH) && v == INFINITY) return NAN;   // (dice, sokalsneath: kz_bool.h)
    if (metric == KZ_EUCLIDEAN) {
        // ArgKmin32 converts the surrogate with the float32 metric object: (double)sqrtf((float)d2)
        // (_argkmin.pyx.tp:285-295 with INPUT_DTYPE_t = float32); ArgKmin64 uses sqrt in float64.
        // exactly what sklearn executes: float32 argument, double sqrt, result rounded back to float32
        if (kz_f32_rows<T>) return (double)(float)sqrt((double)(float)v);
        return sqrt(v);
    }
    return v;
}

// Writes the final k entries of one query from its (value, idx)-sorted prefix.  sorted arrays live in LDS.
// sklearn self removal (neighbors/_base.py:947-965): among the first k+1, drop the entry whose index is the
// query row; if it is absent drop the first one.
template <typename T>
__device__ __forceinline__ void kz_emit_sorted(const double* sval, const int* sidx, int n_sorted, int k, int exclude_self,
                                               int64_t self_row, int metric, double* od, int64_t* oi, int lane, double p = 2.0) {
    int self_rank = -1;
    if (exclude_self) {
        self_rank = 0;
        const int lim = min(n_sorted, k + 1);
        for (int c = 0; c < lim; ++c)
            if ((int64_t)sidx[c] == self_row) {
                self_rank = c;
                break;
            }
    }
    for (int c = lane; c < n_sorted; c += 64) {
        if (c == self_rank) continue;
        const int o = (self_rank >= 0 && c > self_rank) ? c - 1 : c;
        if (o < k) {
            od[o] = kz_output_distance<T>(sval[c], metric, p);
            oi[o] = (int64_t)sidx[c];
        }
    }
}

// Gather parallelism of the finalize kernel: candidate rows per group (KZ_FIN_ROWS), groups in flight per wave (KZ_FIN_DEPTH:
// 2 = one group ahead, 3 = two) and the occupancy the kernel is compiled for (KZ_FIN_WAVES).  Round 3, same box, average
// launch on ns / C3 (tools/job_fin.sh): rows 4 depth 2 at 4 waves per SIMD (round 2's build, 112 VGPRs) 4.06 / 8.47 ms; rows 2
// depth 3 at 5 waves (4 spilled) 3.57 / 7.60; rows 1 depth 2 at 7 waves (70 VGPRs, no spill) 3.03 / 7.37; rows 1 depth 3 at 7
// (6 spilled) 3.14 / 7.25; rows 4 depth 3 at 3 waves 4.96 / 9.59.  Waves in flight beat rows in flight per wave: the phases
// around the gather loop (list load, rank select, rank sort) of one query hide under the gathers of the other waves' queries.
// Round 4 (the loads of the loop issued without branches, so that the prefetch overlaps at all; the per-query values in scalar
// registers: 71 -> 59 VGPRs), finalize time over 4 steps of C3 + 4 of ns, reverse chain not overlapped: rows 1 depth 2 at 8 waves
// 69.2 ms; rows 2 depth 2 at 7 (70 VGPRs) 69.1; rows 1 depth 3 at 7 69.5; **rows 1 depth 3 at 8 (64 VGPRs, no spill) 67.4**; rows 2
// depth 3 at 6 72.9.  Round 5: the selection paths added since (unsorted path, radix selections) brought the 8-wave build to 8
// spilled VGPRs; 7 waves (72 VGPRs, none spilled), same box, two runs each: ns 98.14 / 98.04 -> 97.56 / 97.16 ms per step, C3
// 122.43 / 122.34 -> 122.19 / 121.87.
#ifndef KZ_FIN_ROWS_N
#define KZ_FIN_ROWS_N 1
#endif
#ifndef KZ_FIN_DEPTH
#define KZ_FIN_DEPTH 3
#endif
constexpr int KZ_FIN_ROWS = KZ_FIN_ROWS_N;
// (KZ_FIN_MAXM, kz_fin_wave_bytes: kz_route.h)
// (the finalize kernel for many candidates shares bytes between arrays that are never live together: kz_knn_fin_wide.h)
__host__ __device__ __forceinline__ int kz_fin_wide_wave_bytes(int max_m, int KS) {
    return ((max_m * 8 + KS * 20) + 15) & ~15;
}

// k-th largest (rank = 1: the largest) of n float keys held as SORTABLE unsigned patterns in LDS; returns the pattern.
// Wave-cooperative: 32 counting passes at most, fewer below the common prefix of the patterns.  The entries are read ONCE into
// registers (E per lane, n <= 64 E): a counting pass is then E compares and E ballots, no LDS round trip in the dependent chain
// bit -> count -> next bit (round 5: the finalize kernel for many candidates runs three such selections per query at three waves
// per SIMD -- the chains, not the instruction count, were what it waited for).
// Largest "smallest key of a FULL list" over a query's lists of KP = 16 or 32 entries, the entries held E per lane (entry e = lane +
// 64 i): a list's entries sit in KP consecutive lanes of one i, so every list is reduced inside its lane group -- all lists of an
// i at once, no loop over the lists (32 lists: 8 x 4 shuffle steps instead of 32 dependent rounds of 5).  -inf: no full list.
template <int E>
__device__ __forceinline__ float kz_full_lists_bound(const float (&key)[E], const bool (&ok)[E], int M, int KP, int lane) {
    float bound = -INFINITY;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        if (64 * i >= M) break;   // (uniform)
        int c = ok[i] ? 1 : 0;
        float mn = ok[i] ? key[i] : INFINITY;
        for (int off = KP >> 1; off >= 1; off >>= 1) {   // (uniform trip count: 4 or 5)
            c += __shfl_xor(c, off, 64);
            mn = fminf(mn, __shfl_xor(mn, off, 64));
        }
        if (c == KP && lane + 64 * i < M) bound = fmaxf(bound, mn);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bound = fmaxf(bound, __shfl_xor(bound, off, 64));
    return bound;
}

// (core: the lane's E patterns in registers; pattern 0 = no entry)
template <int E>
__device__ __forceinline__ unsigned kz_radix_kth_u32_regs(const unsigned (&x)[E], unsigned all_or, unsigned all_and, int rank) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const unsigned differ = all_or ^ all_and;
    const int top = differ ? 31 - __clz(differ) : -1;
    unsigned thr = top >= 31 ? 0u : (top < 0 ? all_and : (all_and & ~((2u << top) - 1u)));
    for (int bit = top; bit >= 0; --bit) {
        const unsigned cand = thr | (1u << bit);
        int c = 0;
#pragma unroll
        for (int i = 0; i < E; ++i) c += (int)__popcll(__ballot(x[i] >= cand));
        if (c >= rank) thr = cand;
    }
    return thr;
}
template <int E>
__device__ __forceinline__ unsigned kz_radix_kth_u32_e(const unsigned* u, int n, int rank, int lane) {
    unsigned x[E];
    unsigned all_or = 0u, all_and = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = lane + 64 * i;
        const bool in = e < n;
        x[i] = in ? u[e] : 0u;   // (pattern 0 is below every candidate threshold, which has at least one bit set)
        all_or |= x[i];
        all_and &= in ? x[i] : 0xffffffffu;
    }
    return kz_radix_kth_u32_regs<E>(x, all_or, all_and, rank);
}
// (the generic finalize kernel is compiled for 64 VGPRs: it keeps the LDS loops)
template <bool REGS = false>
__device__ __forceinline__ unsigned kz_radix_kth_u32(const unsigned* u, int n, int rank, int lane) {
    if (REGS && n <= 256) return kz_radix_kth_u32_e<4>(u, n, rank, lane);
    if (REGS && n <= 512) return kz_radix_kth_u32_e<8>(u, n, rank, lane);
    unsigned all_or = 0u, all_and = 0xffffffffu;
    for (int e = lane; e < n; e += 64) {
        all_or |= u[e];
        all_and &= u[e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const unsigned differ = all_or ^ all_and;
    const int top = differ ? 31 - __clz(differ) : -1;
    unsigned thr = top >= 31 ? 0u : (top < 0 ? all_and : (all_and & ~((2u << top) - 1u)));
    for (int bit = top; bit >= 0; --bit) {
        const unsigned cand = thr | (1u << bit);
        int c = 0;
        for (int e0 = 0; e0 < n; e0 += 64) c += (int)__popcll(__ballot(e0 + lane < n && u[e0 + lane] >= cand));
        if (c >= rank) thr = cand;
    }
    return thr;
}
// rank-th SMALLEST (rank = 1: the smallest) of n non-negative doubles in LDS (their bit patterns order like the values).
template <int E>
__device__ __forceinline__ unsigned long long kz_radix_kth_small_f64_e(const double* v, int n, int rank, int lane) {
    unsigned long long x[E];
    unsigned long long all_or = 0ull, all_and = ~0ull;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = lane + 64 * i;
        const bool in = e < n;
        x[i] = in ? (unsigned long long)__double_as_longlong(v[e]) : ~0ull;   // (the largest pattern: never BELOW a candidate)
        all_or |= in ? x[i] : 0ull;
        all_and &= x[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const unsigned long long differ = all_or ^ all_and;
    const int top = differ ? 63 - __clzll(differ) : -1;
    unsigned long long thr = top >= 63 ? 0ull : (top < 0 ? all_and : (all_and & ~((2ull << top) - 1ull)));
    for (int bit = top; bit >= 0; --bit) {
        const unsigned long long cand = thr | (1ull << bit);
        int c = 0;   // entries below cand
#pragma unroll
        for (int i = 0; i < E; ++i) c += (int)__popcll(__ballot(x[i] < cand));
        if (c < rank) thr = cand;
    }
    return thr;
}
template <bool REGS = false>
__device__ __forceinline__ unsigned long long kz_radix_kth_small_f64(const double* v, int n, int rank, int lane) {
    if (REGS && n <= 256) return kz_radix_kth_small_f64_e<4>(v, n, rank, lane);
    unsigned long long all_or = 0ull, all_and = ~0ull;
    for (int e = lane; e < n; e += 64) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v[e]);
        all_or |= b;
        all_and &= b;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const unsigned long long differ = all_or ^ all_and;
    const int top = differ ? 63 - __clzll(differ) : -1;
    // thr = the smallest value with at least `rank` entries <= it: build the largest prefix p such that fewer than `rank` entries are
    // BELOW p, bit by bit from the top
    unsigned long long thr = top >= 63 ? 0ull : (top < 0 ? all_and : (all_and & ~((2ull << top) - 1ull)));
    for (int bit = top; bit >= 0; --bit) {
        const unsigned long long cand = thr | (1ull << bit);
        int c = 0;   // entries below cand
        for (int e0 = 0; e0 < n; e0 += 64)
            c += (int)__popcll(__ballot(e0 + lane < n && (unsigned long long)__double_as_longlong(v[e0 + lane]) < cand));
        if (c < rank) thr = cand;
    }
    return thr;
}

// Rank-based selection of the KP best of M <= 64*E list entries (key descending, row ascending; entries with row < 0 are
// empty).  Lane l holds entries l, l+64, ...; returns the number of entries written to ck/ci (ordered by rank).
template <int E>
__device__ __forceinline__ int kz_rank_select(const float* ekey, const int* eidx, int M, int KP, float* ck, int* ci, int lane) {
    float x[E];
    int xi[E], rank[E];
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const int e = lane + 64 * u;
        x[u] = e < M ? ekey[e] : -INFINITY;
        xi[u] = e < M ? eidx[e] : -1;
        rank[u] = 0;
    }
    int n_valid = 0;
#pragma unroll
    for (int v = 0; v < E; ++v) {
        n_valid += __popcll(__ballot(xi[v] >= 0));
        const int lim = min(64, M - 64 * v);
        for (int jj = 0; jj < lim; ++jj) {  // jj is wave-uniform: the broadcasts are v_readlane (spelled out: __shfl compiled to ds_bpermute)
            const int oi = __builtin_amdgcn_readlane(xi[v], jj);
            if (oi < 0) continue;   // (uniform)
            const float ox = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(x[v]), jj));
#pragma unroll
            for (int u = 0; u < E; ++u)
                if (64 * u < M) rank[u] += (ox > x[u] || (ox == x[u] && oi < xi[u])) ? 1 : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < E; ++u) {
        if (xi[u] >= 0 && rank[u] < KP) {
            ck[rank[u]] = x[u];
            ci[rank[u]] = xi[u];
        }
    }
    return n_valid < KP ? n_valid : KP;
}

// One query, one wave (only wave-level synchronisation inside).
// NV (round 6): 16-byte loads per lane and candidate row in the pipelined re-rank -- 1: float32 rows of up to 256 elements, 2: up to
// 512 (the second 256-element chunk's four fma continue the first chunk's chain: kz_wave_dot's order).  d = 300 -- the dimension
// of the entity-alignment embeddings kiez is used on, and of BASELINE configuration 4 -- used to take the generic loop below: no
// load in flight under the sums, the query row re-read per candidate (250 k x 1 M x 300: 7.3 ms per launch against 4.3 at d = 200).
template <typename T, int FROWS, int NV = 1>
__device__ __forceinline__ void kz_finalize_query(const KnnFinParams& p, const int64_t q, const int lane, char* wbase) {
    const int KS = p.KSEL > 0 ? p.KSEL : p.KP;   // candidates selected and re-ranked
    double* cv = reinterpret_cast<double*>(wbase);
    double* sv = cv + KS;
    float* ekey = reinterpret_cast<float*>(sv + KS);
    int* eidx = reinterpret_cast<int*>(ekey + p.max_m);
    float* ck = reinterpret_cast<float*>(eidx + p.max_m);
    int* ci = reinterpret_cast<int*>(ck + KS);
    int* si = ci + KS;
    const int KP = p.KP;
    const int k_eff = p.k + (p.exclude_self ? 1 : 0);
    // the query's own row and norm first: their latency passes under the list phase
    const int64_t qrow = p.row_map ? (int64_t)p.row_map[p.q_begin + q] : p.q_begin + q;
    const int64_t qout = p.row_map ? qrow : q;   // output row (row_map: out_dist / out_ind / fail_list are indexed by matrix rows)
    const T* qptr = reinterpret_cast<const T*>(p.qraw) + qrow * (int64_t)p.d;
    const double qs = p.qsqn[qrow];

    const int64_t lrow = p.list_row0 + q;
    const int n_pieces = p.lay.pieces[kz_list_region(lrow, p.lay)];
    const int halves = p.lay.halves;
    const int M = n_pieces * halves * KP;
    // entry e of this query: piece e / (halves KP), lane-half (e / KP) % halves, list entry e % KP  (kz_list_wave_base)
    if (p.lay.contig) {
        // fp16 kernel: the query's pieces x K' entries are one contiguous run
        const int64_t l0 = kz_list_contig_off(lrow, p.lay, KP, 0);
        for (int e = lane; e < M; e += 64) {
            ekey[e] = p.in_key[l0 + e];
            int r = p.in_idx[l0 + e];
            if (p.idx_map && r >= 0) r = p.idx_map[r];
            eidx[e] = r;
        }
    } else {
        const int64_t lwave = kz_list_wave_base(lrow, p.lay, KP, 0) + (lrow & 31);
        for (int e = lane; e < M; e += 64) {
            const int piece = e / (halves * KP);
            const int rem = e - piece * halves * KP;
            const int hh = rem / KP;
            const int ee = rem - hh * KP;
            const int64_t off = lwave + ((int64_t)piece * KP + ee) * KZ_LSTRIDE + hh * 32;
            ekey[e] = p.in_key[off];
            eidx[e] = p.in_idx[off];
        }
    }
    kz_wave_sync();

    // Long-k route (KS > KP): the union of the per-range lists holds the KS best approximate keys only if no range
    // contributes more than its list can hold.  A FULL list may have evicted rows: everything outside it has a key <= its
    // smallest entry -- the largest such value over the full lists joins the certification bound below.
    float piece_bound = p.list_floor ? p.list_floor[p.q_begin + q] : -INFINITY;
    if (KS > KP) {
        for (int l0 = 0; l0 < M; l0 += KP) {   // (uniform; KP is a multiple of 16, lists are at most 128 entries)
            float mn = INFINITY;
            int cnt = 0;
            for (int e = lane; e < KP; e += 64) {
                const bool ok = eidx[l0 + e] >= 0;
                cnt += ok ? 1 : 0;
                mn = ok ? fminf(mn, ekey[l0 + e]) : mn;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                cnt += __shfl_xor(cnt, off, 64);
                mn = fminf(mn, __shfl_xor(mn, off, 64));
            }
            if (cnt == KP) piece_bound = fmaxf(piece_bound, mn);
        }
    }
    // top-KS of the M entries by (key desc, idx asc).  Up to 64 entries: rank counting (ck / ci come out ordered).  More (round
    // 5): rank counting is O(M^2 / 64) per lane -- 160 entries (ten lists of 16): ~3 500 of a query's ~8 000 instructions -- and
    // NOTHING below needs the selected keys in order: the KS best by a radix select + compaction (unordered), further down the
    // k-th best of them by a second radix select and the candidates within 2 eps of it by compaction.
    int V = 0;
    bool unsorted = false;
    float sel_min = INFINITY, left_max = -INFINITY;   // unsorted path: smallest selected key; largest selected key NOT re-ranked
    if (M <= 64) {
        V = kz_rank_select<1>(ekey, eidx, M, KS, ck, ci, lane);
    } else {
        unsorted = true;
        unsigned* uk = reinterpret_cast<unsigned*>(ekey);   // (the keys are not needed as floats any more)
        auto key_of = [](unsigned u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu)); };
        int nv = 0;
        for (int e = lane; e < M; e += 64) {
            unsigned bts = __float_as_uint(ekey[e]);
            if (bts == 0x80000000u) bts = 0u;   // (-0 = +0)
            const bool valid = eidx[e] >= 0;
            uk[e] = valid ? (bts ^ ((bts >> 31) ? 0xffffffffu : 0x80000000u)) : 0u;
            nv += valid ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) nv += __shfl_xor(nv, off, 64);
        kz_wave_sync();
        const bool all = nv <= KS;
        unsigned thr = 0u;
        if (!all) thr = kz_radix_kth_u32(uk, M, KS, lane);   // (invalid entries carry the smallest pattern: they never reach rank KS)
        for (int e0 = 0; e0 < M; e0 += 64) {   // entries above the threshold (all valid entries when there are at most KS)
            const int e = e0 + lane;
            const bool sel = e < M && eidx[e] >= 0 && (all || uk[e] > thr);
            const unsigned long long mask = __ballot(sel);
            if (sel) {
                const int pos = V + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                const float kf = key_of(uk[e]);
                ck[pos] = kf;
                ci[pos] = eidx[e];
                sel_min = fminf(sel_min, kf);
            }
            V += (int)__popcll(mask);
        }
        if (!all) {   // the remaining places go to the entries AT the threshold with the smallest rows
            int last = -1;
            while (V < KS) {
                int best = 0x7fffffff;
                for (int e = lane; e < M; e += 64) {
                    const int xi = eidx[e];
                    if (xi >= 0 && uk[e] == thr && xi > last && xi < best) best = xi;
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
                if (best == 0x7fffffff) break;   // (cannot happen: at least KS entries are >= thr)
                if (lane == 0) {
                    ck[V] = key_of(thr);
                    ci[V] = best;
                }
                last = best;
                ++V;
                sel_min = fminf(sel_min, key_of(thr));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sel_min = fminf(sel_min, __shfl_xor(sel_min, off, 64));
    }
    kz_wave_sync();

    // Rounding bound of this query's approximate keys and the exact key of a candidate from its exact value.
    //   float32 / split-bf16 operands: |key~ - key| <= gamma (|y|max^2 / 2 + |q| |y|max), key = (|q|^2 - d^2) / 2 (euclidean
    //   family) or 1 - dist (cosine);
    //   fp16 operands (centred vectors x_c = float32(x - mu), operands x_h, residuals r = x_c - x_h measured at pack time):
    //   q_h.y_h - q_c.y_c = -(r_q.y_h + q_h.r_y + r_q.r_y), so by Cauchy-Schwarz on the ACTUAL residual norms
    //     |key~ - key_c| <= |r_q| Yh + |q_h| Ry + |r_q| Ry              (operand rounding; Yh = max |y_h|, Ry = max |r_y|)
    //                      + gamma_acc (Yc2 / 2 + |q_h| Yh)               (float32 accumulation of exact products + bias)
    //                      + 2^-23 (|q_c| + sqrt(Yc2))^2 + 1e-12 (...) + 1e-14 (|q|^2 + |y|max^2)
    //                                                                     (float32 centring round-off, float64 re-rank)
    //   with key_c = (|q_c|^2 - d^2) / 2 and d^2 = the exact squared distance (cosine: 2 dist, rows are unit vectors).
    double eps_q, key_scale = 1.0, qref = qs;
    const bool cosine_plain = p.metric == KZ_COSINE && !p.tier_h;
    if (p.tier_h) {
        const double qc2 = p.q_rowq[qrow * 3 + 0], qh = p.q_rowq[qrow * 3 + 1], qr = p.q_rowq[qrow * 3 + 2];
        const double Yh = p.y_hmax[0], Ry = p.y_hmax[1], Yc2 = p.y_hmax[2];
        const double qc = sqrt(qc2), yc = sqrt(Yc2);
        // (the float64 re-rank evaluates |q|^2 + |y|^2 - 2 q.y on the UNCENTRED rows: its own round-off scales with those)
        const double ymax = p.ystats[0];
        const double raw2 = p.metric == KZ_COSINE ? 2.0 : qs + ymax * ymax;
        eps_q = p.eps_mult * (qr * Yh + qh * Ry + qr * Ry + p.gamma_acc * (0.5 * Yc2 + qh * Yh) +
                              1.1920928955078125e-07 * (qc + yc) * (qc + yc) + 1e-12 * (0.5 * Yc2 + qc2) + 1e-14 * raw2);
        // reverse direction of a dual pass: the key was accumulated on top of THIS row's bias (|q_c|^2 / 2 joins the
        // accumulation term) and went through one more float32 rounding when it was filed as key' = acc - bias(t) + bias(q)
        if (p.dual_col) eps_q += p.eps_mult * (p.gamma_acc * 0.5 * qc2 + 1.1920928955078125e-07 * (0.5 * Yc2 + 0.5 * qc2 + qh * Yh));
        key_scale = p.hscale[1];
        qref = qc2;
    } else if (p.metric == KZ_COSINE) {
        eps_q = p.gamma * 1.001;
    } else {
        const double ymax = p.ystats[0];
        const double scale = 0.5 * ymax * ymax + sqrt(qs) * ymax;
        eps_q = p.gamma * scale;
        // the relative bound assumes the products stay in the normal float32 range (data at the 1e-19 scale and below
        // underflows in the matrix pipe): such rows are left to the exact float64 kernels
        if (scale < 1e-30) eps_q = INFINITY;
    }
    auto exact_key = [&](double v) {
        if (cosine_plain) return 1.0 - v;
        return 0.5 * (qref - (p.metric == KZ_COSINE ? 2.0 * v : v));
    };

    // Which candidates need an exact distance?  Those that can still be among the exact top-k: a candidate c with
    // key~_c < key~_(k) - 2 eps has key_c <= key~_c + eps < key~_(k) - eps <= (k-th best exact key of the re-ranked ones),
    // so it is out.  The list is ordered by approximate key: the re-rank covers a prefix of Vr >= k_eff candidates (K' = 64,
    // k = 50: ~52 gathered rows instead of 64).  The certification below re-checks the first pruned candidate.
    int Vr = V;
    if (unsorted) {
        if (V > k_eff && eps_q < INFINITY) {
            // the k-th best selected key (radix select over the sortable patterns, scratch: sv is written after the re-rank), then
            // the candidates within 2 eps of it to the front of ekey / eidx (the list copy is spent): the re-rank's set, unordered
            unsigned* su = reinterpret_cast<unsigned*>(sv);
            for (int c = lane; c < V; c += 64) {
                unsigned b = __float_as_uint(ck[c]);
                if (b == 0x80000000u) b = 0u;
                su[c] = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
            }
            kz_wave_sync();
            const unsigned uk_k = kz_radix_kth_u32(su, V, k_eff, lane);
            const float key_k = __uint_as_float(uk_k ^ ((uk_k >> 31) ? 0x80000000u : 0xffffffffu));
            const double thr = (double)key_k * key_scale - 2.0 * eps_q;
            int cnt = 0;
            for (int c0 = 0; c0 < V; c0 += 64) {
                const int c = c0 + lane;
                const bool in = c < V && (double)ck[c] * key_scale >= thr;
                const unsigned long long mask = __ballot(in);
                if (in) {
                    const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    ekey[pos] = ck[c];
                    eidx[pos] = ci[c];
                } else if (c < V) {
                    left_max = fmaxf(left_max, ck[c]);
                }
                cnt += (int)__popcll(mask);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) left_max = fmaxf(left_max, __shfl_xor(left_max, off, 64));
            Vr = cnt;       // (>= k_eff: the k_eff best keys are all >= key_k)
            ck = ekey;
            ci = eidx;
            kz_wave_sync();
        }
    } else if (V > k_eff && eps_q < INFINITY) {
        const double thr = (double)ck[k_eff - 1] * key_scale - 2.0 * eps_q;
        int cnt = 0;
        for (int c = lane; c < V; c += 64) cnt += ((double)ck[c] * key_scale >= thr) ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        Vr = cnt < k_eff ? k_eff : cnt;
    }

    // exact float64 re-rank of the Vr candidates, FROWS rows in flight per pass (independent gathers and butterfly sums
    // overlap); the per-candidate arithmetic is exactly kz_wave_dot / kz_wave_dot_normalized (kz_common.h)
    const T* yraw = reinterpret_cast<const T*>(p.yraw);
    const bool vec = kz_row_vec_ok(qptr, p.d) && kz_row_vec_ok(yraw, p.d);
#ifdef KZ_NO_FIN_PIPE
    if (false) {
#else
    if ((kz_f32_rows<T> || kz_half_rows<T>) && vec && p.d <= 256 * NV && Vr > 0) {
#endif   // (Vr == 0: a reverse-direction row without a single event)
        // float32 rows of up to 256 NV elements (NV 16-byte loads per lane and row) and float16 / bfloat16 rows of as many (8-byte
        // loads, widened in the reduce step as kz_row4 widens them; the generic loop below has no load in flight under the sums and
        // is a quarter slower on such rows, profiles/half_inputs.md): the loads of the NEXT group of FROWS
        // candidates are issued before the current group's fma chains and butterfly sums -- same arithmetic in the same order
        // as the generic loop below (and as kz_wave_dot), only the memory latency of group g+1 hides under the sums of group g
        const int k0 = 4 * lane;
        bool act[NV];
        int k0r[NV];
        double qk[4 * NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            act[c] = k0 + 256 * c < p.d;
            k0r[c] = act[c] ? k0 + 256 * c : 0;
            double t[4] = {0.0, 0.0, 0.0, 0.0};
            if (act[c]) {
                kz_row4(qptr, k0r[c], p.d, true, t);
                if (p.metric == KZ_COSINE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = t[e] / qs;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) qk[4 * c + e] = t[e];
        }
        using Frag = KzRowFrag<T>;
        auto issue = [&](int c0, Frag (&buf)[FROWS][NV], double (&ysb)[FROWS]) {
#pragma unroll
            for (int u = 0; u < FROWS; ++u) {
                // (no branch around a load, and no load under a condition: with loads on some paths only the compiler waits for
                //  ALL outstanding loads -- s_waitcnt vmcnt(0), the group just issued included -- before the first use of the
                //  current group, and the prefetch hides nothing (the loop ran at latency + arithmetic per candidate).  Lanes
                //  past the end of the row read its first elements and never use them; the group past the last one is the last
                //  candidate again.)
                const int yi = ci[min(c0 + u, Vr - 1)];
                ysb[u] = p.ysqn[yi];
#pragma unroll
                for (int c = 0; c < NV; ++c)
                    buf[u][c] = *reinterpret_cast<const Frag*>(yraw + (int64_t)yi * p.d + k0r[c]);
            }
        };
        auto reduce = [&](int c0, const Frag (&buf)[FROWS][NV], const double (&ysb)[FROWS]) {
#pragma unroll
            for (int u = 0; u < FROWS; ++u) {
                double a = 0.0;
                bool done = false;
                if (p.metric == KZ_COSINE && p.fast_div) {
                    const double rcp = 1.0 / ysb[u];   // (wave-uniform: every lane holds the same row norm)
                    const int rcp_hi = __builtin_amdgcn_readfirstlane((int)((unsigned long long)__double_as_longlong(rcp) >> 32));
                    if ((rcp_hi & 0x7ff00000) != 0x7ff00000) {
#pragma unroll
                        for (int c = 0; c < NV; ++c) {
                            double yk[4];
                            kz_frag4<T>(buf[u][c], yk);
                            if (act[c]) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) a = fma(qk[4 * c + e], kz_div_shared(yk[e], ysb[u], rcp), a);
                            }
                        }
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int c = 0; c < NV; ++c) {
                        double yk[4];
                        kz_frag4<T>(buf[u][c], yk);
                        if (act[c]) {
                            if (p.metric == KZ_COSINE) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) a = fma(qk[4 * c + e], yk[e] / ysb[u], a);
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) a = fma(qk[4 * c + e], yk[e], a);
                            }
                        }
                    }
                }
                const double dot = kz_wave_sum(a);
                double v;
                if (p.metric == KZ_COSINE) {
                    v = fmin(fmax(1.0 - dot, 0.0), 2.0);
                } else {
                    v = fmax((qs + ysb[u]) - 2.0 * dot, 0.0);
                }
                if (lane == 0 && c0 + u < Vr) cv[c0 + u] = v;
            }
        };
#if KZ_FIN_DEPTH == 3
        // three groups in flight (a rotating set of three register buffers, the loop unrolled by three: no copies): the gathers
        // of groups g + 1 and g + 2 are under way while group g is reduced
        constexpr int R = FROWS;
        Frag b0[R][NV], b1[R][NV], b2[R][NV];
        double y0[R], y1[R], y2[R];
        issue(0, b0, y0);
        issue(R, b1, y1);
        for (int c0 = 0;;) {   // (all conditions wave-uniform)
            issue(c0 + 2 * R, b2, y2);
            reduce(c0, b0, y0);
            if ((c0 += R) >= Vr) break;
            issue(c0 + 2 * R, b0, y0);
            reduce(c0, b1, y1);
            if ((c0 += R) >= Vr) break;
            issue(c0 + 2 * R, b1, y1);
            reduce(c0, b2, y2);
            if ((c0 += R) >= Vr) break;
        }
#else
        Frag cur[FROWS][NV], nxt[FROWS][NV];
        double ys_c[FROWS], ys_n[FROWS];
        issue(0, cur, ys_c);
        for (int c0 = 0; c0 < Vr; c0 += 2 * FROWS) {   // (unrolled by two: the buffers swap roles, no copies)
            issue(c0 + FROWS, nxt, ys_n);
            reduce(c0, cur, ys_c);
            if (c0 + FROWS >= Vr) break;
            issue(c0 + 2 * FROWS, cur, ys_c);
            reduce(c0 + FROWS, nxt, ys_n);
        }
#endif
    } else
    for (int c0 = 0; c0 < Vr; c0 += FROWS) {
        const T* yp[FROWS];
        double ys[FROWS], acc[FROWS];
#pragma unroll
        for (int u = 0; u < FROWS; ++u) {
            const int yi = ci[min(c0 + u, Vr - 1)];
            yp[u] = yraw + (int64_t)yi * p.d;
            ys[u] = p.ysqn[yi];
            acc[u] = 0.0;
        }
        for (int k0 = 4 * lane; k0 < p.d; k0 += 256) {
            double qk[4];
            kz_row4(qptr, k0, p.d, vec, qk);
            if (p.metric == KZ_COSINE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) qk[e] = qk[e] / qs;
            }
#pragma unroll
            for (int u = 0; u < FROWS; ++u) {
                double yk[4];
                kz_row4(yp[u], k0, p.d, vec, yk);
                if (p.metric == KZ_COSINE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[u] = fma(qk[e], yk[e] / ys[u], acc[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[u] = fma(qk[e], yk[e], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FROWS; ++u) {
            const double dot = kz_wave_sum(acc[u]);
            double v;
            if (p.metric == KZ_COSINE) {
                v = fmin(fmax(1.0 - dot, 0.0), 2.0);  // sklearn cosine_distances: S *= -1; S += 1; clip(0, 2)
            } else {
                v = fmax((qs + ys[u]) - 2.0 * dot, 0.0);  // |x|^2 - 2 x.y + |y|^2, clamped (_argkmin.pyx.tp:494-502)
            }
            if (lane == 0 && c0 + u < Vr) cv[c0 + u] = v;
        }
    }
    kz_wave_sync();
    // rank by (value asc, idx asc) and scatter into sorted order
    for (int c = lane; c < Vr; c += 64) {
        const double v = cv[c];
        const int id = ci[c];
        int rank = 0;
        for (int o = 0; o < Vr; ++o) {
            const double ov = cv[o];
            const int oid = ci[o];
            rank += (ov < v || (ov == v && oid < id)) ? 1 : 0;
        }
        sv[rank] = v;
        si[rank] = id;
    }
    kz_wave_sync();

    // Self-check of the bound the certification rests on: for every candidate both the approximate key (ck, from the
    // fused kernel) and the exact key (from the float64 re-rank) are known here.
    bool bound_violated = false;
    if (eps_q > 0.0 && eps_q < INFINITY && p.err_ratio_bits) {
        double worst = 0.0;
        for (int c = lane; c < Vr; c += 64) {
            const double v = cv[c];
            if (v > 0.0)  // (a distance clamped at 0 no longer carries the exact key)
                worst = fmax(worst, fabs((double)ck[c] * key_scale - exact_key(v)) / eps_q);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off, 64));
        bound_violated = worst > 1.0;   // (wave-uniform after the butterfly) never expected: see the certification below
        if (lane == 0 && worst > 0.0) {
            // a million waves hit ONE address: read first -- an ordinary load (served by this XCD's L2; a stale value only costs
            // a redundant atomicMax), not an agent-scope atomic load that goes to the memory side every time -- and only the
            // (rare) new maxima pay for the atomic
            const unsigned long long bits = (unsigned long long)__double_as_longlong(worst);
            if (bits > *(const volatile unsigned long long*)p.err_ratio_bits) atomicMax(p.err_ratio_bits, bits);
        }
    }

    // Certification (DESIGN.md "Certified candidate sets").  |key~ - key| <= eps for every index row.  A row outside
    // the candidate set has key~ <= ck[KP-1] (the K'-th best approximate key), hence an exact key <= ck[KP-1] + eps.
    // The exact key of the k-th re-ranked candidate is known.  If it is strictly larger, no outside row can enter -- or
    // tie with -- the exact top-k.  V < KP means no list ever evicted anything: the set is complete.
    bool certified;
    if (p.excl_floor) {
        // dual pass: outside the list are events that lost the selection (key~ <= ck[KP-1], full lists only) and the rows
        // that never were events (key~ < floor)
        double bound = (double)p.excl_floor[qrow];
        if (V == KP) bound = fmax(bound, (double)(unsorted ? sel_min : ck[KP - 1]));
        certified = V >= k_eff && bound * key_scale + eps_q < exact_key(sv[k_eff - 1]);
    } else {
        // rows outside the selected set: behind the KS-th selected key (when the selection is full), or evicted from a full
        // list (long-k route: piece_bound; with KS = KP a full list implies a full selection whose KS-th key is at least as
        // large, so the first term alone is the round-1 rule).  Neither: no list ever evicted anything, the set is complete.
        float bound = piece_bound;
        if (V == KS) bound = fmaxf(bound, unsorted ? sel_min : ck[KS - 1]);
        if (bound == -INFINITY)
            certified = (V >= min((int64_t)k_eff, p.n_i));
        else
            certified = V >= k_eff && (double)bound * key_scale + eps_q < exact_key(sv[k_eff - 1]);
    }
    // ... and the candidates that were not re-ranked are out by the same argument (implied by how Vr was chosen; re-checked)
    if (Vr < V && !((double)(unsorted ? left_max : ck[Vr]) * key_scale + eps_q < exact_key(sv[k_eff - 1]))) certified = false;
    // An approximate key further than eps from its exact value contradicts the bound everything above rests on (a kernel
    // or hardware fault, not a property of the data): do not trust this row's candidate set, send it down a tier.
    if (bound_violated) certified = false;
    if (!certified) {
        if (lane == 0) {
            const int pos = atomicAdd(p.fail_count, 1);
            p.fail_list[pos] = (int)qout;
            if (p.fail_tau) p.fail_tau[pos] = Vr >= k_eff ? sv[k_eff - 1] : (double)INFINITY;
        }
        return;
    }
    kz_emit_sorted<T>(sv, si, Vr, p.k, p.exclude_self, p.self_ids ? p.self_ids[q] : qrow, p.metric,
                      p.out_dist + qout * (int64_t)p.k, p.out_ind + qout * (int64_t)p.k, lane);
}

// A workgroup finalizes KZ_FIN_QPB consecutive queries (wave w takes queries w, w+4, ...).  32 per workgroup (sharing the list
// cache lines of one wave-interleaved block) measured 2x SLOWER than 4: finalize is latency-bound and wants many workgroups.
constexpr int KZ_FIN_QPB = 4;
#ifndef KZ_FIN_WAVES_2
#define KZ_FIN_WAVES_2 5  // ... of the two-loads-per-row build (NV = 2: 24 more registers of gather buffers and query elements)
#endif
#ifndef KZ_FIN_WAVES
#define KZ_FIN_WAVES 7  // minimum waves per SIMD the finalize kernel is compiled for (see KZ_FIN_ROWS_N above)
#endif
// FROWS / MINW: candidate rows gathered per group and the occupancy compiled for.  <1, KZ_FIN_WAVES> is the kernel of every
// ordinary pass (a dozen to ~50 gathered rows per query: waves in flight beat rows in flight per wave); <8, 2> serves the long-k
// route (hundreds of gathered rows per query, one workgroup per CU for its LDS anyway: the gathers of a query were a chain of
// ~k / 2 round trips).
template <typename T, int FROWS, int MINW, int NV = 1>
__global__ __launch_bounds__(256, MINW) void kz_knn_finalize_kernel(KnnFinParams p) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    const int lane = threadIdx.x & 63;
    // (wave number in a scalar register: the query number, its matrix row and everything loaded per query -- norm, image statistics
    //  -- are then scalar loads issued at the top of the query, not vector loads of one address by 64 lanes)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* wbase = fsm + (size_t)wave * kz_fin_wave_bytes(p.max_m, p.KSEL > 0 ? p.KSEL : p.KP);
    for (int rep = 0; rep < KZ_FIN_QPB / 4; ++rep) {
        const int64_t q = p.q_first + (int64_t)blockIdx.x * KZ_FIN_QPB + rep * 4 + wave;
        if (q >= p.q_last) break;  // whole wave leaves; only wave-level sync inside
        kz_finalize_query<T, FROWS, NV>(p, q, lane, wbase);
        kz_wave_sync();
    }
}

#include "kz_knn_fin_wide.h"

// Which build of the finalize kernel a pass launches (KZ_FIN_BUILD_*, kiez_amd.h): decided once per pass, from the parameters alone.
static int kz_fin_build(const KnnFinParams& fp, int KP, int dtype) {
    const bool wide = (fp.KSEL > 0 ? fp.KSEL : KP) > 160;   // the long-k route
    // (many selected candidates + float32 rows on the fp16 tier, ordinary direction: kz_knn_fin_wide.h)
    const bool rows_vec = fp.d <= 256 && (fp.d & 3) == 0 && (((uintptr_t)fp.qraw | (uintptr_t)fp.yraw) & 15u) == 0;
    if (wide && dtype == KZ_F32 && fp.tier_h && !fp.excl_floor && rows_vec) return KZ_FIN_BUILD_WIDE;
    if (wide) return KZ_FIN_BUILD_MANY;
    // (float32 rows of 260 .. 512 elements, 16-byte aligned -- float16 / bfloat16 rows of as many, 8-byte aligned: the build whose
    //  pipelined re-rank takes two loads per lane and row)
    const bool two_chunks = (dtype == KZ_F32 || kz_dtype_is_half(dtype)) && fp.d > 256 && fp.d <= 512 && (fp.d & 3) == 0 &&
                            (((uintptr_t)fp.qraw | (uintptr_t)fp.yraw) & (dtype == KZ_F32 ? 15u : 7u)) == 0;
    return two_chunks ? KZ_FIN_BUILD_TWO_LOADS : KZ_FIN_BUILD_ORDINARY;
}

// The finalize launches of one pass: one per list region (the dynamic LDS follows the region's entry count: occupancy of
// the gather).  fp.q_first / q_last / max_m are filled here.
static int kz_launch_finalize(kz_ctx* ctx, KnnFinParams& fp, const KzListLayout& lay, int KP, int64_t q_count, int dtype) {
    // the launches of this pass: [first query, last query), entries per query
    struct Group { int64_t lo, hi; int max_m; } groups[KZ_MAX_REGIONS];
    int n_groups = 0;
    for (int rg = 0; rg < lay.n_regions; ++rg) {
        const int64_t lo = (int64_t)(rg > 0 ? lay.qt_end[rg - 1] : 0) * KZ_TILE - fp.list_row0;
        // (neighbouring regions with the same number of ranges -- forced ranges: all of them -- go out as ONE launch)
        while (rg + 1 < lay.n_regions && lay.pieces[rg + 1] == lay.pieces[rg]) ++rg;
        const int64_t hi = (int64_t)lay.qt_end[rg] * KZ_TILE - fp.list_row0;
        Group g = {lo < 0 ? 0 : lo, hi > q_count ? q_count : hi, lay.pieces[rg] * lay.halves * KP};
        if (g.hi > g.lo) groups[n_groups++] = g;
    }
    // The SMALL launches -- the last query tiles of a pass, swept in many short ranges so that they fill the chip: a few hundred
    // queries with hundreds of list entries each, all latency (100k x 100k: 117 us after the 284 us of the main launch) -- go to
    // the context's second stream and run BESIDE the large one (fork / join by events), unless that stream is busy with the
    // reverse chain of a shared sweep or is the stream this call runs on.
    const hipStream_t main_stream = ctx->stream;
    const bool fork = n_groups >= 2 && ctx->stream2 && ctx->stream2 != main_stream && !ctx->stream2_busy;
    int big = 0;
    for (int g = 1; g < n_groups; ++g)
        if (groups[g].hi - groups[g].lo > groups[big].hi - groups[big].lo) big = g;
    const int build = kz_fin_build(fp, KP, dtype);
    const bool wide2 = build == KZ_FIN_BUILD_WIDE, wide = wide2 || build == KZ_FIN_BUILD_MANY, two_chunks = build == KZ_FIN_BUILD_TWO_LOADS;
    const void* fk = nullptr;   // (the kernel of every launch of this pass: chosen -- and an element type refused -- before the fork)
    if (dtype != KZ_F32) {
        // (float64 rows: the generic re-rank loop, whose loads go through kz_row4; the 2-byte types: the pipelined re-rank on
        //  8-byte loads where the rows allow it -- the kernel decides, as for float32 -- else the generic loop too)
        const int rcd = kz_dispatch_rows(dtype, "kz_knn", [&](auto e) {
            using T = typename decltype(e)::type;
            if constexpr (kz_half_rows<T>) {
                if (two_chunks) {
                    fk = (const void*)kz_knn_finalize_kernel<T, KZ_FIN_ROWS, KZ_FIN_WAVES_2, 2>;
                    return (int)KZ_OK;
                }
            }
            fk = wide ? (const void*)kz_knn_finalize_kernel<T, 4, 2> : (const void*)kz_knn_finalize_kernel<T, KZ_FIN_ROWS, KZ_FIN_WAVES>;
            return (int)KZ_OK;
        });
        if (rcd != KZ_OK) return rcd;
    } else if (wide2)
        fk = (const void*)kz_knn_finalize_wide_kernel<float, 4>;
    else if (wide)
        fk = (const void*)kz_knn_finalize_kernel<float, 8, 2>;
    else if (two_chunks)
        fk = (const void*)kz_knn_finalize_kernel<float, KZ_FIN_ROWS, KZ_FIN_WAVES_2, 2>;
    else
        fk = (const void*)kz_knn_finalize_kernel<float, KZ_FIN_ROWS, KZ_FIN_WAVES>;
    if (fork) {
        KZ_HIP(hipEventRecord(ctx->ev[7], main_stream));
        KZ_HIP(hipStreamWaitEvent(ctx->stream2, ctx->ev[7], 0));
    }
    for (int pass = 0; pass < 2; ++pass) {   // (fork: the small launches first, on the second stream; then the large one)
        for (int g = 0; g < n_groups; ++g) {
            const bool side = fork && g != big;
            if (fork ? (side != (pass == 0)) : pass == 1) continue;
            const hipStream_t st = side ? ctx->stream2 : main_stream;
            fp.q_first = groups[g].lo;
            fp.q_last = groups[g].hi;
            fp.max_m = groups[g].max_m;
            fp.fast_div = ctx->fin_fast_div;
            const int fin_blocks = (int)((fp.q_last - fp.q_first + KZ_FIN_QPB - 1) / KZ_FIN_QPB);
            size_t fin_lds = (size_t)4 * kz_fin_wave_bytes(fp.max_m, fp.KSEL > 0 ? fp.KSEL : KP);
            if (wide2) fin_lds = (size_t)4 * kz_fin_wide_wave_bytes(fp.max_m, fp.KSEL);
            if (fin_lds > 65536) KZ_HIP(hipFuncSetAttribute(fk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_lds));
            void* args[] = {&fp};
            KZ_HIP(hipLaunchKernel(fk, dim3(fin_blocks), dim3(256), args, fin_lds, st));
        }
    }
    KZ_HIP(hipGetLastError());
    if (fork) {
        KZ_HIP(hipEventRecord(ctx->ev[11], ctx->stream2));
        KZ_HIP(hipStreamWaitEvent(main_stream, ctx->ev[11], 0));
    }
    return KZ_OK;
}
