// Host-only ROUTE decisions of a search (no HIP in this header, like kz_plan.h: tests/host/route_sanitize.cpp compiles it with
// g++ -fsanitize=address,undefined on the CPU).  kz_common.h includes it for the product.
//
// Where a route is DECIDED is here: plain numbers and flags in (KzRouteIn: copied once at the top of a call; KzResearch: what a
// re-search asks for), small structs out (KzRoute: the list geometry and tier a pass runs with; KzAfterPass: where its uncertified
// rows go).  Where it is EXECUTED is kz_knn.hip: whatever allocates or launches (kz_himage_dealt with its NOMEM fall-through,
// kz_himage_ensure, the probe's sub-searches) stays there, between the pure calls.
//
//   kz_route_lists          -- list length / long-k geometry / exact-only of a call, and what a re-search raises
//   kz_route_tier           -- operand tier of the call
//   kz_route_short_geometry -- short-list route of the ordinary kernel: lists of 16 over P ranges of the dealt image?
//   kz_route_wide_geometry  -- wide route: many lists of 16?
//   kz_route_take_dealt     -- the ONE place a route of lists of 16 on the dealt image is taken
//   kz_route_to_long        -- the ONE way back to the one long list per query
//   kz_probe_wanted / kz_probe_verdict / kz_probe_wide_wins / kz_route_start_hard -- the tier probe's gate and verdicts
//   kz_route_sub_pieces     -- index ranges per query tile of one launch
//   kz_after_pass           -- where the rows a pass could not certify go: never what this pass just tried
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KZ_ROUTE_HD __host__ __device__ __forceinline__
#else
#define KZ_ROUTE_HD static inline
#endif

enum { KZ_TIER_F32 = 0, KZ_TIER_BF = 1, KZ_TIER_H = 2 };

// ---- constants the decisions read (each defined here, once) ---------------------------------------------------------------------
constexpr int KZ_K_DUAL_SHORT_DIV = 5;   // short-list routes: one list of 16 per this many neighbours (k / 5 lists)
constexpr double KZ_K_PROBE_MIN_MS = 12.0;   // searches below "probe_min_pairs" distance pairs take neither the tier probe nor a floor -- unless the sweep is at least this many model-ms (2 n_q n_i d / 1e12) long
constexpr int KZ_K_EXACT_DIRECT_ROWS = 32;   // at most this many rows left by the split-bf16 tier skip the float32-operand kernel and go to the exact kernels
constexpr int KZ_FIN_MAXM = 4096;  // list entries per query: 4 waves x (4096*8 + 128*28) B = 142 KiB of LDS at most
// Rows a K' = 16 pass could not certify: few (the usual handful) -> more lists of 16, it is all latency; many (hard data) -> lists
// of 64, which certify more of them in one go (400k x 400k, k = 10, clusters of very different density: 140 against 112 ms)
constexpr int KZ_ESC_SHORT_MAX_ROWS = 2048;
constexpr int KZ_MAX_PIECES = 128;  // index ranges per query tile (each range keeps its own K'-entry list per query).  Round 4: 64 -> 128
                                    // (a search of 8 .. 700 rows against 1 M: 0.84 .. 0.92 -> 0.61 .. 0.74 ms; 256: the finalize kernel's selection eats the gain)
constexpr int KZ_RANGE_MIN_ROWS = 128;      // fewer rows: the whole-index kernels (a sweep for a handful of rows costs more than it saves)
constexpr int KZ_RG_MIN_ROWS = 2048;   // failed rows from which representatives are tried
constexpr int KZ_EXACT_MAX_K = 4096;

// Per-wave LDS of the finalize kernel for a launch whose queries hold at most max_m list entries.
KZ_ROUTE_HD int kz_fin_wave_bytes(int max_m, int KP) {
    return ((max_m * 8 + KP * 28) + 15) & ~15;
}
constexpr int KZ_FIN_LDS_BYTES = 160 * 1024;   // of a CU: four waves' worth of kz_fin_wave_bytes must fit

// Slices (16 features) of the fp16 image of a matrix with kg k-groups: d_pad / 16 -- rounded up to a multiple of 8 beyond 32
// slices (the wide-row builds of the fp16 kernel, kz_knn_h_inst.h, exist for 32, 40, 48, 56 and 64 slices only; the padding
// slices are zero, and zero products add exactly nothing to the float32 accumulators) and to a multiple of 16 beyond 64 (the
// parity-split builds, kz_knn_hx16.h: 80, 96, 112 and 128 slices -- each wave pair splits them into two of the counts above).
KZ_ROUTE_HD int kz_h_nsr(int kg) {
    const int s = kg / 4;
    return s <= 32 ? s : (s <= 64 ? (s + 7) & ~7 : (s + 15) & ~15);
}
// The fp16 tier exists for 2 .. 24 slices (d <= 384) and 32 .. 128 slices (d = 497 .. 2048: the wide-row builds up to 64 slices,
// the parity-split builds beyond); 25 .. 31 slices and more than 128 run on float32 operands.
KZ_ROUTE_HD bool kz_h_slices_ok(int kg) {
    const int s = kg / 4;
    return (s >= 2 && s <= 24) || (s >= 32 && s <= 128);
}

static inline int kz_pick_list_len(int k_eff) {
    if (k_eff <= 12) return 16;
    if (k_eff <= 26) return 32;
    if (k_eff <= 54) return 64;
    if (k_eff <= 110) return 128;
    return 0;
}

// What a re-search asks of kz_knn_impl (the default asks for nothing: the context's settings).  The caller decides the fields together.
struct KzResearch {
    int prec = -1;            // operands: -1 = the context's setting (kz_ctx::precision), else 0 / 1 / 2
    int min_kp = 0;           // smallest list length, 16 .. 128 (escalated rows of the fp16 tier: longer lists on the same operand images)
    bool more_lists = false;  // escalated rows of a K' = 16 pass: more lists of 16 instead of longer ones (min_kp 0)
    int wide_lists = 0;       // > 0: the fp16 tier's WIDE route with this many lists of 16 per query (min_kp 0)
    bool no_short = false;    // not the short-list route (rows that route could not certify: a re-search differs from the pass that failed)
};
static inline KzResearch kz_research_wide(int lists) {   // (a caller's probe has found that this data needs margin in ranks, not better operands)
    KzResearch r;
    r.prec = 0;
    r.wide_lists = lists;
    return r;
}
static inline bool kz_research_is_default(const KzResearch& rs) {   // (a top-level call's)
    return rs.prec < 0 && rs.min_kp == 0 && !rs.more_lists && rs.wide_lists == 0;
}

// What the decisions read, copied once at the top of the call.
struct KzRouteIn {
    // the matrices
    int64_t n_tiles = 0;      // index tiles
    int64_t n = 0;            // index rows
    int kg = 0;               // k-groups of the index (d_pad / 4)
    int n_slices = 0;         // kz_h_nsr(kg)
    bool gemm_form = true;    // the metric has an inner-product form (everything below KZ_MANHATTAN)
    bool same_kg = true;      // query->kg == index->kg
    bool range_ok = false;    // the range re-search applies to this pair (kz_range.h: kz_range_shapes_ok -- dtype, d, alignment, options)
    // the call
    int k_eff = 0;
    bool dual = false;        // a pass of kz_knn_dual
    // the context's options
    int precision = 0, esc_bf = 1, short_ord = 1, short_ord_min_tiles = 48, wide_lists = 32, wide_sel = 256, tier_probe = 1024, chunk_rows = 0;
    double probe_min_pairs = 5e10;
    // KzDualPass
    int short_pieces = 0, short_ksel = 0, short_kp = 0;
    bool dual_probed = false;
};

struct KzLists {
    int KP = 0;       // entries of a list, 16 / 32 / 64 / 128
    int KSEL = 0;     // > 0: the finalize kernel selects this many entries of a query's lists
    int pieces = 0;   // > 0: exactly this many index ranges (lists) per query tile
};
// The list geometry and tier a pass runs with.  Nothing outside this header assigns the lists or short_ord.
struct KzRoute {
    KzLists cur;              // this pass
    KzLists lng;              // the one long list per query: what the call would use without a route of lists of 16 (kz_route_to_long)
    int KP_class = 0;         // list length of k's class, before any route (128 on the long-k route; 0: exact-only)
    int tier = KZ_TIER_F32;
    bool exact_only = false;  // the call runs entirely on the exact float64 kernels
    bool short_ord = false;   // lists of 16 over ranges of the row-dealt image
    bool wide_route = false;
    int route_P = 0;          // ranges the short-list route dealt the index over (kz_himage_dealt)
    int min_pieces_call = 0;
};
static inline bool kz_route_same_lists(const KzLists& a, const KzLists& b) { return a.KP == b.KP && a.KSEL == b.KSEL && a.pieces == b.pieces; }

// (split-bf16 operands exist: d = 497 .. 2048, 32 .. 128 slices: the fp16 tier's wide-row and parity-split builds -- and no split-bf16 tier: precision = 2 runs on float32
//  operands there, and so does every row the fp16 pass leaves that would have gone to the split-bf16 operands: esc_bf)
static inline bool kz_route_bf_ok(const KzRouteIn& in) { return in.n_slices >= 2 && in.n_slices <= 24 && in.same_kg; }
static inline bool kz_route_esc_bf(const KzRouteIn& in) { return in.esc_bf && kz_route_bf_ok(in); }

// More than 110 neighbours per query: no fused kernel keeps a list that long -- but the kernels keep ONE list per query and
// index RANGE, and the finalize kernel merges them.  LONG-k ROUTE (111 .. ~540 neighbours): lists of 128 over S >= k / 24
// index ranges (a range then holds ~24 of a query's k nearest rows on average; a range that holds more than its list does is
// seen by the certification -- kz_finalize_query: piece_bound -- and the row goes down the tiers), from which the finalize
// kernel selects and re-ranks KSEL = k + max(16, k / 8) candidates.  Beyond that (or an index too short to cut into S
// ranges of >= 4 tiles) the call runs entirely on the exact float64 kernels (k selection rounds over the full distance row
// per query: correct for any k <= n, and slow -- the reference's scikit-learn path has no such limit either,
// sklearn_nearest_neighbors.py:51-65; INTEGRATION.md "Deviations").
// The Minkowski family beyond p = 2 (KZ_MANHATTAN, KZ_CHEBYSHEV, KZ_MINKOWSKI) has no inner-product form: no MFMA kernel, the
// call runs entirely on the exact float64 kernels (scikit-learn's own generic DatasetsPair path is the slow one there too).
// Returns false when k is beyond what the exact kernels take (KZ_EXACT_MAX_K): the call is refused.
static inline bool kz_route_lists(const KzRouteIn& in, const KzResearch& rs, KzRoute* out) {
    KzRoute r;
    const int k_eff = in.k_eff;
    int KP = in.gemm_form ? kz_pick_list_len(k_eff) : 0;
    int KSEL = 0, long_pieces = 0;
    if (KP == 0 && !in.dual && in.gemm_form) {
        const int S = k_eff / 24 + 1 > 4 ? k_eff / 24 + 1 : 4;
        const int sel = k_eff + (k_eff / 8 > 16 ? k_eff / 8 : 16);
        // (finalize: 4 waves x (S 128 entries x 8 B + KSEL x 28 B) of LDS per workgroup)
        // (float32-operand tier: two lane-half lists per range, hence at most 8 ranges = 16 lists, see kz_prepare_pass)
        if (S <= KZ_FIN_MAXM / 128 && 4 * kz_fin_wave_bytes(S * 128, sel) <= KZ_FIN_LDS_BYTES &&
            4 * kz_fin_wave_bytes((S < 8 ? S : 8) * 256, sel) <= KZ_FIN_LDS_BYTES && in.n_tiles >= (int64_t)4 * S) {
            KP = 128;
            KSEL = sel;
            long_pieces = S;
        }
    }
    // SHORT-LIST ROUTE of the dual pass (13 .. 110 neighbours): the same construction the other way round -- lists
    // of 16 over k / 5 index ranges instead of one list of 32 / 64 / 128 per query.  The K' = 16 kernel keeps three workgroups per CU
    // and its merges short; a range that holds 16 or more of a query's nearest rows is seen by the certification (piece_bound).
    // The caller has dealt the index tiles over the ranges (kz_knn_dual.h): near rows of a query sit in ALL ranges alike.
    r.KP_class = KP;
    if (in.dual && in.short_pieces > 0 && KP > in.short_kp && rs.min_kp <= in.short_kp) {
        KP = in.short_kp;
        KSEL = in.short_ksel;
        long_pieces = in.short_pieces;
    }
    r.exact_only = KP == 0;
    if (r.exact_only) {
        if (k_eff > KZ_EXACT_MAX_K) return false;
        KP = 128;   // (list geometry of the scratch block only; no list kernel runs)
    }
    if (KP < rs.min_kp) KP = rs.min_kp < 128 ? rs.min_kp : 128;   // (list lengths are 16 / 32 / 64 / 128)
    // rs.more_lists (escalated rows of a K' = 16 pass): MORE LISTS instead of longer ones -- a list of 16 per index range over at
    // least four ranges, the finalize kernel selecting k + 16 of their entries.  The bound of the certification becomes the
    // largest 16th-best key of a RANGE (a quarter of the index or less) instead of the 16th-best key of the whole index: the
    // margin in ranks a failed row needs, with the K' = 16 kernel and a quarter of the entries to merge (14 rows of a 1M-row
    // index: 0.75 + 0.62 ms with lists of 64 over 64 ranges).
    if (rs.more_lists) {
        if (KP == 16 && !r.exact_only && KSEL == 0 && in.n_tiles >= 16) {
            KSEL = k_eff + 48;   // (<= 60 of the >= 64 entries)
            r.min_pieces_call = 4;
        } else if (!r.exact_only && KP < 64) {
            KP = 64;   // (an index of a few tiles: lists of 64 -- every re-search must ask for MORE than the pass that failed)
        }
    }
    r.cur.KP = KP;
    r.cur.KSEL = KSEL;
    r.cur.pieces = long_pieces;
    r.lng = r.cur;   // (the list geometry this call would use without the route)
    *out = r;
    return true;
}

// ---- tier of this call ----------------------------------------------------------------------------------------------------------
static inline void kz_route_tier(const KzRouteIn& in, const KzResearch& rs, KzRoute* r) {
    const int precision = rs.prec >= 0 ? rs.prec : in.precision;
    int tier = KZ_TIER_F32;
    if (precision != 1 && kz_h_slices_ok(in.kg) && in.same_kg) {
        if (precision != 2) tier = KZ_TIER_H;
        else if (kz_route_bf_ok(in)) tier = KZ_TIER_BF;
    }
    if (r->exact_only) tier = KZ_TIER_F32;   // (nothing is packed or launched for it)
    r->tier = tier;
}

// SHORT-LIST ROUTE of the ordinary kernel: as in the dual pass, lists of 16 over P index ranges instead of one list of 32 /
// 64 / 128 per query -- on a second image of the index whose ROWS are dealt over the ranges (kz_himage_dealt; in the caller's
// row order the near rows of a query may all sit in one stretch).  P lists hold at least as many entries as the list they
// replace; taken when a range has at least 48 tiles (measured down to 49: k = 100 on 125k index rows 15.3 -> 8.2 ms, k = 50 on
// 83k rows 11.3 -> 9.6, k = 26 on 60k rows 6.9 -> 6.5).  (The long lists' kernels stay for small indexes.)
// True: the route applies with *P_out ranges, the finalize kernel selecting *sel_out entries (the caller deals the image, then
// kz_route_take_dealt).
static inline bool kz_route_short_geometry(const KzRouteIn& in, const KzResearch& rs, const KzRoute& r, int* P_out, int* sel_out) {
    const int k_eff = in.k_eff, KP = r.cur.KP, KSEL = r.cur.KSEL;
    // (the long-k route up to 320 neighbours as well: k / 5 <= 64 lists of 16 instead of 4 .. 14 lists of 128 -- 50k x 500k x 200, main
    //  kernel: k = 128 32.4 -> 12.5 ms, k = 160 35.4 -> 13.3; beyond 32 lists the finalize kernel selects by repeated arg-max)
    const bool longk_lists = KSEL > 0 && r.cur.pieces > 0 && KP == 128 && rs.min_kp == 0 && k_eff <= 320;
    if (in.dual || rs.no_short || r.tier != KZ_TIER_H || !in.short_ord || KP <= 16 || !(KSEL == 0 || longk_lists) || r.exact_only) return false;
    int P = (k_eff + KZ_K_DUAL_SHORT_DIV - 1) / KZ_K_DUAL_SHORT_DIV;
    if (P < KP / 16) P = KP / 16;
    if (rs.min_kp >= 128) P = 16;   // (a re-search that asks for lists of 128: all the ranges the finalize kernel's fast selection takes)
    const int sel = k_eff + (KP >= 128 ? 80 : 48) < P * 16 ? k_eff + (KP >= 128 ? 80 : 48) : P * 16;
    *P_out = P;
    *sel_out = sel;
    // (the finalize kernel selects by rank counting, kz_rank_select<1>, up to 64 entries and by radix select beyond -- held in registers up
    //  to 512 entries in the build for many candidates, read from LDS up to the 1024 of the long-k route's 33 .. 64 lists)
    return P <= (longk_lists ? 64 : 32) && in.n_tiles >= (int64_t)in.short_ord_min_tiles * P && sel >= k_eff &&
           4 * kz_fin_wave_bytes(P * 16, sel) <= KZ_FIN_LDS_BYTES;
}

// WIDE ROUTE (round 5): many lists of 16 -- "wide_lists" (32) of them over as many ranges of the row-dealt image, the finalize
// kernel selecting "wide_sel" (256) of their entries.  For data whose keys are DENSE around the k-th neighbour (tight clusters:
// hundreds of rows of a cluster lie within the rounding bound of the k-th key).  What such a row needs to be certified is margin
// in RANKS -- the bound on the rows outside the candidate set must fall 2 eps below the k-th key, i.e. the set must reach down
// to the ~250th key -- and that costs list events and re-ranked rows, not MFMA products: the fp16 kernel with one product per
// multiply-add stays, where the split-bf16 tier pays three (bench.py "hard": every row failed the fp16 pass with lists worth
// ~100 ranks; with 256 they are certified).  Taken when the tier probe says so or a caller asks for it (rs.wide_lists).
static inline bool kz_route_wide_geometry(const KzRouteIn& in, const KzRoute& r, int P, int* sel_out) {
    const int k_eff = in.k_eff;
    int sel = in.wide_sel < P * 16 ? in.wide_sel : P * 16;
    if (sel < k_eff + 16) sel = k_eff + 16 < P * 16 ? k_eff + 16 : P * 16;
    *sel_out = sel;
    return !in.dual && r.tier == KZ_TIER_H && !r.exact_only && r.lng.KP <= 128 && r.lng.KSEL == 0 && P >= 2 && P <= 32 && P * 16 > r.lng.KP &&
           sel >= k_eff && in.n_tiles >= (int64_t)8 * P && 4 * kz_fin_wave_bytes(P * 16, sel) <= KZ_FIN_LDS_BYTES;
}

// The index has been dealt over P ranges (kz_himage_dealt): P lists of 16 per query, `sel` of their entries selected.
static inline void kz_route_take_dealt(KzRoute* r, int P, int sel, bool wide) {
    r->short_ord = true;
    r->cur.KP = 16;
    r->cur.KSEL = sel;
    r->cur.pieces = P;
    if (wide) r->wide_route = true;
    else r->route_P = P;
}
// Back to the one long list per query (the other tiers' kernels keep one list of K' per query).
static inline void kz_route_to_long(KzRoute* r) {
    r->short_ord = false;
    r->cur = r->lng;
}
// The rest of the call runs at `tier` (kz_after_pass: tier_next).
static inline void kz_route_next_tier(KzRoute* r, int tier) {
    if (tier != r->tier && r->short_ord) kz_route_to_long(r);
    r->tier = tier;
}

// TIER PROBE.  Data that is hard for fp16 as a whole (tight clusters far from the centre: nearly every row fails the first pass'
// certification) used to pay for a complete fp16 sweep and its finalize before anything went down the tiers (bench.py "hard":
// 2 x 31.6 of 150 ms per step).  A large ordinary search therefore first sends a STRIDED sample of its query rows (1024 rows since the end of round 4, 4096 before:
// representative whatever the row order) through the fp16 pass as an escalation-style sub-search; if more than half of them
// cannot be certified, the call starts at the split-bf16 tier.  The sample's results are written to their places (the main
// pass writes the same values again).  Cost on data that is fine: ~0.35 % of a 300k-row sweep + ~0.3 ms (230k x 230k x 128: 13.5 -> 13.2 ms
// with 1024 instead of 4096 rows; 200k x 400k x 200, cosine, k = 50: 32.4 -> 31.8); only top-level searches of >= 5e10 distance pairs
// and >= 16 probe sizes of query rows take it (C1 / C2 do not).  Option "tier_probe" = 0: off.
static inline bool kz_probe_wanted(const KzRouteIn& in, const KzResearch& rs, const KzRoute& r, int64_t q_count) {
    return r.tier == KZ_TIER_H && !in.dual && kz_research_is_default(rs) && !r.exact_only && in.tier_probe > 0 && in.esc_bf &&
           q_count >= (int64_t)16 * in.tier_probe && in.chunk_rows == 0 &&
           ((double)q_count * (double)in.n >= in.probe_min_pairs ||
            2.0 * (double)q_count * (double)in.n * (double)(in.kg * 4) / 1e12 >= KZ_K_PROBE_MIN_MS);
}
struct KzProbeVerdict {
    bool hard;       // more than half of the probe uncertified: the call starts at the next tier
    bool try_wide;   // more than an eighth: the probe rows again through the wide route first
};
// (the verdict counts the rows that left the probe's FIRST pass uncertified, once each -- not the cumulative count of the
//  levels below it, which counted a row that went two levels down twice)
static inline KzProbeVerdict kz_probe_verdict(int n_probe, int64_t n_first_fail, int wide_lists) {
    KzProbeVerdict v;
    v.hard = n_first_fail * 2 > n_probe;
    // LADDER: before better operands, more margin in ranks on the SAME operands -- the probe rows again through the wide
    // route.  Tried from an eighth of the probe uncertified on: re-searching a quarter of the rows one by one costs more
    // than the sweep itself (300 k x 300 k x 96, clusters of very different spread, k = 10: 24 % of the rows re-searched,
    // 24 ms of sweep in a 93 ms call).  Taken when at most a quarter of the probe stays uncertified there AND that is less
    // than half of what the ordinary lists left.
    v.try_wide = n_first_fail * 8 > n_probe && wide_lists >= 2;
    return v;
}
static inline bool kz_probe_wide_wins(int n_probe, int64_t n_first_fail, int64_t n_wide_fail) {
    return n_wide_fail * 4 <= n_probe && n_wide_fail * 2 < n_first_fail;
}
// A hard verdict: the call starts at the split-bf16 tier (wide rows: no split-bf16 operands, the float32 ones).
static inline void kz_route_start_hard(const KzRouteIn& in, KzRoute* r) {
    r->tier = kz_route_bf_ok(in) ? KZ_TIER_BF : KZ_TIER_F32;
    // (data this hard for fp16 is hard for the split-bf16 operands, too, wherever the keys are dense: lists of 64 from the
    //  start -- 300k x 300k x 96, k = 10, clusters of very different spread: rows searched again 135 k -> 51 k, call 170 -> 110 ms)
    if (r->cur.KSEL == 0 && r->cur.KP < 64) r->cur.KP = 64;
    if (r->short_ord) kz_route_to_long(r);   // (the other tiers' kernels keep one list of K' per query)
}

// Index ranges per query tile one launch is forced to (0: the planner's choice).  units: work items of the launch's query tiles,
// slots: work items a round of the kernel holds, n_ytiles: index tiles of the pass.
static inline int kz_route_sub_pieces(const KzRoute& r, int units, int slots, int n_ytiles) {
    // (long-k route: exactly `pieces` index ranges per query tile, one round)
    int force_pieces = (r.tier == KZ_TIER_F32 && r.cur.pieces > 8) ? 8 : r.cur.pieces;
    if (r.tier == KZ_TIER_H && r.short_ord && force_pieces > 0) {
        // a SMALL launch on the short-list route (a re-search of a few hundred uncertified rows, a probe): P ranges per query
        // tile leave most of the chip idle (216 rows x 10 ranges: 20 workgroups sweeping 390 tiles each, 1.98 ms) -- every
        // range is cut further, s P lists of 16 per query (the finalize kernel selects from any number of lists), as long as
        // a piece keeps at least 8 tiles and a query at most KZ_MAX_PIECES (128) lists
        int sub = slots / (units * force_pieces);
        if (sub > KZ_MAX_PIECES / force_pieces) sub = KZ_MAX_PIECES / force_pieces;
        if (sub > n_ytiles / (8 * force_pieces)) sub = n_ytiles / (8 * force_pieces);
        if (sub > 1 && 4 * kz_fin_wave_bytes(force_pieces * sub * 16, r.cur.KSEL) <= KZ_FIN_LDS_BYTES) force_pieces *= sub;
    }
    return force_pieces;
}

// Where the rows a pass could not certify go.
struct KzAfterPass {
    int tier_next;        // tier of the REST of the call
    bool range_direct;    // a few hundred to a few thousand rows of a split-bf16 pass: the range re-search, then the exact kernels
    bool exact_direct;    // the exact kernels at once (a handful of rows of a split-bf16 pass, or range_direct)
    bool rescued;         // the speculative launches behind the finalize kernel have answered them all
    bool escalate;        // searched again as a dense block (`next`); else: the exact kernels (unless rescued)
    bool early_range;     // ... after the grouped range re-search has tried them (kz_range.h "grouped")
    bool ladder;          // ... through kz_escalate_ladder: the wide route on a sample of them first
    bool range_first;     // exact path: behind the range re-search
    KzResearch next;      // what the re-search asks for: (operand tier, list length) -- never what this pass just tried
};
static inline KzAfterPass kz_after_pass(const KzRouteIn& in, const KzResearch& rs, const KzRoute& r, bool probed, int n_fail, int64_t cq_count,
                                        int spec_R) {
    KzAfterPass a;
    const int tier = r.tier, KP = r.cur.KP, KSEL = r.cur.KSEL, long_pieces = r.cur.pieces;
    const bool esc_bf = kz_route_esc_bf(in);
    // More than a quarter of the chunk's rows uncertified: this data needs better operands -- the REST of the call starts at
    // the next tier (not in the dual pass: its kernel exists for the fp16 tier only).  THIS chunk's uncertified rows go down
    // like any others: searching a quarter (or all) of the rows again at the next tier is never more work than redoing the
    // whole chunk there, which is what an earlier version did -- and abandoned the shared sweep altogether (500k x 62.5k, k = 50, 40
    // tight clusters: 579 -> 540 ms cluster by cluster, 528 -> 348 ms shuffled; nearly every row of that set needs better operands).
    a.tier_next = tier;
    if (!in.dual && tier != KZ_TIER_F32 && (int64_t)n_fail * 4 > cq_count)
        a.tier_next = (tier == KZ_TIER_H && esc_bf && long_pieces == 0) ? KZ_TIER_BF : KZ_TIER_F32;
    // A HANDFUL of rows left by the split-bf16 operands skips the float32-operand kernel: that kernel sweeps the whole index for
    // one query tile in at most eight pieces -- 2.2 ms on 300 k rows of d = 64 whatever the row count -- while the exact kernels
    // cost ~35 us a row there (both scale with n d): bench.py "hard", ~20 rows per direction and step: 60.6 -> see r05_notes.
    // (... and so do a few hundred to a few thousand rows where the range re-search applies and the index is large: that kernel's
    //  sweep of the whole index per launch -- 3 ms on 200 k x 200 -- against one fp16 sweep of the failed rows and their pairs;
    //  the tier probe's 1 024 rows paid 2 x 3 ms there on hard data)
    a.range_direct = tier == KZ_TIER_BF && !in.dual && !r.exact_only && n_fail >= KZ_RANGE_MIN_ROWS && n_fail < KZ_RG_MIN_ROWS &&
                     in.n >= 65536 && in.range_ok;
    a.exact_direct = (tier == KZ_TIER_BF && !in.dual && n_fail > 0 && n_fail <= KZ_K_EXACT_DIRECT_ROWS) || a.range_direct;
    // (the speculative launches behind the finalize kernel have answered them all)
    a.rescued = spec_R > 0 && n_fail > 0 && n_fail <= spec_R;
    a.escalate = tier != KZ_TIER_F32 && n_fail > 0 && !a.exact_direct && !a.rescued;
    a.range_first = !r.exact_only && n_fail >= KZ_RANGE_MIN_ROWS && in.range_ok;
    a.early_range = false;
    a.ladder = false;
    if (!a.escalate) return a;
    // Escalate only the uncertified rows: gather them into a dense query block and search it again -- fp16 tier
    // with lists shorter than 128: same operands, lists four times as long (no new image of the index: 14 rows
    // of a 1M-row index cost 0.4 ms this way against 7 ms for packing its float32 image); otherwise the split-bf16
    // operands (from the fp16 tier), then the float32-operand kernel.  The inner call sends its own uncertified rows further down (float32 operands,
    // exact float64 kernels).  Results are scattered back.
    // (more than half of the chunk uncertified: the fp16 operands are the wrong tool for this data, longer lists of the
    //  same keys will not help most of them -- straight to the split-bf16 operands)
    // (... and so are the rows the WIDE route leaves: it already is the fp16 tier's largest margin in ranks)
    const bool fp16_hard = tier == KZ_TIER_H && in.esc_bf &&
                           (r.wide_route || ((int64_t)n_fail * 2 > cq_count && (long_pieces == 0 || r.short_ord || (in.dual && in.short_pieces > 0))));
    const bool widen = tier == KZ_TIER_H && KP < 128 && !fp16_hard;
    // (short-list route: the rows it cannot certify are mostly the ones a list of K' could not certify either -- they go
    //  where that list's failures would have gone, lists four times K', not through a list of K' first)
    const int KP_esc = r.short_ord ? r.lng.KP : (r.KP_class > KP ? r.KP_class : KP);
    // (... when they are many: lists of 128 -- which the callee turns into 16 lists of 16 on the dealt image when the index
    //  is large: more ranges than this pass had, so not the same search again.  A handful -- uniform data: ~2e-4 of the
    //  queries, those whose near rows crowd one range -- is certified by ONE list of K' at a quarter of the cost: 500k x
    //  500k, k = 50: 4.7 -> 1.7 ms per step)
    const bool crowding_only = KP_esc > KP && n_fail <= KZ_ESC_SHORT_MAX_ROWS;
    KzResearch next;
    if (!widen) {   // fp16 with its longest lists, or fp16 altogether, has failed: better operands, this call's own list length
        next.prec = (tier == KZ_TIER_H && esc_bf && (long_pieces == 0 || fp16_hard)) ? 2 : 1;
        // (the float32 operands are the LAST approximate tier and their a-priori bound is the loosest: with this call's own
        //  list length -- 16 for k = 10 -- the K'-th key lies a handful of keys below the k-th and inside the bound wherever
        //  the keys are dense; lists of 64 certify such rows instead of handing them to the exact kernels at ~60 us a row:
        //  300k x 300k x 96, clusters of very different spread: 9 968 rows to the exact kernels and 726 ms per call before, none and
        //  169 ms now; lists of 128 for every call: bench.py "hard", k = 50, 118 -> 225 ms -- its lists of 64 were long enough)
        next.min_kp = ((next.prec == 1 || r.wide_route) && r.KP_class < 64) ? 64 : 0;
    } else if (KP == 16 && KSEL == 0 && n_fail <= KZ_ESC_SHORT_MAX_ROWS) {
        next.prec = 0;
        next.more_lists = true;   // a handful of rows of a K' = 16 pass: more lists of 16
    } else {
        next.prec = 0;
        next.min_kp = crowding_only ? KP_esc : (KP_esc * 4 < 128 ? KP_esc * 4 : 128);
        // (after a short-list pass: one LONG list -- unless many rows failed and the callee can still add ranges)
        next.no_short = KP_esc > KP && (crowding_only || long_pieces >= 16);
    }
    a.next = next;
    // EARLY RANGE RE-SEARCH (kz_range.h "grouped"): thousands of rows the split-bf16 operands could not certify are, on data
    // with clusters far tighter than its extent, rows the float32 operands cannot certify either -- they used to cost a sweep
    // of the whole index there (85 of 180 ms per direction, 200 k x 200 k x 200) before the exact kernels got them.  The
    // groups are tried before the re-search: rows that share a representative's range are answered by the exact kernels at once;
    // the others go on to the next tier as before.
    // (NOT on what an fp16 pass leaves: rows that only lack margin in ranks -- 40 tight clusters, 100 k x 101 k x 128 -- are
    //  cheaper on the ladder's wide route than as 2.4e8 exact pairs: 26.5 -> 33.7 ms with the groups tried there, removed)
    a.early_range = tier == KZ_TIER_BF && !in.dual && n_fail >= KZ_RG_MIN_ROWS && in.range_ok;
    // (fp16 found hard after the fact, no probe beforehand: the ladder on the failed rows -- top-level calls only)
    a.ladder = fp16_hard && !r.wide_route && next.prec == 2 && !probed && kz_research_is_default(rs) && !(in.dual && in.dual_probed);
    return a;
}
