// CPU-only check of the route decisions of a search (kiez_amd/csrc/kz_route.h), built with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// by tests/test_host_sanitize.py.
//   * Cases whose answer follows from the rules written down in kz_route.h and DESIGN.md 3.3 / 3.4: the expected numbers are
//     written out here from those rules, not computed by calling the header.
//   * Invariants over a few thousand random inputs (every metric class, tier and option combination, k_eff 1 .. 4200, 1 .. 2^20
//     index tiles): the selection fits the lists and the finalize kernel's LDS; kz_route_to_long undoes any sequence of takes;
//     the chain of re-searches (kz_after_pass's request fed back in, every row failing every time) ends at the float32 tier or the
//     exact kernels within a few steps and never runs the same (tier, lists) twice.
#include <cstdio>
#include <random>
#include <set>
#include <tuple>

#include "../../kiez_amd/csrc/kz_route.h"

static int fails = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++fails;                                         \
        }                                                    \
    } while (0)

static KzRouteIn base_in(int k_eff, int64_t n_tiles) {   // d = 64 (4 slices), euclidean, every option at its default
    KzRouteIn in;
    in.n_tiles = n_tiles;
    in.n = n_tiles * 128;
    in.kg = 16;
    in.n_slices = kz_h_nsr(in.kg);
    in.k_eff = k_eff;
    return in;
}
// lists per query the pass keeps at least (more_lists leaves the range count to the planner, from four on)
static int pieces_of(const KzRoute& r) { return r.cur.pieces > 0 ? r.cur.pieces : (r.min_pieces_call > 0 ? r.min_pieces_call : 1); }

static void documented_cases() {
    KzRoute r;
    KzResearch none;
    // k = 10 -> one list of 16
    CHECK(kz_route_lists(base_in(10, 1000), none, &r) && r.cur.KP == 16 && r.cur.KSEL == 0 && r.cur.pieces == 0 && !r.exact_only && r.KP_class == 16,
          "k = 10: KP %d KSEL %d pieces %d", r.cur.KP, r.cur.KSEL, r.cur.pieces);
    CHECK(kz_route_lists(base_in(12, 1000), none, &r) && r.cur.KP == 16, "k = 12");
    CHECK(kz_route_lists(base_in(13, 1000), none, &r) && r.cur.KP == 32, "k = 13");
    CHECK(kz_route_lists(base_in(110, 1000), none, &r) && r.cur.KP == 128 && r.cur.KSEL == 0, "k = 110");
    // long-k route, its first k_eff: S = max(4, 111 / 24 + 1) = 5 ranges, KSEL = 111 + max(16, 111 / 8) = 127
    CHECK(kz_route_lists(base_in(111, 20), none, &r) && r.cur.KP == 128 && r.cur.KSEL == 127 && r.cur.pieces == 5 && !r.exact_only && r.KP_class == 128,
          "k = 111: KP %d KSEL %d pieces %d", r.cur.KP, r.cur.KSEL, r.cur.pieces);
    // ... and k_eff = 300: S = 13, KSEL = 300 + 37
    CHECK(kz_route_lists(base_in(300, 52), none, &r) && r.cur.KP == 128 && r.cur.KSEL == 337 && r.cur.pieces == 13, "k = 300: KSEL %d pieces %d",
          r.cur.KSEL, r.cur.pieces);
    // an index of fewer than 4 S tiles: exact-only (the scratch geometry of lists of 128, nothing selected)
    CHECK(kz_route_lists(base_in(111, 19), none, &r) && r.exact_only && r.cur.KP == 128 && r.cur.KSEL == 0 && r.cur.pieces == 0, "k = 111 on 19 tiles");
    kz_route_tier(base_in(111, 19), none, &r);
    CHECK(r.tier == KZ_TIER_F32, "exact-only: nothing is packed");
    // no inner-product form: exact-only whatever k
    {
        KzRouteIn in = base_in(10, 1000);
        in.gemm_form = false;
        CHECK(kz_route_lists(in, none, &r) && r.exact_only, "manhattan");
    }
    // k_eff > KZ_EXACT_MAX_K (4096): refused; 4096 itself: the exact kernels
    CHECK(!kz_route_lists(base_in(4097, 1 << 20), none, &r), "k = 4097 accepted");
    CHECK(kz_route_lists(base_in(4096, 1 << 20), none, &r) && r.exact_only, "k = 4096 refused");
    // more_lists on a K' = 16 pass: KSEL = k_eff + 48 over at least 4 ranges from 16 tiles on, lists of 64 below
    {
        KzResearch more;
        more.prec = 0;
        more.more_lists = true;
        CHECK(kz_route_lists(base_in(10, 16), more, &r) && r.cur.KP == 16 && r.cur.KSEL == 58 && r.min_pieces_call == 4, "more lists: KSEL %d", r.cur.KSEL);
        CHECK(kz_route_lists(base_in(10, 15), more, &r) && r.cur.KP == 64 && r.cur.KSEL == 0 && r.min_pieces_call == 0, "more lists, 15 tiles: KP %d", r.cur.KP);
    }
    // short-list route: P = max(ceil(k_eff / 5), KP / 16) ranges with at least short_ord_min_tiles (48) tiles each
    {
        int P = 0, sel = 0;
        KzRouteIn in = base_in(30, 288);   // KP 64: P = max(6, 4) = 6, sel = min(30 + 48, 96) = 78
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(r.tier == KZ_TIER_H && kz_route_short_geometry(in, none, r, &P, &sel) && P == 6 && sel == 78, "k = 30: P %d sel %d", P, sel);
        in.n_tiles = 287;
        CHECK(!kz_route_short_geometry(in, none, r, &P, &sel), "k = 30 on 287 tiles");
        in = base_in(13, 1000);            // KP 32: P = max(3, 2) = 3, sel = min(13 + 48, 48) = 48
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(kz_route_short_geometry(in, none, r, &P, &sel) && P == 3 && sel == 48, "k = 13: P %d sel %d", P, sel);
        in = base_in(20, 1000);            // KP 32: ceil(20 / 5) = 4 > 2
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(kz_route_short_geometry(in, none, r, &P, &sel) && P == 4 && sel == 64, "k = 20: P %d sel %d", P, sel);
        KzResearch long_lists;             // a re-search that asks for lists of 128: P = 16, sel = min(30 + 80, 256) = 110
        long_lists.prec = 0;
        long_lists.min_kp = 128;
        in = base_in(30, 1000);
        kz_route_lists(in, long_lists, &r);
        kz_route_tier(in, long_lists, &r);
        CHECK(r.cur.KP == 128 && kz_route_short_geometry(in, long_lists, r, &P, &sel) && P == 16 && sel == 110, "min_kp 128: P %d sel %d", P, sel);
        kz_route_take_dealt(&r, P, sel, false);
        CHECK(r.short_ord && r.cur.KP == 16 && r.cur.KSEL == 110 && r.cur.pieces == 16 && r.route_P == 16 && !r.wide_route, "take");
        kz_route_to_long(&r);
        CHECK(!r.short_ord && r.cur.KP == 128 && r.cur.KSEL == 0 && r.cur.pieces == 0, "back to the long list");
        // the long-k route as lists of 16 up to k = 320: P = 64, sel = min(320 + 80, 1024) = 400; k = 321: not
        in = base_in(320, 64 * 48);
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(kz_route_short_geometry(in, none, r, &P, &sel) && P == 64 && sel == 400, "k = 320: P %d sel %d", P, sel);
        in = base_in(321, 65 * 48);
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(!kz_route_short_geometry(in, none, r, &P, &sel), "k = 321");
    }
    // wide route: sel = min(wide_sel, 16 P), raised to k_eff + 16
    {
        int sel = 0;
        KzRouteIn in = base_in(10, 256);
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(kz_route_wide_geometry(in, r, 32, &sel) && sel == 256, "wide 32: sel %d", sel);
        CHECK(kz_route_wide_geometry(in, r, 8, &sel) && sel == 128, "wide 8: sel %d", sel);
        in.wide_sel = 16;
        CHECK(kz_route_wide_geometry(in, r, 32, &sel) && sel == 26, "wide_sel 16: sel %d", sel);
        in.n_tiles = 255;   // fewer than 8 tiles per list
        CHECK(!kz_route_wide_geometry(in, r, 32, &sel), "wide 32 on 255 tiles");
        in = base_in(100, 1000);   // 8 lists of 16 are no more than the list of 128 they would replace
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(!kz_route_wide_geometry(in, r, 8, &sel) && kz_route_wide_geometry(in, r, 32, &sel) && sel == 256, "k = 100 wide");
    }
    // the tier probe's verdicts on 1024 rows: hard above 1/2, the wide route tried above 1/8, taken at or below 1/4 of the probe and
    // below half of what the ordinary lists left
    CHECK(!kz_probe_verdict(1024, 512, 32).hard && kz_probe_verdict(1024, 513, 32).hard, "1/2");
    CHECK(!kz_probe_verdict(1024, 128, 32).try_wide && kz_probe_verdict(1024, 129, 32).try_wide, "1/8");
    CHECK(!kz_probe_verdict(1024, 1024, 0).try_wide, "wide route off");
    CHECK(kz_probe_wide_wins(1024, 1024, 256) && !kz_probe_wide_wins(1024, 1024, 257), "1/4");
    CHECK(kz_probe_wide_wins(1024, 513, 256) && !kz_probe_wide_wins(1024, 512, 256) && kz_probe_wide_wins(1024, 512, 255), "less than half");
    // a hard verdict: split-bf16 with lists of 64; no split-bf16 operands beyond 24 slices: the float32 ones
    {
        KzRouteIn in = base_in(10, 4000);
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        kz_route_start_hard(in, &r);
        CHECK(r.tier == KZ_TIER_BF && r.cur.KP == 64, "hard: tier %d KP %d", r.tier, r.cur.KP);
        in.kg = 4 * 32;
        in.n_slices = kz_h_nsr(in.kg);
        kz_route_lists(in, none, &r);
        kz_route_tier(in, none, &r);
        CHECK(r.tier == KZ_TIER_H, "32 slices: fp16");
        kz_route_start_hard(in, &r);
        CHECK(r.tier == KZ_TIER_F32, "hard at 32 slices: tier %d", r.tier);
    }
}

struct Gen {
    std::mt19937_64 rng{11};
    int pick(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }
    bool coin(int pct) { return pick(1, 100) <= pct; }
    KzRouteIn in() {
        KzRouteIn in;
        in.k_eff = coin(50) ? pick(1, 130) : pick(1, 4200);
        in.n_tiles = (int64_t)1 << pick(0, 20);
        if (in.n_tiles > 1) in.n_tiles += (int64_t)(rng() % (uint64_t)in.n_tiles);
        if (in.n_tiles > (1 << 20)) in.n_tiles = 1 << 20;
        in.n = in.n_tiles * 128 - pick(0, 127);
        in.kg = 4 * (coin(70) ? pick(1, 26) : pick(1, 140));
        in.n_slices = kz_h_nsr(in.kg);
        in.gemm_form = coin(85);
        in.same_kg = coin(92);
        in.range_ok = coin(50);
        in.precision = pick(0, 2);
        in.esc_bf = coin(80);
        in.short_ord = coin(80);
        const int mt[] = {1, 4, 8, 48};
        in.short_ord_min_tiles = mt[pick(0, 3)];
        const int wl[] = {0, 2, 8, 32};
        in.wide_lists = wl[pick(0, 3)];
        const int ws[] = {16, 256, 512};
        in.wide_sel = ws[pick(0, 2)];
        in.tier_probe = coin(80) ? 1024 : 0;
        in.dual = coin(20);
        if (in.dual && in.k_eff >= 13 && in.k_eff <= 110 && coin(70)) {   // the shared sweep's short lists (kz_knn_dual.h)
            in.short_kp = 16;
            in.short_pieces = (in.k_eff + 4) / 5;
            in.short_ksel = in.k_eff + 48 < in.short_pieces * 16 ? in.k_eff + 48 : in.short_pieces * 16;
        }
        in.dual_probed = in.dual && coin(50);
        return in;
    }
    KzResearch rs() {
        KzResearch r;
        if (coin(40)) return r;
        r.prec = pick(-1, 2);
        const int kp[] = {0, 16, 32, 64, 128};
        r.min_kp = kp[pick(0, 4)];
        r.more_lists = r.min_kp == 0 && coin(30);
        r.wide_lists = r.min_kp == 0 && !r.more_lists && coin(30) ? (coin(50) ? 32 : pick(2, 32)) : 0;
        r.no_short = coin(30);
        return r;
    }
};

// lists + tier + the routes on the dealt image, as kz_knn_impl takes them (have_image: kz_himage_dealt found memory)
static bool route_of(const KzRouteIn& in, const KzResearch& rs, bool have_image, KzRoute* r) {
    if (!kz_route_lists(in, rs, r)) return false;
    kz_route_tier(in, rs, r);
    int P = 0, sel = 0;
    if (kz_route_short_geometry(in, rs, *r, &P, &sel) && have_image) kz_route_take_dealt(r, P, sel, false);
    if (rs.wide_lists > 0 && kz_route_wide_geometry(in, *r, rs.wide_lists, &sel) && have_image) kz_route_take_dealt(r, rs.wide_lists, sel, true);
    return true;
}
static void check_lists(const KzRouteIn& in, const KzRoute& r, int trial, const char* what) {
    CHECK(r.cur.KP == 16 || r.cur.KP == 32 || r.cur.KP == 64 || r.cur.KP == 128, "trial %d %s: KP %d", trial, what, r.cur.KP);
    if (r.cur.KSEL <= 0) return;
    const int entries = pieces_of(r) * r.cur.KP;
    CHECK(in.k_eff <= r.cur.KSEL && r.cur.KSEL <= entries, "trial %d %s: k_eff %d KSEL %d entries %d", trial, what, in.k_eff, r.cur.KSEL, entries);
    CHECK(4 * kz_fin_wave_bytes(entries, r.cur.KSEL) <= 160 * 1024, "trial %d %s: %d B of LDS", trial, what, 4 * kz_fin_wave_bytes(entries, r.cur.KSEL));
    CHECK(entries <= KZ_FIN_MAXM, "trial %d %s: %d entries", trial, what, entries);
}

static void random_invariants() {
    Gen g;
    for (int trial = 0; trial < 6000; ++trial) {
        const KzRouteIn in = g.in();
        const KzResearch rs = g.rs();
        KzRoute r0;
        if (!kz_route_lists(in, rs, &r0)) {
            CHECK(in.k_eff > KZ_EXACT_MAX_K, "trial %d: k_eff %d refused", trial, in.k_eff);
            continue;
        }
        CHECK(!(r0.exact_only && r0.cur.KSEL > 0), "trial %d: exact-only with a selection", trial);
        check_lists(in, r0, trial, "lists");
        // any sequence of takes, then back: exactly the lists of kz_route_lists
        KzRoute r = r0;
        kz_route_tier(in, rs, &r);
        for (int step = g.pick(0, 4); step > 0; --step) {
            int P = 0, sel = 0;
            if (g.coin(50)) {
                if (kz_route_short_geometry(in, rs, r, &P, &sel)) {
                    kz_route_take_dealt(&r, P, sel, false);
                    check_lists(in, r, trial, "short");
                    CHECK(r.short_ord && r.cur.KP == 16 && r.cur.pieces == P && r.route_P == P, "trial %d: short take", trial);
                }
            } else {
                P = g.coin(50) ? in.wide_lists : g.pick(1, 40);
                if (kz_route_wide_geometry(in, r, P, &sel)) {
                    kz_route_take_dealt(&r, P, sel, true);
                    check_lists(in, r, trial, "wide");
                    CHECK(r.short_ord && r.wide_route && r.cur.pieces == P && sel >= in.k_eff && sel <= P * 16, "trial %d: wide take", trial);
                }
            }
            // a small launch cuts the ranges further, never beyond KZ_MAX_PIECES lists or the finalize kernel's LDS
            const int n_ytiles = (int)in.n_tiles;
            const int fpz = kz_route_sub_pieces(r, g.pick(1, 64), g.pick(1, 2048), n_ytiles);
            if (r.cur.pieces > 0 && r.tier == KZ_TIER_H) {
                CHECK(fpz >= r.cur.pieces && fpz % r.cur.pieces == 0 && (fpz == r.cur.pieces || fpz <= KZ_MAX_PIECES), "trial %d: %d pieces", trial, fpz);
                if (fpz > r.cur.pieces)
                    CHECK(4 * kz_fin_wave_bytes(fpz * 16, r.cur.KSEL) <= 160 * 1024 && n_ytiles / fpz >= 8, "trial %d: %d sub-pieces", trial, fpz);
            }
        }
        if (g.coin(30)) kz_route_next_tier(&r, g.pick(0, 2));
        kz_route_to_long(&r);
        CHECK(!r.short_ord && kz_route_same_lists(r.cur, r0.cur) && kz_route_same_lists(r.lng, r0.cur), "trial %d: to_long gives KP %d KSEL %d pieces %d", trial,
              r.cur.KP, r.cur.KSEL, r.cur.pieces);
    }
}

// The ladder of re-searches with every row failing every pass.
static void termination() {
    Gen g;
    int longest = 0;
    for (int trial = 0; trial < 6000; ++trial) {
        KzRouteIn in = g.in();
        if (in.k_eff > KZ_EXACT_MAX_K) in.k_eff = KZ_EXACT_MAX_K;
        KzResearch rs;   // a top-level call
        int64_t rows = g.coin(50) ? g.pick(1, 3000) : g.pick(1, 200000);
        const bool probed = g.coin(30);
        std::set<std::tuple<int, int, int, int, int>> seen;
        bool done = false;
        int steps = 0;
        for (; steps < 12 && !done; ++steps) {
            KzRoute r;
            CHECK(route_of(in, rs, g.coin(90), &r), "trial %d step %d: refused", trial, steps);
            check_lists(in, r, trial, "chain");
            const auto state = std::make_tuple(r.tier, r.cur.KP, r.cur.KSEL, r.cur.pieces, r.min_pieces_call);
            CHECK(seen.insert(state).second, "trial %d step %d: (tier %d, KP %d, KSEL %d, pieces %d) again", trial, steps, r.tier, r.cur.KP, r.cur.KSEL,
                  r.cur.pieces);
            const KzAfterPass ap = kz_after_pass(in, rs, r, probed && steps == 0, (int)rows, rows, 0);
            CHECK(!ap.rescued, "trial %d: rescued without a speculation", trial);
            if (!ap.escalate) {   // the exact kernels take what is left
                CHECK(r.tier == KZ_TIER_F32 || ap.exact_direct, "trial %d step %d: the ladder ends at tier %d", trial, steps, r.tier);
                done = true;
                break;
            }
            CHECK(!(ap.ladder && steps > 0), "trial %d step %d: the ladder after the fact in a re-search", trial, steps);
            KzResearch next = ap.next;
            CHECK(!kz_research_is_default(next), "trial %d step %d: a re-search that asks for nothing", trial, steps);
            in.dual = false;   // (a re-search is an ordinary search of a dense block of rows)
            in.short_pieces = in.short_ksel = in.short_kp = 0;
            in.dual_probed = false;
            if (ap.ladder && rows >= 4096) {   // kz_escalate_ladder: the wide route on all rows where a sample of them took it and it helped
                int P = in.wide_lists;
                if (in.n_tiles < (int64_t)8 * P) P = (int)(in.n_tiles / 8);
                KzRoute rw;
                if (P >= 8 && route_of(in, kz_research_wide(P), true, &rw) && rw.wide_route && g.coin(50)) next = kz_research_wide(P);
            }
            rs = next;
        }
        CHECK(done, "trial %d: no end after %d steps", trial, steps);
        if (steps + 1 > longest) longest = steps + 1;
    }
    std::printf("longest ladder: %d passes\n", longest);
    CHECK(longest <= 8, "a ladder of %d passes", longest);
}

int main() {
    documented_cases();
    random_invariants();
    termination();
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
