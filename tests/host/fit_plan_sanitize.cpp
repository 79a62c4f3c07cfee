// CPU-only check of the plan of a whole fit / kneighbors (kiez_amd/csrc/kz_fit_plan.h), built with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// by tests/test_fit_plan_host.py.  kz_fit_plan is enumerated over small n, K, every kind and every flag and compared with the rules
// of include/kiez_amd.h (kz_fit) written out a second time, rule by rule, without the header's control flow:
//   * the refusals and their status, decided from the inputs alone, in the documented order;
//   * which searches fit runs, whether the forward lists come out of fit, which tail kneighbors runs;
//   * the buffer sizes.
#include <cstdio>
#include <initializer_list>

#include "../../kiez_amd/csrc/kz_fit_plan.h"

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

// the expected status, from the list of refusals alone
static int expect_status(const KzFitIn& in) {
    if (in.kind < 0 || in.kind > 5) return 1;
    if (in.K < 1) return 1;
    if (in.kind != 0 && in.K < 2) return 1;                                                  // a reduction needs two candidates
    const long long side = in.single_source ? (long long)in.n_source - 1 : (long long)(in.n_source < in.n_target ? in.n_source : in.n_target);
    if (in.K > side) return 1;                                                               // no clamping here
    if (in.K > 4095) return 3;
    if (in.precomputed) return 3;
    if (!in.single_source && !in.agree) return 1;
    return 0;
}

static void check(const KzFitIn& in) {
    const KzFitPlan p = kz_fit_plan(in);
    const int want = expect_status(in);
    CHECK(p.status == want, "status %d, expected %d (ns %lld nt %lld single %d K %d kind %d sweep %d pre %d agree %d)", p.status, want,
          (long long)in.n_source, (long long)in.n_target, in.single_source, in.K, in.kind, in.shared_sweep, in.precomputed, in.agree);
    CHECK(p.why != nullptr, "no reason string");
    if (p.status != 0 || want != 0) {
        // a refusal plans nothing
        CHECK(p.search == 0 && p.tail == 0 && p.reverse_bytes == 0 && p.forward_bytes == 0 && p.state_bytes == 0 && p.split_bytes == 0 &&
                  p.forward_at_fit == 0,
              "a refused fit carries a plan");
        CHECK(p.status == 0 || p.why[0] != 0, "a refusal without a reason");
        return;
    }
    const long long ns = in.n_source, ni = in.single_source ? in.n_source : in.n_target;
    CHECK(p.n_query == ns && p.n_index == ni, "sizes %lld x %lld", (long long)p.n_query, (long long)p.n_index);
    CHECK(p.forward_exclude_self == (in.single_source ? 1 : 0), "exclude_self %d", p.forward_exclude_self);
    if (in.kind == 0) {
        CHECK(p.search == KZ_FIT_SEARCH_NONE && p.tail == KZ_FIT_TAIL_KNN && !p.forward_at_fit, "no reduction: search %d tail %d", p.search, p.tail);
        CHECK(p.reverse_bytes == 0 && p.forward_bytes == 0 && p.state_bytes == 0 && p.split_bytes == 0 && p.n_state == 0, "no reduction owns buffers");
        return;
    }
    // the searches
    int search;
    if (!in.single_source)
        search = in.shared_sweep ? KZ_FIT_SEARCH_DUAL : KZ_FIT_SEARCH_REVERSE;
    else
        search = (in.shared_sweep && in.K + 1 <= ns && in.K + 1 <= 110) ? KZ_FIT_SEARCH_SPLIT : KZ_FIT_SEARCH_REVERSE;
    CHECK(p.search == search, "search %d, expected %d (single %d sweep %d K %d n %lld)", p.search, search, in.single_source, in.shared_sweep, in.K, ns);
    if (search == KZ_FIT_SEARCH_DUAL) CHECK(p.larger_first == (ns >= ni ? 1 : 0), "larger first %d for %lld x %lld", p.larger_first, ns, ni);
    CHECK(p.forward_at_fit == (search == KZ_FIT_SEARCH_DUAL || search == KZ_FIT_SEARCH_SPLIT ? 1 : 0), "forward at fit %d for search %d",
          p.forward_at_fit, search);
    // the tail
    if (in.kind == 5) {
        CHECK(p.tail == KZ_FIT_TAIL_EMPIRIC && p.n_state == 0 && p.fused == 0, "MP empiric: tail %d state %d", p.tail, p.n_state);
    } else {
        CHECK(p.tail == KZ_FIT_TAIL_FUSED, "pointwise kind %d: tail %d", in.kind, p.tail);
        CHECK(p.fused == (in.K <= 128 ? 1 : 0), "fused %d at K %d", p.fused, in.K);
        CHECK(p.n_state == (in.kind == 4 ? 2 : 1), "state vectors %d for kind %d", p.n_state, in.kind);
    }
    // the buffers
    CHECK(p.reverse_bytes == (size_t)(16 * ni * in.K), "reverse bytes %zu", p.reverse_bytes);
    CHECK(p.forward_bytes == (size_t)(16 * ns * in.K), "forward bytes %zu", p.forward_bytes);
    CHECK(p.state_bytes == (size_t)(8 * ni * p.n_state), "state bytes %zu", p.state_bytes);
    CHECK(p.split_bytes == (search == KZ_FIT_SEARCH_SPLIT ? (size_t)(16 * ns * (in.K + 1)) : 0), "split bytes %zu", p.split_bytes);
}

int main() {
    int n = 0;
    const long long sizes[] = {1, 2, 3, 11, 12, 109, 110, 111, 112, 129, 130, 300, 5000};
    const int Ks[] = {-1, 0, 1, 2, 3, 10, 11, 108, 109, 110, 111, 127, 128, 129, 130, 299, 300, 301, 4095, 4096, 4999, 5000};
    for (long long ns : sizes)
        for (long long nt : sizes)
            for (int single : {0, 1}) {
                if (single && nt != sizes[0]) continue;   // (the target's size is not read: one pass)
                for (int K : Ks)
                    for (int kind = -1; kind <= 6; ++kind)
                        for (int sweep : {0, 1})
                            for (int pre : {0, 1})
                                for (int agree : {0, 1}) {
                                    KzFitIn in{};
                                    in.n_source = ns;
                                    in.n_target = single ? 987654321 : nt;   // (must not matter for single source)
                                    in.single_source = single;
                                    in.K = K;
                                    in.kind = kind;
                                    in.shared_sweep = sweep;
                                    in.precomputed = pre;
                                    in.agree = agree;
                                    check(in);
                                    ++n;
                                }
            }
    // sizes past 2^31 entries: the byte counts are 64-bit
    KzFitIn big{};
    big.n_source = 3000000000ll;
    big.n_target = 2500000000ll;
    big.K = 100;
    big.kind = KZ_FP_CSLS;
    big.shared_sweep = 1;
    big.agree = 1;
    check(big);
    ++n;
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
