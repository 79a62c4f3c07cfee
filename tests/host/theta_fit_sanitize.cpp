// CPU-only check of the fit behind the shared sweep's MODEL THRESHOLDS (kiez_amd/csrc/kz_floor.h: kz_theta_fit, kz_floor_r2),
// built with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// by tests/test_theta_fit.py and run as a program of its own.  Fit rows: [|t_c|^2, k_p keys in descending order] per probe row.
//   * a probe whose k-th keys ARE a line is recovered (alpha, beta, margin ~ 0), and the counts are the ones constructed;
//   * constant |t_c|^2: beta = 0, alpha = the mean k-th key, margin = the largest shortfall;
//   * non-finite values and zero rows: no model; k_p < k: no model;
//   * saturated rows (every kept neighbour at or above the threshold) and short rows (fewer than k) are counted exactly;
//   * random probes: no row short at margin scale >= 1, mean / max of the counts agree with a recount.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../kiez_amd/csrc/kz_floor.h"

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

int main() {
    {   // an exact line: row i has its k-th key ON the line, `above[i]` keys at or above it in all
        const int n = 64, k_p = 12, k = 4, w = k_p + 1;
        std::vector<double> r((size_t)n * w);   // exactly sized: ASan sees any out-of-range access
        std::vector<int> above(n);
        for (int i = 0; i < n; ++i) {
            const double x = 2.0 + 0.125 * i, line = -1.5 + 0.75 * x;
            above[i] = k + i % (k_p - k);       // k .. k_p - 1: neither short nor saturated
            r[(size_t)i * w] = x;
            for (int j = 1; j <= k_p; ++j) {
                double key;
                if (j < k) key = line + 0.01 * (k - j);
                else if (j == k) key = line;
                else if (j <= above[i]) key = line;   // ties with the k-th key: at the threshold, counted
                else key = line - 0.01 * (j - above[i]);
                r[(size_t)i * w + j] = key;
            }
        }
        KzThetaFit f;
        CHECK(kz_theta_fit(r.data(), n, k_p, k, 1.3, &f), "line rejected");
        CHECK(std::fabs(f.alpha + 1.5) < 1e-9 && std::fabs(f.beta - 0.75) < 1e-10 && f.margin < 1e-9, "line: alpha %g beta %g margin %g", f.alpha,
              f.beta, f.margin);
        // (margin ~ 1e-16 of rounding: a key constructed ON the line may fall a rounding error below alpha + beta x; the counts are
        //  checked against a recount with the fitted numbers, and against the construction within that tolerance)
        long long total = 0;
        int mx = 0;
        for (int i = 0; i < n; ++i) {
            const double tau = f.alpha + f.beta * r[(size_t)i * w] - f.margin;
            int c = 0;
            for (int j = 1; j <= k_p; ++j) c += r[(size_t)i * w + j] >= tau ? 1 : 0;
            total += c;
            mx = std::max(mx, c);
        }
        CHECK(f.max_count == mx && std::fabs(f.mean_count - (double)total / n) < 1e-12, "line: counts %d / %g against %d / %g", f.max_count,
              f.mean_count, mx, (double)total / n);
        CHECK(f.n_saturated == 0, "line: %d saturated rows", f.n_saturated);
        CHECK(f.max_count <= k_p - 1 && f.mean_count <= (double)(k_p - 1), "line: counts beyond the construction");
    }
    {   // constant |t_c|^2
        const int n = 3, k_p = 2, k = 1, w = 3;
        std::vector<double> r = {2.0, 1.0, 0.5, 2.0, 3.0, 2.5, 2.0, -1.0, -2.0};
        KzThetaFit f;
        CHECK(kz_theta_fit(r.data(), n, k_p, k, 1.0, &f), "constant x rejected");
        CHECK(f.beta == 0.0 && std::fabs(f.alpha - 1.0) < 1e-12 && std::fabs(f.margin - 2.0) < 1e-12, "constant x: %g %g %g", f.alpha, f.beta, f.margin);
        // tau = -1 for every row: row 0 {1, .5} -> 2 (saturated), row 1 {3, 2.5} -> 2 (saturated), row 2 {-1, -2} -> 1
        CHECK(f.n_saturated == 2 && f.n_short == 0 && f.max_count == 2 && std::fabs(f.mean_count - 5.0 / 3.0) < 1e-12, "constant x: sat %d short %d max %d mean %g",
              f.n_saturated, f.n_short, f.max_count, f.mean_count);
        (void)w;
        // the model itself (scale 0): tau = 1: row 0 -> 1, row 1 -> 2 (saturated), row 2 -> 0 (short)
        CHECK(kz_theta_fit(r.data(), n, k_p, k, 0.0, &f), "scale 0 rejected");
        CHECK(f.margin == 0.0 && f.n_saturated == 1 && f.n_short == 1 && f.max_count == 2 && std::fabs(f.mean_count - 1.0) < 1e-12, "scale 0: sat %d short %d max %d mean %g",
              f.n_saturated, f.n_short, f.max_count, f.mean_count);
        // one row
        CHECK(kz_theta_fit(r.data(), 1, k_p, k, 1.0, &f) && f.margin == 0.0 && f.beta == 0.0 && f.max_count == 1 && f.n_short == 0, "one row");
    }
    {   // no model
        std::vector<double> r = {2.0, 1.0, 0.5, 2.5, 3.0, 2.5, 3.0, -1.0, -2.0};
        KzThetaFit f;
        CHECK(!kz_theta_fit(r.data(), 0, 2, 1, 1.0, &f), "zero rows accepted");
        CHECK(f.alpha == 0.0 && f.beta == 0.0 && f.margin == 0.0 && f.max_count == 0 && f.n_saturated == 0 && f.n_short == 0, "zero rows: output not cleared");
        CHECK(!kz_theta_fit(r.data(), 3, 2, 3, 1.0, &f), "k_p < k accepted");
        CHECK(!kz_theta_fit(r.data(), 3, 2, 0, 1.0, &f), "k = 0 accepted");
        const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
        for (double v : bad) {
            std::vector<double> q = r;
            q[4] = v;   // the k-th key of row 1
            CHECK(!kz_theta_fit(q.data(), 3, 2, 1, 1.0, &f), "non-finite k-th key accepted (%g)", v);
            q = r;
            q[3] = v;   // |t_c|^2 of row 1
            CHECK(!kz_theta_fit(q.data(), 3, 2, 1, 1.0, &f), "non-finite |t_c|^2 accepted (%g)", v);
        }
        // a non-finite key that is NOT the k-th: the model stands, the key counts as an event only when it compares >= tau
        std::vector<double> q = r;
        q[5] = std::numeric_limits<double>::quiet_NaN();
        CHECK(kz_theta_fit(q.data(), 3, 2, 1, 1.0, &f), "NaN beyond the k-th key rejected the model");
        std::vector<double> pr = {1.0, 2.0, 1.0, 3.0, 1.0, std::numeric_limits<double>::quiet_NaN()};
        CHECK(kz_floor_r2(pr.data(), 3) == 0.0 && kz_floor_r2(pr.data(), 0) == 0.0 && kz_floor_r2(pr.data(), 1) == 0.0, "r2 of degenerate probes");
        pr = {1.0, 2.0, 2.0, 4.0, 3.0, 6.0};
        CHECK(std::fabs(kz_floor_r2(pr.data(), 3) - 1.0) < 1e-12, "r2 of a line");
        pr = {1.0, 2.0, 1.0, 4.0, 1.0, 6.0};
        CHECK(kz_floor_r2(pr.data(), 3) == 0.0, "r2 with constant x");
    }
    {   // random probes
        std::mt19937_64 rng(11);
        std::normal_distribution<double> gauss(0.0, 1.0);
        std::uniform_real_distribution<double> uni(0.0, 1.0);
        for (int trial = 0; trial < 200; ++trial) {
            const int n = 1 + (int)(uni(rng) * 1500), k_p = 1 + (int)(uni(rng) * 110), k = 1 + (int)(uni(rng) * k_p), w = k_p + 1;
            const double a = 10.0 * gauss(rng), b = gauss(rng), noise = 0.01 + uni(rng), gap = 0.001 + 0.2 * uni(rng);
            std::vector<double> r((size_t)n * w);
            for (int i = 0; i < n; ++i) {
                const double x = 5.0 + 3.0 * uni(rng);
                r[(size_t)i * w] = x;
                std::vector<double> keys(k_p);
                for (int j = 0; j < k_p; ++j) keys[j] = a + b * x + noise * gauss(rng) - gap * j * uni(rng);
                std::sort(keys.begin(), keys.end(), [](double p, double q) { return p > q; });
                for (int j = 0; j < k_p; ++j) r[(size_t)i * w + 1 + j] = keys[j];
            }
            const double scale = trial % 2 ? 1.0 : 1.3;
            KzThetaFit f;
            CHECK(kz_theta_fit(r.data(), n, k_p, k, scale, &f), "trial %d: finite probe rejected", trial);
            CHECK(f.n_short == 0, "trial %d: %d rows short of k at margin scale %g", trial, f.n_short, scale);
            long long total = 0;
            int mx = 0, sat = 0;
            for (int i = 0; i < n; ++i) {
                const double tau = f.alpha + f.beta * r[(size_t)i * w] - f.margin;
                int c = 0;
                for (int j = 1; j <= k_p; ++j) c += r[(size_t)i * w + j] >= tau ? 1 : 0;
                total += c;
                mx = std::max(mx, c);
                sat += c == k_p ? 1 : 0;
            }
            CHECK(f.max_count == mx && f.n_saturated == sat && std::fabs(f.mean_count - (double)total / n) < 1e-9, "trial %d: counts differ from a recount", trial);
            CHECK(f.max_count >= k && f.max_count <= k_p, "trial %d: max count %d outside [%d, %d]", trial, f.max_count, k, k_p);
        }
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
