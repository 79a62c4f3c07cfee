#!/usr/bin/env python3
"""Randomised cross-check of the value regimes of tests/value_regimes.py on the GPU box: data scaled by 2^-66 .. 2^e_max, per-row
scales under cosine, query / index scale ratios up to 2^20, common offsets up to 1e5 spreads, single rows 1e3 .. 1e9 times the rest,
row norms spread over 2^-6 .. 2^6, rows just under the input limit -- random (regime, parameter, shape, metric, dtype, k, single)
through the three first-pass tiers (bit-identical, max_err_ratio < 1), against the oracle (index for index where the oracle's own
neighbours are >= 16 ulps of |q|^2 + |y|^2 apart in every row, tie-tolerantly else; rows on which the oracle's own order contradicts
exact arithmetic by >= 2 ulps are counted as `oracle-misordered` and not compared) and, for the power-of-two regimes, against the
unscaled run bit for bit; every third two-matrix case also through the shared sweep (`dual_force` 1) against two searches.

    python3 tools/fuzz_values.py [n_cases] [seed]
"""
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402
from tests import value_regimes as V  # noqa: E402  (generators and the checker the GPU tests use)


def random_case(rng):
    regime = str(rng.choice(["pow2", "cosine_row_scales", "mismatch", "offset", "outlier", "heavy_rows", "limit"]))
    d = int(rng.choice([3, 17, 48, 64, 100, 200, 208, 257, 320, 384, 400, 500, 768, 1024, 1536, 2049]))
    dtype = np.float32 if rng.rand() < 0.5 else np.float64
    metric = str(rng.choice(["euclidean", "sqeuclidean", "cosine"]))
    n_q, n_i = int(rng.choice([1, 31, 129, 257, 700])), int(rng.choice([127, 129, 500, 1500, 2049, 4000]))
    k = int(rng.choice([1, 5, 10, 13, 30, 50, 110]))
    single = bool(rng.rand() < 0.25)
    c = dict(regime=regime, d=d, dtype=dtype, metric=metric, n_q=n_q, n_i=n_i, single=single, seed=int(rng.randint(1 << 30)),
             short=int(rng.randint(0, 2)), gen=str(rng.choice(["rand", "randn"])), param=None)
    if regime == "pow2":
        c["param"] = V.POW2_EXPONENTS[rng.randint(len(V.POW2_EXPONENTS))]
        if c["param"] == -66:     # float32 products (and float32 euclidean distances) leave the normal range: float64, no euclidean
            c["dtype"] = np.float64
            c["metric"] = metric if metric != "euclidean" else "sqeuclidean"
    elif regime == "cosine_row_scales":
        c["metric"], c["param"] = "cosine", "rows"
    elif regime == "mismatch":
        c["r"], c["larger"], c["single"] = int(rng.choice(V.MISMATCH_R)), str(rng.choice(["query", "index"])), False
        c["param"] = f"{c['larger']}*2^{c['r']}"
    elif regime == "offset":
        c["param"] = float(rng.choice([1e2, 1e3, 1e4, 1e5]))
    elif regime == "outlier":
        c["m"], c["where"], c["side"] = float(rng.choice(V.OUTLIER_M)), str(rng.choice(V.OUTLIER_WHERE)), str(rng.choice(V.OUTLIER_SIDE))
        c["param"] = f"{c['m']:g}-{c['where']}-{c['side']}"
        if c["where"] == "ragged":
            c["n_i"] = n_i = max(n_i, 500)   # (128 j + 1 rows)
    elif regime == "heavy_rows":
        c["metric"], c["single"], c["param"] = (metric if metric != "cosine" else "euclidean"), False, "light_first"
    else:
        c["single"], c["param"] = False, "under"
    if c["metric"] == "cosine" and regime in ("pow2", "mismatch"):
        c["gen"] = "randn"
    c["k"] = max(1, min(k, (n_i if not c["single"] else n_i - 1) - 2))
    return c


def shared_sweep_problems(ctx, q, y, k, metric):
    """kz_knn_dual with the shared sweep forced against `dual_stride` 0 (two searches) and against kz_knn itself, bit for bit; the
    rounding bound's self-check of all four searches."""
    out, problems = {}, []
    try:
        for stride in (0, 1):
            ctx.set_option("dual_force", 1)
            ctx.set_option("dual_stride", stride)
            am, bm = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
            (d1, i1, s1), (d2, i2, s2) = N.knn_dual(ctx, am, bm, k)
            out[stride] = (d1.numpy(), i1.numpy(), d2.numpy(), i2.numpy())
            name = "shared sweep" if stride else "two searches"
            problems += V.stats_problems(s1, len(q), f"{name} a->b") + V.stats_problems(s2, len(y), f"{name} b->a")
        ctx.set_option("dual_force", 0)
        am, bm = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
        dd, ii, _ = N.knn(ctx, am, bm, k)
        if not (np.array_equal(out[1][0], dd.numpy()) and np.array_equal(out[1][1], ii.numpy())):
            problems.append("the shared sweep's a->b differs from kz_knn")
        dd, ii, _ = N.knn(ctx, bm, am, k)
        if not (np.array_equal(out[1][2], dd.numpy()) and np.array_equal(out[1][3], ii.numpy())):
            problems.append("the shared sweep's b->a differs from kz_knn")
    finally:
        ctx.set_option("dual_force", 0)
        ctx.set_option("dual_stride", 1)
    if not all(np.array_equal(a, b) for a, b in zip(out[0], out[1])):
        problems.append("the shared sweep differs from two searches")
    return problems


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    ctx = N.Context.get()
    bad = 0
    for i in range(n_cases):
        c = random_case(rng)
        data = V.make(c)
        q, y = data[1] if c["regime"] in ("pow2", "cosine_row_scales") else data
        gaps, _ = V.gap_ulps(q, y, c["k"], c["metric"], exclude_self=c["single"])
        strict = bool(gaps.min() >= V.STRICT_GAP_ULPS)
        # rows on which the oracle itself orders a pair against exact arithmetic although it is >= 2 ulps apart (seen at an offset
        # of 1e5 spreads, d = 200: its expansion is several ulps off there) say nothing about the device: not compared, but counted
        misordered = np.flatnonzero(gaps <= -V.TIE_ULPS)
        problems, ratios, st = V.check_knn_case(ctx, c, strict=strict, skip_rows=misordered)
        dual = i % 3 == 0 and not c["single"] and c["k"] <= min(len(q), len(y), 110)
        if dual:
            problems += shared_sweep_problems(ctx, q, y, c["k"], c["metric"])
        bad += 1 if problems else 0
        print("BAD" if problems else "ok ", f"{c['regime']}({c['param']}) n_q={len(q)} n_i={len(y)} d={c['d']} {c['metric']} {np.dtype(c['dtype']).name}",
              f"k={c['k']} single={c['single']} short={c['short']} dual={int(dual)} strict={int(strict)} oracle-misordered={len(misordered)}", "tier", V.TIER_NAMES[st["first_pass"]],
              "fail", st["n_first_pass_fail"], "esc", st["n_escalated_rows"], "fb", st["n_fallback_rows"],
              "ratio " + " ".join(f"{t} {r:.3f}" for t, r in sorted(ratios.items())), *problems, flush=True)
    print("cases", n_cases, "bad", bad)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
