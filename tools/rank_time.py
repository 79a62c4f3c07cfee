"""Time of kz_gold_ranks (every query row with a gold id) beside kz_knn at k = 10 on the same shape with every row sent to the exact
kernels (eps_scale huge: the parent's only way to touch every pair exactly).  Both calls synchronise the stream before they return, so
the times are host wall times around one call, best of three after a warm-up.  One JSON line per case.

    python tools/rank_time.py [--out FILE] [--cases small|large|all]
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402

CASES = {"small": [("euclidean", 15_000, 300), ("manhattan", 15_000, 300), ("jaccard", 15_000, 300)],
         "large": [("euclidean", 100_000, 128)]}
CASES["all"] = CASES["small"] + CASES["large"]


def best_of(fn, ctx, reps=3):
    fn()
    ctx.sync()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    args = ap.parse_args()
    ctx = N.Context.get()
    rng = np.random.default_rng(0)
    lines = []
    for metric, n, d in CASES[args.cases]:
        if metric == "jaccard":
            s, t = (rng.random((n, d)) < 0.4).astype(np.float32), (rng.random((n, d)) < 0.4).astype(np.float32)
        else:
            s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, metric), N.DeviceMatrix(ctx, t, metric)
        gold = ctx.to_device(rng.integers(0, n, n).astype(np.int64))
        rank_ms = best_of(lambda: N.gold_ranks(ctx, sm, tm, gold), ctx)
        ranks = N.gold_ranks(ctx, sm, tm, gold).numpy()
        stats = {}

        def search():
            stats.update(N.knn(ctx, sm, tm, 10)[2])
        ctx.set_option("eps_scale", 1e30)
        try:
            knn_ms = best_of(search, ctx)           # (as the library runs it: the range re-search is tried first, kz_range.h)
            ctx.set_option("exact_rows", 2)         # (the whole-index exact kernels at once: what kz_gold_ranks calls)
            knn_dense_ms = best_of(search, ctx)
        finally:
            ctx.set_option("eps_scale", 1.0)
            ctx.set_option("exact_rows", 3)
        line = {"metric": metric, "dtype": "float32", "n_query": n, "n_index": n, "d": d, "gold_ranks_ms": round(rank_ms, 2),
                "knn_k10_exact_ms": round(knn_ms, 2), "knn_k10_exact_no_range_ms": round(knn_dense_ms, 2),
                "knn_exact_rows": int(stats["n_fallback_rows"]),
                "knn_fallback_ms": round(float(stats["fallback_ms"]), 2), "pairs_per_s_gold_ranks": round(n * n / rank_ms * 1e3, 0),
                "mean_rank": float(ranks.mean()), "min_rank": int(ranks.min())}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
