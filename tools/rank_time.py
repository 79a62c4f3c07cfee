"""Time of kz_gold_ranks (every query row with a gold id) beside kz_knn at k = 10 on the same shape with every row sent to the exact
kernels (eps_scale huge: the parent's only way to touch every pair exactly).  Both calls synchronise the stream before they return, so
the times are host wall times around one call, best of three after a warm-up.  The euclidean float32 cases also time
kz_gold_ranks_reduced on the same matrices and gold ids, once per kind, with arbitrary positive state vectors (the native call takes
any): `reduced_ms` and the ratio to the plain call.  One JSON line per case.

    python tools/rank_time.py [--out FILE] [--cases small|large|all] [--metric NAME] [--ranks-only]

`--metric euclidean --ranks-only` is the run to put under `rocprofv3 --kernel-trace --stats`: only the rank calls of one metric, so
that the trace's per-kernel totals split into the distance kernel and the two count kernels.
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
    ap.add_argument("--metric", default=None, help="only the cases of this metric")
    ap.add_argument("--ranks-only", action="store_true", help="skip the kz_knn comparison")
    args = ap.parse_args()
    ctx = N.Context.get()
    rng = np.random.default_rng(0)
    lines = []
    for metric, n, d in CASES[args.cases]:
        if args.metric and metric != args.metric:
            continue
        if metric == "jaccard":
            s, t = (rng.random((n, d)) < 0.4).astype(np.float32), (rng.random((n, d)) < 0.4).astype(np.float32)
        else:
            s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, metric), N.DeviceMatrix(ctx, t, metric)
        gold = ctx.to_device(rng.integers(0, n, n).astype(np.int64))
        rank_ms = best_of(lambda: N.gold_ranks(ctx, sm, tm, gold), ctx)
        ranks = N.gold_ranks(ctx, sm, tm, gold).numpy()
        reduced = {}
        if metric == "euclidean":
            # (states of the data's own scale: means near the typical distance, deviations a tenth of it)
            scale = float(np.sqrt(2.0 * d))
            q_a, t_a = (ctx.to_device(scale * (0.5 + 0.5 * rng.random(n))) for _ in range(2))
            q_b, t_b = (ctx.to_device(0.1 * scale * (0.5 + rng.random(n))) for _ in range(2))
            for name, kind in (("csls", N.RANK_CSLS), ("ls", N.RANK_LS), ("nicdm", N.RANK_NICDM), ("mp_normal", N.RANK_MP_NORMAL)):
                two = kind == N.RANK_MP_NORMAL
                q_state, t_state = ((q_a, q_b), (t_a, t_b)) if two else (q_a, t_a)
                reduced[name] = best_of(lambda: N.gold_ranks_reduced(ctx, sm, tm, gold, kind, q_state, t_state), ctx)
        line = {"metric": metric, "dtype": "float32", "n_query": n, "n_index": n, "d": d, "gold_ranks_ms": round(rank_ms, 2),
                "pairs_per_s_gold_ranks": round(n * n / rank_ms * 1e3, 0), "mean_rank": float(ranks.mean()), "min_rank": int(ranks.min())}
        if not args.ranks_only:
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
            line.update({"knn_k10_exact_ms": round(knn_ms, 2), "knn_k10_exact_no_range_ms": round(knn_dense_ms, 2),
                         "knn_exact_rows": int(stats["n_fallback_rows"]), "knn_fallback_ms": round(float(stats["fallback_ms"]), 2)})
        if reduced:
            line["reduced_ms"] = {k: round(v, 2) for k, v in reduced.items()}
            line["reduced_over_plain"] = {k: round(v / rank_ms, 3) for k, v in reduced.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
