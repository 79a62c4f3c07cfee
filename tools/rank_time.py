"""Time of kz_gold_ranks (every query row with a gold id) beside kz_knn at k = 10 on the same shape with every row sent to the exact
kernels (eps_scale huge: the parent's only way to touch every pair exactly).  Both calls synchronise the stream before they return, so
the times are host wall times around one call, best of three after a warm-up.  The euclidean float32 cases also time
kz_gold_ranks_reduced on the same matrices and gold ids, once per kind, with arbitrary positive state vectors (the native call takes
any): `reduced_ms` and the ratio to the plain call.  One JSON line per case.

    python tools/rank_time.py [--out FILE] [--cases small|large|all|wide] [--metric NAME] [--ranks-only] [--route exact|sweep|both]
                              [--gold uniform|correlated] [--n ROWS] [--rounds 7] [--no-reduced]

`--cases wide`: the text-encoder widths of the wide-row and parity-split count sweeps, 15 k x 15 k and 100 k x 100 k at d = 768, 1024,
1536 and 2048, euclidean and cosine on the same data (run it with `--route both --ranks-only --no-reduced --rounds 3`).

`--route both` (euclidean and cosine float32 cases) times gold_ranks(route="exact") and gold_ranks(route="sweep") ALTERNATED in one process -- seven
rounds after a warm-up of each, median and min .. max per route -- checks that the two rank vectors are equal and adds the sweep's
statistics (kz_rank_sweep_stats: band pairs, fallback rows, max_err_ratio, device times); it does the same for
gold_ranks_reduced against gold_ranks_reduced_sweep under CSLS and NICDM (`reduced_csls`, `reduced_nicdm`).  `--gold correlated`: the index row of every
gold id is its query row plus noise (ranks near 0), instead of uniform random gold ids (ranks near n / 2).

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
CASES["wide"] = [(m, n, d) for n in (15_000, 100_000) for d in (768, 1024, 1536, 2048) for m in ("euclidean", "cosine")]


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
    ap.add_argument("--route", default="exact", choices=["exact", "sweep", "both"])
    ap.add_argument("--gold", default="uniform", choices=["uniform", "correlated"])
    ap.add_argument("--n", type=int, default=None, help="only the cases of this many rows")
    ap.add_argument("--rounds", type=int, default=7, help="alternated rounds of --route both")
    ap.add_argument("--no-reduced", action="store_true", help="skip the kz_gold_ranks_reduced timings")
    args = ap.parse_args()
    ctx = N.Context.get()
    rng = np.random.default_rng(0)
    lines = []
    shape = None
    for metric, n, d in CASES[args.cases]:
        if (args.metric and metric != args.metric) or (args.n and n != args.n):
            continue
        if args.cases == "wide" and shape == (n, d):
            pass   # (the metrics of a wide shape share its data and gold ids)
        elif metric == "jaccard":
            s, t = (rng.random((n, d)) < 0.4).astype(np.float32), (rng.random((n, d)) < 0.4).astype(np.float32)
        else:
            s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        if args.cases != "wide" or shape != (n, d):
            gold_ids = rng.integers(0, n, n).astype(np.int64)
            if args.gold == "correlated" and metric != "jaccard":
                gold_ids = rng.permutation(n).astype(np.int64)
                t[gold_ids] = s + 0.05 * rng.standard_normal((n, d)).astype(np.float32)
        shape = (n, d)
        sm, tm = N.DeviceMatrix(ctx, s, metric), N.DeviceMatrix(ctx, t, metric)
        gold = ctx.to_device(gold_ids)
        route = "sweep" if args.route == "sweep" else "exact"
        keep = []   # (--cases wide: one timed call, whose ranks are kept -- the alternated rounds below are the measurement)
        rank_ms = best_of(lambda: keep.append(N.gold_ranks(ctx, sm, tm, gold, route=route)), ctx, reps=1 if args.cases == "wide" else 3)
        ranks = keep[-1].numpy()
        routes = {}
        if args.route == "both" and metric in ("euclidean", "cosine"):
            times, st = {"exact": [], "sweep": []}, {}
            for r in times:
                N.gold_ranks(ctx, sm, tm, gold, route=r)
            ctx.sync()
            for _ in range(args.rounds):
                for r in times:
                    t0 = time.perf_counter()
                    got = N.gold_ranks(ctx, sm, tm, gold, route=r, stats=st if r == "sweep" else None)
                    ctx.sync()
                    times[r].append((time.perf_counter() - t0) * 1e3)
                    assert np.array_equal(got.numpy(), ranks), "the routes disagree"
            routes = {"gold": args.gold, "sweep_stats": st,
                      **{f"{r}_ms": {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for r, v in times.items()}}
        reduced = {}
        if metric == "euclidean" and not args.no_reduced:
            # (states of the data's own scale: means near the typical distance, deviations a tenth of it)
            scale = float(np.sqrt(2.0 * d))
            q_a, t_a = (ctx.to_device(scale * (0.5 + 0.5 * rng.random(n))) for _ in range(2))
            q_b, t_b = (ctx.to_device(0.1 * scale * (0.5 + rng.random(n))) for _ in range(2))
            for name, kind in (("csls", N.RANK_CSLS), ("ls", N.RANK_LS), ("nicdm", N.RANK_NICDM), ("mp_normal", N.RANK_MP_NORMAL)):
                two = kind == N.RANK_MP_NORMAL
                q_state, t_state = ((q_a, q_b), (t_a, t_b)) if two else (q_a, t_a)
                reduced[name] = best_of(lambda: N.gold_ranks_reduced(ctx, sm, tm, gold, kind, q_state, t_state), ctx)
            if args.route == "both":   # kz_gold_ranks_reduced against kz_gold_ranks_reduced_sweep, alternated as above
                calls = {"exact": N.gold_ranks_reduced, "sweep": N.gold_ranks_reduced_sweep}
                for name, kind in (("csls", N.RANK_CSLS), ("nicdm", N.RANK_NICDM)):
                    times, st = {"exact": [], "sweep": []}, {}
                    want = calls["exact"](ctx, sm, tm, gold, kind, q_a, t_a).numpy()
                    calls["sweep"](ctx, sm, tm, gold, kind, q_a, t_a)
                    ctx.sync()
                    for _ in range(7):
                        for r in times:
                            t0 = time.perf_counter()
                            got = calls[r](ctx, sm, tm, gold, kind, q_a, t_a, **({"stats": st} if r == "sweep" else {}))
                            ctx.sync()
                            times[r].append((time.perf_counter() - t0) * 1e3)
                            assert np.array_equal(got.numpy(), want), "the reduced routes disagree"
                    routes[f"reduced_{name}"] = {"sweep_stats": dict(st), **{f"{r}_ms": {"median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                                                                                        "max": round(max(v), 3)} for r, v in times.items()}}
        line = {"metric": metric, "dtype": "float32", "n_query": n, "n_index": n, "d": d, "gold_ranks_ms": round(rank_ms, 2),
                "pairs_per_s_gold_ranks": round(n * n / rank_ms * 1e3, 0), "mean_rank": float(ranks.mean()), "min_rank": int(ranks.min())}
        line.update(routes)
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
