"""Time of (a) one kz_softmin_rows call, (b) one kz_gold_ranks_reduced CSLS call with a gold id on every row on the same matrices in
the same process -- the same value work with a count where the first has a reduction -- and (c) Sinkhorn(n_iter=10).fit on the same
data (float32 euclidean; 2 L soft-min calls and the two uploads).  A pair of HIP events around each call, one warm-up, the median of
`--reps` (>= 5) calls: every timed call ends with a synchronise of the context's stream, so the events -- recorded on the otherwise
idle null stream before the call and after it -- enclose all of its device work.  One JSON line per shape.

    python tools/sinkhorn_time.py [--out FILE] [--cases small|large|all] [--reps N] [--native-only]

`--native-only` is the run to put under `rocprofv3 --kernel-trace --stats`: the two native calls alone, so that the trace's per-kernel
totals split into the distance kernel, the count kernel and the two soft-min kernels.
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--native-only", action="store_true", help="skip Sinkhorn.fit")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    lines = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
        gold = ctx.to_device(rng.integers(0, n, n).astype(np.int64))
        # (states and a temperature of the data's own scale: the typical distance is sqrt(2 d))
        scale = float(np.sqrt(2.0 * d))
        eps = 0.02 * scale
        q_a, t_a = (ctx.to_device(scale * (0.5 + 0.5 * rng.random(n))) for _ in range(2))
        off = ctx.to_device(0.1 * scale * rng.standard_normal(n))
        softmin_ms = median_ms(ev, lambda: N.softmin_rows(ctx, sm, tm, eps, off=off), reps)
        rank_ms = median_ms(ev, lambda: N.gold_ranks_reduced(ctx, sm, tm, gold, N.RANK_CSLS, q_a, t_a), reps)
        line = {"metric": "euclidean", "dtype": "float32", "n_query": n, "n_index": n, "d": d, "eps": round(eps, 4), "reps": reps,
                "softmin_rows_ms": round(softmin_ms, 2), "gold_ranks_reduced_ms": round(rank_ms, 2),
                "softmin_rows_over_gold_ranks_reduced": round(softmin_ms / rank_ms, 3),
                "pairs_per_s_softmin_rows": round(n * n / softmin_ms * 1e3, 0)}
        if not args.native_only:
            from kiez_amd import Kiez, Sinkhorn

            def fit():
                kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=Sinkhorn,
                          hubness_kwargs={"temperature": eps, "n_iter": 10})
                kz.fit(s, t)
                ctx.sync()
                return kz
            line["sinkhorn_fit_10_iterations_ms"] = round(median_ms(ev, fit, reps), 2)   # (includes both uploads)
            line["sinkhorn_fit_over_softmin_rows"] = round(line["sinkhorn_fit_10_iterations_ms"] / softmin_ms, 2)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
