"""Time of the whole-index calls on a precomputed distance matrix beside the same calls on the embeddings the matrix was computed
from (float32, sqeuclidean): kz_knn (k = 10) in both directions, kz_gold_ranks_reduced (CSLS, a gold id on every row), one
kz_softmin_rows call and Sinkhorn(n_iter=10).fit.  The matrix is the library's own value of every pair (kz_pair_values, block by
block, cast to float32) and stays in HBM: the precomputed calls read it in place.  A pair of HIP events around each call (every timed
call ends with a synchronise of the context's stream), one warm-up, the best of three.  One JSON line per shape.

    python tools/precomputed_time.py [--out FILE] [--cases small|large|all] [--trace-only]

`--trace-only` is the run to put under `rocprofv3 --kernel-trace --stats`: the two kz_knn calls on the matrix alone, three times each,
so that the trace's per-kernel totals give the rows-direction and the columns-direction gather kernel on the same matrix -- the same
bytes per value (the element in, 8 bytes out), the same number of launches.
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import Events  # noqa: E402

CASES = {"small": [(15_000, 300)], "large": [(50_000, 128)]}
CASES["all"] = CASES["small"] + CASES["large"]


def best_ms(ev, fn, reps=3):
    fn()   # warm-up: code objects, the pool's buffers
    return min(ev.ms(fn) for _ in range(reps))


def own_distances(ctx, sm, tm, block=1024):
    """float32 [n_s, n_t] on the device: kz_pair_values of every pair, cast."""
    n_s, n_t = sm.shape[0], tm.shape[0]
    out = ctx.empty((n_s, n_t), np.float32)
    ind = ctx.to_device(np.tile(np.arange(n_t, dtype=np.int64), (min(block, n_s), 1)))
    val = ctx.empty((min(block, n_s), n_t), np.float64)
    for r0 in range(0, n_s, block):
        nr = min(block, n_s - r0)
        N._check(ctx.lib.kz_pair_values(ctx.handle, sm.handle, r0, nr, tm.handle, ind.ptr, n_t, val.ptr), "kz_pair_values")
        N._check(ctx.lib.kz_cast_f64_f32(ctx.handle, val.ptr, out.view_rows(r0, nr).ptr, nr * n_t), "kz_cast_f64_f32")
    ctx.sync()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--trace-only", action="store_true", help="the two kz_knn calls on the matrix alone")
    args = ap.parse_args()
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    lines = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, "sqeuclidean"), N.DeviceMatrix(ctx, t, "sqeuclidean")
        D = own_distances(ctx, sm, tm)
        rows, cols = N.DeviceMatrix.precomputed(ctx, None, device_ptr=D.ptr.value, shape=D.shape, dtype=D.dtype, borrow=True, keepalive=D)
        if args.trace_only:
            for _ in range(3):
                N.knn(ctx, rows, cols, 10)
                N.knn(ctx, cols, rows, 10)
            continue
        # the two paths agree before anything is timed: same neighbours (the matrix holds the embedding path's values, rounded to float32)
        pi = N.knn(ctx, rows, cols, 10, q_count=64)[1].numpy()
        ei = N.knn(ctx, sm, tm, 10, q_count=64)[1].numpy()
        agree = float((pi == ei).mean())
        gold = ctx.to_device(rng.integers(0, n, n).astype(np.int64))
        scale = 2.0 * d   # the typical squared distance
        eps = 0.02 * scale
        q_a, t_a = (ctx.to_device(scale * (0.5 + 0.5 * rng.random(n))) for _ in range(2))
        off = ctx.to_device(0.1 * scale * rng.standard_normal(n))
        line = {"metric": "sqeuclidean", "dtype": "float32", "n_source": n, "n_target": n, "d": d, "eps": round(eps, 4), "reps": 3,
                "neighbours_agree_first_64_rows": round(agree, 4)}

        def sinkhorn(metric, *data):
            from kiez_amd import Kiez, Sinkhorn

            def fit():
                kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=Sinkhorn,
                          hubness_kwargs={"temperature": eps, "n_iter": 10})
                kz.fit(*data)
                ctx.sync()
            return fit
        calls = [
            ("knn_k10_rows", lambda: N.knn(ctx, rows, cols, 10), lambda: N.knn(ctx, sm, tm, 10)),
            ("knn_k10_columns", lambda: N.knn(ctx, cols, rows, 10), lambda: N.knn(ctx, tm, sm, 10)),
            ("gold_ranks_reduced_csls", lambda: N.gold_ranks_reduced(ctx, rows, cols, gold, N.RANK_CSLS, q_a, t_a),
             lambda: N.gold_ranks_reduced(ctx, sm, tm, gold, N.RANK_CSLS, q_a, t_a)),
            ("softmin_rows", lambda: N.softmin_rows(ctx, rows, cols, eps, off=off), lambda: N.softmin_rows(ctx, sm, tm, eps, off=off)),
            ("sinkhorn_fit_10_iterations", sinkhorn("precomputed", D), sinkhorn("sqeuclidean", s, t)),   # (embeddings: includes both uploads)
        ]
        for name, pre, emb in calls:
            p_ms, e_ms = best_ms(ev, pre), best_ms(ev, emb)
            line[f"{name}_precomputed_ms"] = round(p_ms, 3)
            line[f"{name}_embeddings_ms"] = round(e_ms, 3)
            line[f"{name}_embeddings_over_precomputed"] = round(e_ms / p_ms, 2)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rows, cols, D
        ctx.trim()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
