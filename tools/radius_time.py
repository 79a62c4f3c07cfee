"""Time of the radius calls (kz_radius_neighbors_reduced under CSLS, kz_radius_neighbors under the search metric; float32 euclidean,
standard-normal data) beside the list call of the same shape with k = 10: kz_knn_reduced, which walks the same exact float64 value
kernels and selects where the radius call counts, scans and fills.  The radius is the median over the rows of the row's own 10th
value in that list: about 10 pairs a row.  Per shape and value:
  * `list`      the list call (CSLS: kz_knn_reduced k = 10; plain: kz_knn k = 10, the certified fp16 MFMA route -- there for scale only);
  * `single`    radius_neighbors with the allocation policy: ONE walk where the first call's 32 pairs a row hold the result
                (`policy_walks` says whether they did);
  * `unsorted`  the same with sort_results = False (the row sort's share);
  * `counts`    capacity 0: count and scan alone;
  * `two_call`  counts first, then a call with capacity = total: what a caller pays when the first allocation was too small.
A pair of HIP events around each call (every call ends with a synchronise of the context's stream), one warm-up, the best of three,
one process.  Writes a markdown table (`--out`, default profiles/radius_neighbors.md) and prints one JSON line per row of it.

    python tools/radius_time.py [--out FILE] [--cases small|large|all]

Under `rocprofv3 --kernel-trace --stats -- python tools/radius_time.py --out /dev/null` the per-kernel totals split a call into the
distance kernel, the count, the two scans, the fill and the sort.
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402


def best_ms(ev, fn, reps=3):
    fn()   # warm-up: code objects, the pool's buffers
    return min(ev.ms(fn) for _ in range(reps))


def write_table(rows, out):
    """The markdown table of the rows main() measured (csls before plain within a shape)."""
    def num(v):
        return f"{v:,}".replace(",", " ")
    lines = ["# `radius_neighbors` beside the list call of the same shape (one MI355X, one process)", "",
             "`tools/radius_time.py`: float32 euclidean, standard-normal data, CSLS states from the 10 forward / reverse neighbours; the radius",
             "is the median over the rows of the row's own 10th value in the k = 10 list.  A pair of HIP events around each call (every call",
             "ends with a synchronise of the context's stream), one warm-up, the best of three.  `list`: `kz_knn_reduced` k = 10 under CSLS --",
             "the same exact float64 value kernels with a selection -- and `kz_knn` k = 10 under the plain metric, the certified fp16 MFMA",
             "route, which is there for scale only.  `single`: the allocation policy (walks: how many walks of the value kernels it took);",
             "`two call`: the counts, then a call with capacity = total.  The last column divides `single` by the shape's `kz_knn_reduced`",
             "time for both values: the call that walks the same value kernels.", "",
             "| shape (n_query × n_index × d) | value | pairs a row (longest row; empty rows) | list | single (walks) | unsorted | counts only | two call "
             "| single / `kz_knn_reduced` |",
             "|---|---|---|---|---|---|---|---|---|"]
    reduced_list = {(r["n_query"], r["d"]): r["list_ms"] for r in rows if r["value"] == "csls"}
    for r in rows:
        lines.append(f"| {num(r['n_query'])} × {num(r['n_index'])} × {r['d']} | {r['value']} | {r['pairs_per_row']:.1f} ({num(r['longest_row'])}; "
                     f"{num(r['empty_rows'])}) | {r['list_ms']:.2f} ms | {r['single_ms']:.2f} ms ({r['policy_walks']}) | {r['unsorted_ms']:.2f} ms "
                     f"| {r['counts_ms']:.2f} ms | {r['two_call_ms']:.2f} ms | {r['single_ms'] / reduced_list[(r['n_query'], r['d'])]:.3f} |")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/radius_neighbors.md")
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    args = ap.parse_args()
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
        # CSLS's own states: the means of the 10 forward / reverse neighbour distances (what `fit` / `kneighbors` compute)
        q_a = N.row_stats(ctx, N.knn(ctx, sm, tm, 10)[0], mean=True)[0]
        t_a = N.row_stats(ctx, N.knn(ctx, tm, sm, 10)[0], mean=True)[0]
        for value in ("csls", "plain"):
            if value == "csls":
                kind, state = N.RANK_CSLS, (q_a, t_a)
                def list_call():
                    return N.knn_reduced(ctx, sm, tm, 10, kind, *state)[0]
            else:
                kind, state = None, (None, None)
                def list_call():
                    return N.knn(ctx, sm, tm, 10)[0]
            radius = float(np.median(list_call().numpy()[:, 9]))

            def radius_call(**kw):
                return N.radius_neighbors(ctx, sm, tm, radius, kind, *state, **kw)

            def two_call():
                _, total = N.radius_counts(ctx, sm, tm, radius, kind, *state)
                return radius_call(capacity=total)
            indptr, ind, dist, total = radius_call()
            counts = np.diff(indptr.numpy())
            walks = 1 if total <= N.RADIUS_FIRST_CAPACITY_PER_ROW * n else 2   # (the policy's second call, where 32 pairs a row fall short)
            again = two_call()
            assert again[3] == total and np.array_equal(again[1].numpy(), ind.numpy())
            row = {"n_query": n, "n_index": n, "d": d, "value": value, "radius": radius, "pairs": total, "pairs_per_row": total / n,
                   "longest_row": int(counts.max()), "empty_rows": int((counts == 0).sum()), "policy_walks": walks,
                   "list_ms": best_ms(ev, list_call), "single_ms": best_ms(ev, radius_call),
                   "unsorted_ms": best_ms(ev, lambda: radius_call(sort_results=False)),
                   "counts_ms": best_ms(ev, lambda: N.radius_counts(ctx, sm, tm, radius, kind, *state)),
                   "two_call_ms": best_ms(ev, two_call)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    write_table(rows, args.out)


if __name__ == "__main__":
    main()
