"""Time of kneighbors_whole_index on its two routes: route="exact" (kz_knn_reduced: the float64 value kernels over every pair, then a
two-level selection) and route="sweep" (kz_knn_reduced_sweep: thresholds seeded from the forward candidate lists, the rank-one emit
sweep of the fp16 images, the exact w of its candidates, a per-row selection).  CSLS, k = 10, n_candidates = 10, float32 euclidean and
cosine, standard-normal data, 15 k x 15 k x 300 and 100 k x 100 k x 128, after one fit.
The routes alternate call by call in one process; a pair of HIP events around each call (every call ends with a synchronise of the
context's stream), one warm-up each, the median of five.  The two routes' results are compared byte for byte before anything is timed.
The sweep call's statistics (route taken, log entries, the largest error ratio, the device times of its stages) are part of the row.
Writes a markdown table (`--out`, default profiles/whole_index_sweep.md) and one JSON line per row (`--jsonl`).

    python tools/whole_index_sweep_time.py [--out FILE] [--jsonl FILE] [--cases small|large|all] [--reps 5]

Under `rocprofv3 --kernel-trace --stats -- python tools/whole_index_sweep_time.py --out /dev/null --jsonl /dev/null --reps 1` the
per-kernel totals split the sweep route into the seed and threshold kernels, the emit sweep, the two sorts, the resolve and the select.
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from tools.radius_sweep_time import alternated_ms  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402


def write_table(rows, out):
    def num(v):
        return f"{v:,}".replace(",", " ")
    lines = ["# `kneighbors_whole_index`: route=\"sweep\" beside route=\"exact\" (one MI355X, one process)", "",
             "`tools/whole_index_sweep_time.py`: CSLS, k = 10, n_candidates = 10, float32, standard-normal data; routes alternated call by call,",
             "a pair of HIP events around each call, one warm-up, the median of five.  `candidates`: log entries of the sweep; `sweep` /",
             "`resolve`: device times of the call's stages (seeds, thresholds and sweep; sorts, exact w and selection).", "",
             "| shape | metric | exact | sweep | route taken | candidates | per row | max err ratio | sweep | resolve | fallback |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        s = r["sweep_stats"]
        lines.append(f"| {num(r['n_query'])} × {num(r['n_index'])} × {r['d']} | {r['metric']} | {r['exact_ms']:.2f} ms | {r['sweep_ms']:.2f} ms "
                     f"| {s['route_taken']} | {num(s['n_candidates'])} | {s['n_candidates'] / r['n_query']:.1f} | {s['max_err_ratio']:.3f} "
                     f"| {s['sweep_ms']:.2f} ms | {s['resolve_ms']:.2f} ms | {s['fallback_ms']:.2f} ms |")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/whole_index_sweep.md")
    ap.add_argument("--jsonl", default="profiles/whole_index_sweep_time.jsonl")
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        for metric in ("euclidean", "cosine"):
            kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness="CSLS").fit(s, t)
            exact = kz.kneighbors_whole_index_device(10)
            sweep = kz.kneighbors_whole_index_device(10, route="sweep")
            assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(exact, sweep))
            del exact, sweep
            ms = alternated_ms(ev, {"exact": lambda: kz.kneighbors_whole_index_device(10),
                                    "sweep": lambda: kz.kneighbors_whole_index_device(10, route="sweep")}, args.reps)
            kz.kneighbors_whole_index_device(10, route="sweep")
            row = {"n_query": n, "n_index": n, "d": d, "metric": metric, "hubness": "CSLS", "k": 10, "n_candidates": 10,
                   "exact_ms": ms["exact"], "sweep_ms": ms["sweep"], "sweep_stats": dict(kz.algorithm.reduced_stats_)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    write_table(rows, args.out)
    with open(args.jsonl, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
