"""Time of radius_neighbors on its two routes: route="exact" (kz_radius_neighbors: the float64 value kernels over every pair) and
route="sweep" (kz_radius_neighbors_sweep: the fp16 emit sweep, then the exact values of its candidates).  float32 euclidean and
cosine, standard-normal data, 15 k x 15 k x 300 and 100 k x 100 k x 128.  Two radii per shape and metric, each the midpoint of the
widest gap among 2 000 sorted values of the k = 100 lists (kz_knn) around the (15 n)-th and the (50 n)-th smallest: about 15 pairs a
row, and about 50, where the allocation policy's first call (32 pairs a row) falls short and BOTH routes pay a second call.  Per radius:
  * `neighbors`  radius_neighbors with the allocation policy, sorted rows;
  * `counts`     radius_counts (capacity 0: the count kernel on the sweep route).
The routes alternate call by call in one process; a pair of HIP events around each call (every call ends with a synchronise of the
context's stream), one warm-up each, the median of five.  The two routes' results are compared byte for byte before anything is timed.
The stats of every native call of the last timed sweep call are part of the row.  Writes a markdown table (`--out`, default
profiles/radius_sweep.md) and one JSON line per row (`--jsonl`, default profiles/radius_sweep.jsonl).

    python tools/radius_sweep_time.py [--out FILE] [--jsonl FILE] [--cases small|large|all|wide|wide_small|wide_large] [--reps 5]
                                      [--per-row 15,50] [--overflow]

`--cases wide`: the text-encoder widths of the wide-row and parity-split sweeps, 15 k x 15 k (`wide_small`) and 100 k x 100 k
(`wide_large`) at d = 768, 1024, 1536 and 2048.  `--overflow` adds, per shape and metric, a radius of about 90 pairs a row: beyond the
sweep's log (64 entries a row, at least 2^20), so route="sweep" pays the sweep AND the exact route.

Under `rocprofv3 --kernel-trace --stats -- python tools/radius_sweep_time.py --out /dev/null --jsonl /dev/null --reps 1` the
per-kernel totals split the sweep route into the emit / count sweep, the two sorts, the resolve, the row kernels and the row sort.
"""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402

CASES = dict(CASES, wide_small=[(15_000, d) for d in (768, 1024, 1536, 2048)], wide_large=[(100_000, d) for d in (768, 1024, 1536, 2048)])
CASES["wide"] = CASES["wide_small"] + CASES["wide_large"]


def alternated_ms(ev, calls, reps):
    """{name: median ms} of the calls, one warm-up each, then `reps` rounds in which the calls follow each other."""
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            times[name].append(ev.ms(fn))
    return {name: statistics.median(t) for name, t in times.items()}


def gap_near(flat, centre, window=2000):
    """The midpoint of the widest gap among the `window` sorted values around place `centre`."""
    lo = max(centre - window // 2, 0)
    gaps = np.diff(flat[lo:lo + window])
    at = int(np.argmax(gaps))
    return float(flat[lo + at] + 0.5 * gaps[at])


def write_table(rows, out):
    def num(v):
        return f"{v:,}".replace(",", " ")
    lines = ["# `radius_neighbors` / `radius_counts`: route=\"sweep\" beside route=\"exact\" (one MI355X, one process)", "",
             "`tools/radius_sweep_time.py`: float32, standard-normal data; routes alternated call by call, a pair of HIP events around each",
             "call, one warm-up, the median of five.  `walks`: native calls of the allocation policy (2: the first call's 32 pairs a row fell",
             "short, on both routes).  `candidates`: log entries of the sweep's last native call; `sweep` / `resolve`: its device times.", "",
             "| shape | metric | pairs a row | walks | neighbors exact | neighbors sweep | counts exact | counts sweep | route taken | candidates "
             "| max err ratio | sweep | resolve |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        s = r["sweep_stats"][-1]
        lines.append(f"| {num(r['n_query'])} × {num(r['n_index'])} × {r['d']} | {r['metric']} | {r['pairs_per_row']:.1f} | {r['policy_walks']} "
                     f"| {r['neighbors_exact_ms']:.2f} ms | {r['neighbors_sweep_ms']:.2f} ms | {r['counts_exact_ms']:.2f} ms "
                     f"| {r['counts_sweep_ms']:.2f} ms | {[c['route_taken'] for c in r['sweep_stats']]} | {num(s['n_candidates'])} "
                     f"| {s['max_err_ratio']:.3f} | {s['sweep_ms']:.2f} ms | {s['resolve_ms']:.2f} ms |")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/radius_sweep.md")
    ap.add_argument("--jsonl", default="profiles/radius_sweep.jsonl")
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-row", type=lambda v: [int(x) for x in v.split(",")], default=[15, 50], help="pairs a row of the radii")
    ap.add_argument("--overflow", action="store_true", help="also a radius whose candidates overflow the sweep's log")
    args = ap.parse_args()
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        for metric in ("euclidean", "cosine"):
            sm, tm = N.DeviceMatrix(ctx, s, metric), N.DeviceMatrix(ctx, t, metric)
            flat = np.sort(N.knn(ctx, sm, tm, 100)[0].numpy(), axis=None)   # (the pairs within a radius that admits 50 a row: in the lists,
            for per_row in args.per_row + ([90] if args.overflow else []):   #  but for hubs with more than 100)
                radius = gap_near(flat, per_row * n)
                stats = {}
                exact = N.radius_neighbors(ctx, sm, tm, radius)
                sweep = N.radius_neighbors(ctx, sm, tm, radius, route="sweep", stats=stats)
                assert exact[3] == sweep[3] and all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(exact[:3], sweep[:3]))
                total = exact[3]
                del exact, sweep
                ms = alternated_ms(ev, {
                    "neighbors_exact": lambda: N.radius_neighbors(ctx, sm, tm, radius),
                    "neighbors_sweep": lambda: N.radius_neighbors(ctx, sm, tm, radius, route="sweep", stats=stats),
                    "counts_exact": lambda: N.radius_counts(ctx, sm, tm, radius),
                    "counts_sweep": lambda: N.radius_counts(ctx, sm, tm, radius, route="sweep")}, args.reps)
                N.radius_neighbors(ctx, sm, tm, radius, route="sweep", stats=stats)
                row = {"n_query": n, "n_index": n, "d": d, "metric": metric, "radius": radius, "pairs": total, "pairs_per_row": total / n,
                       "policy_walks": 1 if total <= N.RADIUS_FIRST_CAPACITY_PER_ROW * n else 2, "sweep_stats": stats["calls"]}
                row.update({name + "_ms": v for name, v in ms.items()})
                print(json.dumps(row), flush=True)
                rows.append(row)
    write_table(rows, args.out)
    with open(args.jsonl, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
