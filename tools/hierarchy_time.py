"""Time of the single-linkage hierarchy (kz_forest_csr) on the shapes and CSRs of tools/components_time.py:
cosine, CSLS (n_candidates 10), standard-normal float32 data at 15 k x 15 k x 300 and 100 k x 100 k x 128 -- `neighbor_pairs(10,
"mutual")`, `neighbor_pairs(10, "union")` and `radius_neighbors` at about 10 pairs per row, all `reduced=True` -- plus every pair of
4 k x 4 k x 64 (one giant component on few nodes: the case where atomic contention would show), a path of 10^6 nodes with random
weights and one hub row.  Per CSR:
  (a) the forest call beside the components call (labels and sizes) on the same CSR;
  (b) a cut between the two middle distinct forest values beside, for the radius CSRs, `components_radius_device(t)` end to end (join + components) at
      the same t;
  (c) for the radius CSRs a 32-point `cluster_curve` (gold = the identity: the data has no entities, the cost is what is measured)
      beside 32 x the end-to-end figure of (b) -- a product, the 32 joins are not run;
  (d) the rounds the forest took;
  (f) the final sort alone (kz_csr_sort_rows on the forest's (value, entry) in compaction order, ascending entry) and its share.
HIP events around each device call, wall clock for `cluster_curve` (it scores on the host); one warm-up, then the best of three.  One
process.  Prints one JSON line per row; `--out` writes them as a markdown table.

    python tools/hierarchy_time.py [--out FILE] [--cases small|large|all]
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from kiez_amd import evaluate, matching  # noqa: E402
from tools.components_time import K, best_ms  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402


def wall_ms(fn, reps=3):
    fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def measure(ctx, ev, case, pairs, join_at=None):
    """One row: `pairs` the PairList of the CSR with values; `join_at(t)`: the facade's end-to-end components call at threshold t."""
    n_q, n_t = pairs.n_q, pairs.n_target
    row = {"case": case, "rows": n_q, "targets": n_t, "pairs": pairs.n_entries}
    row["components_ms"] = best_ms(ev, lambda: pairs.components(True))
    row["forest_ms"] = best_ms(ev, pairs.forest)
    h = matching._hierarchy_of(pairs)
    row.update(rounds=h.rounds, forest_edges=int(h.value.shape[0]), components=h.n_components)
    if h.value.shape[0]:
        # (f) the sort on its own input: the forest in compaction order
        order = np.argsort(h.entry)
        ptr = ctx.to_device(np.array([0, order.shape[0]], dtype=np.int64))
        host_e, host_v = h.entry[order], h.value[order]

        def sort_once():
            e, v = ctx.to_device(host_e), ctx.to_device(host_v)
            return ev.ms(lambda: N.csr_sort_rows(ctx, ptr, e, v, 2 ** 31 - 2))
        sort_once()
        row["sort_ms"] = min(sort_once() for _ in range(3))
        row["sort_share"] = row["sort_ms"] / row["forest_ms"]
        # between the two middle distinct values: no stored value equals t (a float32-cosine fit stores values rounded to float32
        # AFTER the join's comparison, so a join AT a stored value may leave out the pair that rounded down to it)
        distinct = np.unique(h.value)
        t = float(distinct[distinct.size // 2]) if distinct.size < 2 else 0.5 * float(distinct[distinct.size // 2 - 1] + distinct[distinct.size // 2])
        row["cut_threshold"] = t
        row["cut_ms"] = best_ms(ev, lambda: h.cut_device(t, True))
        row["cut_clusters"] = h.n_clusters(t)
        if join_at is not None:
            row["join_plus_components_ms"] = best_ms(ev, lambda: join_at(t))
            if join_at(t)[2].shape[0] != row["cut_clusters"]:
                raise RuntimeError(f"{case}: the cut and the join disagree at t = {t}")
            gold = np.arange(n_q, dtype=np.int64) % n_t
            row["curve_32_points_ms"] = wall_ms(lambda: evaluate.cluster_curve(h, gold, max_points=32))
            row["32_joins_plus_components_ms"] = 32 * row["join_plus_components_ms"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    args = ap.parse_args()
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(s, t)
        shape = f"{n}x{n}x{d} cosine CSLS"
        for mode in ("mutual", "union"):
            rows.append(measure(ctx, ev, f"{shape} neighbor_pairs({K}, {mode})", kz._pairs_of_both_directions(K, mode, True)))
        radius = float(np.median(kz.kneighbors(K)[0][:, -1]))   # the reduced value of the 10th neighbour of the median row
        rows.append(measure(ctx, ev, f"{shape} radius_neighbors({radius:.4f})", kz._pairs_within_radius(radius, True),
                            lambda t: kz.components_radius_device(t, reduced=True, return_sizes=True)))
        del kz
        ctx.trim()
    # one giant component on few nodes: every pair of 4 k x 4 k
    n = 4000
    s, t = rng.standard_normal((n, 64)).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(s, t)
    rows.append(measure(ctx, ev, "4000x4000x64 radius = inf (one giant component)", kz._pairs_within_radius(np.inf, True)))
    del kz
    ctx.trim()
    # a path s - t - s - t ... of 10^6 nodes, ids shuffled, random weights
    half = 500_000
    perm_s, perm_t = rng.permutation(half), rng.permutation(half)
    src, tgt = np.concatenate([perm_s, perm_s[1:]]), np.concatenate([perm_t, perm_t[:-1]])
    order = np.argsort(src, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=half))]).astype(np.int64)
    rows.append(measure(ctx, ev, "path of 10^6 nodes, shuffled ids, random weights",
                        N.PairList.csr(ctx, ctx.to_device(indptr), ctx.to_device(tgt[order].astype(np.int64)), ctx.to_device(rng.random(src.shape[0])),
                                       half)))
    # one hub row that every target is in, in front of 100 000 rows of one random target each
    n = 100_000
    indptr = np.concatenate([[0], n + np.arange(n + 1)]).astype(np.int64)
    ind = np.concatenate([np.arange(n), rng.integers(0, n, n)]).astype(np.int64)
    rows.append(measure(ctx, ev, "hub row of 100 000 targets + 100 000 rows of one",
                        N.PairList.csr(ctx, ctx.to_device(indptr), ctx.to_device(ind), ctx.to_device(rng.random(ind.shape[0])), n)))
    if args.out:
        keys = sorted({k for r in rows for k in r if k != "case"}, key=lambda k: max(list(r).index(k) if k in r else -1 for r in rows))
        with open(args.out, "w") as f:
            f.write("| case | " + " | ".join(keys) + " |\n|" + "---|" * (len(keys) + 1) + "\n")
            for r in rows:
                cells = [f"{r[k]:.3f}" if isinstance(r.get(k), float) else str(r.get(k, "")) for k in keys]
                f.write(f"| {r['case']} | " + " | ".join(cells) + " |\n")


if __name__ == "__main__":
    main()
