"""Time of `neighbor_pairs(10, mode="union", reduced=True)` split into its stages -- the two searches, the set step
(kz_lists_combine), the values (kz_pairs_values) and the row sort (kz_csr_sort_rows) -- beside `kneighbors(10)`, and of ten Sinkhorn
iterations on the union support (kz_sinkhorn_csr) beside the same on the forward candidate lists (kz_sinkhorn_lists).  Cosine, CSLS
(n_candidates 10), standard-normal float32 data at 15 k x 15 k x 300 and 100 k x 100 k x 128.
A pair of HIP events around each call (every call ends with a synchronise of the context's stream), one warm-up, then `--reps`
repeats: the median, the smallest and the largest are printed.  One process.  Prints one JSON line per shape; `--out` writes them
as a markdown table.

    python tools/neighbor_pairs_time.py [--out FILE] [--cases small|large|all] [--reps 5]
"""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402

K = 10


def spread_ms(ev, fn, reps, before=None):
    """(median, min, max) of `reps` timed calls behind one warm-up; `before` runs untimed in front of every call."""
    times = []
    for i in range(reps + 1):
        if before is not None:
            before()
        t = ev.ms(fn)
        if i:
            times.append(t)
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    reps = max(args.reps, 3)
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(s, t)
        nn, hub = kz.algorithm, kz.hubness
        sm, tm = nn.source_index, nn.target_index
        kind, q_state, t_state = hub._forward_rank_state()
        row = {"case": f"{n}x{n}x{d} cosine CSLS k={K} union reduced"}
        # the searches: two separate ones, and the one sweep that serves both where it applies
        row["search_forward_ms"] = spread_ms(ev, lambda: N.knn(ctx, sm, tm, K), reps)
        row["search_reverse_ms"] = spread_ms(ev, lambda: N.knn(ctx, tm, sm, K), reps)
        row["search_both_one_sweep_ms"] = spread_ms(ev, lambda: N.knn_dual(ctx, sm, tm, K), reps)
        fwd_d, fwd_i, _ = N.knn(ctx, sm, tm, K)
        _, rev_i, _ = N.knn(ctx, tm, sm, K)
        # the stages behind the searches
        row["combine_ms"] = spread_ms(ev, lambda: N.lists_combine(ctx, fwd_i, rev_i, "union"), reps)
        indptr, ind, total = N.lists_combine(ctx, fwd_i, rev_i, "union")
        lens = np.diff(indptr.numpy())
        row.update(pairs=int(total), pairs_per_row=float(lens.mean()), longest_row=int(lens.max()), empty_rows=int((lens == 0).sum()),
                   mutual_pairs=int(N.lists_combine(ctx, fwd_i, rev_i, "mutual", capacity=0)[2]))
        row["values_ms"] = spread_ms(ev, lambda: N.pairs_values(ctx, sm, tm, indptr, ind, kind, q_state, t_state), reps)
        row["values_plain_ms"] = spread_ms(ev, lambda: N.pairs_values(ctx, sm, tm, indptr, ind), reps)
        val = N.pairs_values(ctx, sm, tm, indptr, ind, kind, q_state, t_state)
        s_ind, s_val = ctx.empty(ind.shape, np.int64), ctx.empty(val.shape, np.float64)

        def unsorted():
            s_ind.copy_from(ind)
            s_val.copy_from(val)
        row["sort_ms"] = spread_ms(ev, lambda: N.csr_sort_rows(ctx, indptr, s_ind, s_val, n), reps, before=unsorted)
        # the calls as a user makes them
        row["neighbor_pairs_ms"] = spread_ms(ev, lambda: kz.neighbor_pairs_device(K, mode="union", reduced=True), reps)
        row["neighbor_pairs_mutual_ms"] = spread_ms(ev, lambda: kz.neighbor_pairs_device(K, mode="mutual", reduced=True), reps)
        row["kneighbors_ms"] = spread_ms(ev, lambda: nn.kneighbors_device(K), reps)
        row["match_pairs_ms"] = spread_ms(ev, lambda: kz.match_pairs_device(K, mode="union", reduced=True), reps)
        # ten Sinkhorn iterations: the union's plain values beside the forward candidate lists
        plain = N.pairs_values(ctx, sm, tm, indptr, ind)
        row["sinkhorn_union_ms"] = spread_ms(ev, lambda: N.sinkhorn_csr(ctx, indptr, ind, plain, n, 0.05, 10), reps)
        row["sinkhorn_candidates_ms"] = spread_ms(ev, lambda: N.sinkhorn_lists(ctx, fwd_d, fwd_i, n, 0.05, 10), reps)
        g = N.sinkhorn_csr(ctx, indptr, ind, plain, n, 0.05, 10)[1].numpy()
        g_c = N.sinkhorn_lists(ctx, fwd_d, fwd_i, n, 0.05, 10)[1].numpy()
        row.update(targets_without_potential_union=int(np.isnan(g).sum()), targets_without_potential_candidates=int(np.isnan(g_c).sum()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        keys = [k for k in rows[0] if k != "case"]
        with open(args.out, "w") as f:
            f.write("| figure | " + " | ".join(r["case"] for r in rows) + " |\n|" + "---|" * (len(rows) + 1) + "\n")
            for k in keys:
                cells = []
                for r in rows:
                    v = r.get(k, "")
                    cells.append(f"{v['median']:.3f} ms ({v['min']:.3f} .. {v['max']:.3f})" if isinstance(v, dict) else
                                 f"{v:.2f}" if isinstance(v, float) else str(v))
                f.write(f"| {k} | " + " | ".join(cells) + " |\n")


if __name__ == "__main__":
    main()
