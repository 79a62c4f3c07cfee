"""Time of the one-to-one, assignment and Sinkhorn steps on a CSR pair list (kz_match_csr, kz_assign_csr, kz_sinkhorn_csr) beside
the fixed-width calls on the SAME pairs padded to the longest row (kz_match_lists, kz_assign_lists, kz_sinkhorn_lists; only where
the longest row has at most 4 096 entries).  Cosine, CSLS (n_candidates 10), standard-normal float32 data at 15 k x 15 k x 300 and
100 k x 100 k x 128.  The radius is found by bisection on the totals of `radius_counts` (the reduced distances), for about 32 pairs
a row; the pairs come from `radius_neighbors_device` and never leave HBM.  Per shape:
  * `match`     the stable matching;
  * `assign`    the auction with unmatched_cost 0.7 into the range of the listed values (the short-run setting of
                profiles/assignment.md) and the default eps;
  * `sinkhorn`  ten iterations at temperature 0.05.
A hub-heavy synthetic case follows (`--hubs`): 30 entries a row, and 1 % of the rows with 10 240 -- run it once with the library as
built and once with a library built with -DKZ_CSR_LONG_ROW=2147483647 (KIEZ_AMD_LIB=path), which has no wave bid; its auction runs
at eps = the value range / 1000 with at most 200 000 rounds (uniform random values are a contested auction).
A pair of HIP events around each call (every call ends with a synchronise of the context's stream), one warm-up, the best of three,
one process.  Prints one JSON line per row; `--out` writes them as a markdown table.

    python tools/csr_lists_time.py [--out FILE] [--cases small|large|all] [--hubs]
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402

PAIRS_PER_ROW = 32


def best_ms(ev, fn, reps=3):
    fn()   # warm-up: code objects, the pool's buffers
    return min(ev.ms(fn) for _ in range(reps))


def radius_for(kz, n, per_row=PAIRS_PER_ROW, steps=14):
    """The radius whose total of `radius_counts(reduced=True)` is nearest per_row n, by bisection between the smallest and the
    largest value of the 64-neighbour whole-index lists."""
    w, _ = kz.kneighbors_whole_index(64)
    lo, hi = float(np.nanmin(w)), float(np.nanmax(w))
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if int(kz.radius_counts(mid, reduced=True).sum()) < per_row * n:
            lo = mid
        else:
            hi = mid
    return hi


def padded(ctx, indptr, ind, dist):
    """The pairs as [n_q, longest row] lists on the device (-1 / NaN behind a row), or None where a row is beyond 4 096."""
    h_ptr = indptr.numpy()
    lens = np.diff(h_ptr)
    width = max(int(lens.max()), 1)
    if width > 4096:
        return None
    n_q = lens.size
    p_ind = np.full((n_q, width), -1, dtype=np.int64)
    p_dist = np.full((n_q, width), np.nan, dtype=dist.dtype)
    rows = np.repeat(np.arange(n_q), lens)
    cols = np.arange(int(h_ptr[-1])) - np.repeat(h_ptr[:-1], lens)
    p_ind[rows, cols] = ind.numpy()
    p_dist[rows, cols] = dist.numpy()
    return ctx.to_device(p_dist), ctx.to_device(p_ind)


def time_case(ctx, ev, name, indptr, ind, dist, n_index, eps_share=None, max_rounds=10_000_000):
    """eps_share None: the default eps, the value range / (1000 n_q); else the value range * eps_share."""
    lens = np.diff(indptr.numpy())
    lo, hi = N.assign_range_csr(ctx, indptr, ind, dist, n_index)
    u = lo + 0.7 * (hi - lo)
    eps = (hi - lo) / (1000.0 * lens.size) if eps_share is None else (hi - lo) * eps_share
    dist64 = ctx.to_device(dist.numpy().astype(np.float64))
    row = {"case": name, "n_q": int(lens.size), "n_index": int(n_index), "pairs": int(lens.sum()), "pairs_per_row": float(lens.mean()),
           "longest_row": int(lens.max()), "rows_above_long_row": int((lens > N.CSR_LONG_ROW).sum())}
    row["match_csr_ms"] = best_ms(ev, lambda: N.match_csr(ctx, indptr, ind, dist, n_index))
    row["assign_csr_ms"] = best_ms(ev, lambda: N.assign_csr(ctx, indptr, ind, dist, n_index, u, eps, max_rounds))
    row["assign_rounds"] = N.assign_csr(ctx, indptr, ind, dist, n_index, u, eps, max_rounds)[3]
    row["sinkhorn_csr_ms"] = best_ms(ev, lambda: N.sinkhorn_csr(ctx, indptr, ind, dist64, n_index, 0.05, 10))
    lists = padded(ctx, indptr, ind, dist)
    if lists is not None:
        p_dist, p_ind = lists
        p_dist64 = ctx.to_device(p_dist.numpy().astype(np.float64))
        row["padded_entries"] = int(p_ind.shape[0] * p_ind.shape[1])
        row["match_lists_ms"] = best_ms(ev, lambda: N.match_lists(ctx, p_dist, p_ind, n_index))
        row["assign_lists_ms"] = best_ms(ev, lambda: N.assign_lists(ctx, p_dist, p_ind, n_index, u, eps, max_rounds))
        row["sinkhorn_lists_ms"] = best_ms(ev, lambda: N.sinkhorn_lists(ctx, p_dist64, p_ind, n_index, 0.05, 10))
        a = N.assign_csr(ctx, indptr, ind, dist, n_index, u, eps, max_rounds)
        b = N.assign_lists(ctx, p_dist, p_ind, n_index, u, eps, max_rounds)
        assert (a[0].numpy() == b[0].numpy()).all() and a[3] == b[3], "the CSR and the padded auction disagree"
    row["assign_eps"], row["assign_converged"] = eps, bool(N.assign_csr(ctx, indptr, ind, dist, n_index, u, eps, max_rounds)[4])
    return row


def hub_case(ctx, rng, n_q=100_000, n_index=100_000, short=30, long=10_240):
    lens = np.full(n_q, short, dtype=np.int64)
    lens[rng.choice(n_q, n_q // 100, replace=False)] = long
    indptr = np.zeros(n_q + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    ind = rng.integers(0, n_index, size=int(indptr[-1])).astype(np.int64)
    dist = rng.random(ind.size).astype(np.float32)
    order = np.lexsort((dist, np.repeat(np.arange(n_q), lens)))   # every row ascending by value
    return ctx.to_device(indptr), ctx.to_device(ind[order]), ctx.to_device(dist[order])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--hubs", action="store_true", help="the hub-heavy synthetic case as well")
    args = ap.parse_args()
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    rows = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS")
        kz.fit(s, t)
        radius = radius_for(kz, n)
        indptr, ind, dist = kz.hubness.radius_neighbors_device(radius, sort_results=True)
        row = time_case(ctx, ev, f"{n}x{n}x{d} cosine CSLS", indptr, ind, dist, n)
        row["radius"] = radius
        row["facade_match_ms"] = best_ms(ev, lambda: kz.match_radius_device(radius, reduced=True))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.hubs:
        indptr, ind, dist = hub_case(ctx, rng)
        # (uniform random values are a contested auction: a coarse eps and a round limit keep the run to seconds)
        row = time_case(ctx, ev, "hubs 100000x100000, 1 % rows of 10240", indptr, ind, dist, 100_000, eps_share=1e-3, max_rounds=200_000)
        row["library"] = str(N.library_path())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        keys = sorted({k for r in rows for k in r if k != "case"})
        with open(args.out, "w") as f:
            f.write("| case | " + " | ".join(keys) + " |\n|" + "---|" * (len(keys) + 1) + "\n")
            for r in rows:
                f.write(f"| {r['case']} | " + " | ".join(f"{r[k]:.3f}" if isinstance(r.get(k), float) else str(r.get(k, "")) for k in keys) + " |\n")


if __name__ == "__main__":
    main()
