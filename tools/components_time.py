"""Time of the components step (kz_components_csr, labels and sizes) beside the call that produces its CSR and beside
`scipy.sparse.csgraph.connected_components` on the same CSR on the host (the reference figure: the CSR is already on the host there,
the copy is not counted).  Cosine, CSLS (n_candidates 10), standard-normal float32 data at 15 k x 15 k x 300 and 100 k x 100 k x 128:
`neighbor_pairs(10, "mutual")`, `neighbor_pairs(10, "union")` and `radius_neighbors` at a radius of about 10 pairs per row, all
`reduced=True`.  Three synthetic rows: one giant component (radius = inf on 4 k x 4 k x 64), a path of 10^6 nodes with shuffled ids,
one hub row that every target is in.
A pair of HIP events around each device call (every call ends with a synchronise of the context's stream), one warm-up, then the best
of three.  One process.  Prints one JSON line per row; `--out` writes them as a markdown table.

    python tools/components_time.py [--out FILE] [--cases small|large|all]
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from tools.whole_index_time import CASES, Events  # noqa: E402

K = 10


def best_ms(ev, fn, reps=3):
    fn()   # warm-up: code objects, the pool's buffers
    return min(ev.ms(fn) for _ in range(reps))


def scipy_ms(indptr, ind, n_t, reps=3):
    """(best of `reps` in ms, number of components) of scipy's connected_components on A = [[0, B], [B.T, 0]]; building A is not timed."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n_q = indptr.shape[0] - 1
    ok = (ind >= 0) & (ind < n_t)
    rows = np.repeat(np.arange(n_q, dtype=np.int64), np.diff(indptr))[ok]
    B = sp.csr_matrix((np.ones(rows.shape[0], dtype=np.int8), (rows, ind[ok])), shape=(n_q, n_t))
    A = sp.bmat([[None, B], [B.T, None]], format="csr")
    best, c = float("inf"), 0
    for _ in range(reps):
        t0 = time.perf_counter()
        c, _ = connected_components(A, directed=False)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, int(c)


def measure(ctx, ev, case, indptr, ind, n_t, produce=None):
    """One row of the table: `indptr`, `ind` DeviceArrays of the CSR, `produce` the call that makes it (None: a synthetic CSR)."""
    row = {"case": case, "rows": indptr.shape[0] - 1, "targets": n_t, "pairs": ind.shape[0]}
    if produce is not None:
        row["producing_call_ms"] = best_ms(ev, produce)
    row["components_ms"] = best_ms(ev, lambda: N.components_csr(ctx, indptr, ind, n_t, sizes=True))
    row["components_labels_only_ms"] = best_ms(ev, lambda: N.components_csr(ctx, indptr, ind, n_t))
    _, _, size_q, size_t, c = N.components_csr(ctx, indptr, ind, n_t, sizes=True)
    sizes = size_q.numpy() + size_t.numpy()
    row.update(components=c, largest=int(sizes.max()), singletons=int((sizes == 1).sum()),
               one_to_one=int(((size_q.numpy() == 1) & (size_t.numpy() == 1)).sum()))
    row["scipy_host_ms"], c_ref = scipy_ms(indptr.numpy(), ind.numpy(), n_t)
    if c_ref != c:
        raise RuntimeError(f"{case}: {c} components on the device, {c_ref} from scipy")
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
            indptr, ind = kz.neighbor_pairs_device(K, mode=mode, reduced=True, return_distance=False)
            rows.append(measure(ctx, ev, f"{shape} neighbor_pairs({K}, {mode})", indptr, ind, n,
                                lambda: kz.neighbor_pairs_device(K, mode=mode, reduced=True)))
        radius = float(np.median(kz.kneighbors(K)[0][:, -1]))   # the reduced value of the 10th neighbour of the median row
        indptr, ind, _ = kz._pairs_within_radius(radius, True)[:3]
        rows.append(measure(ctx, ev, f"{shape} radius_neighbors({radius:.4f})", indptr, ind, n, lambda: kz._pairs_within_radius(radius, True)))
        del kz
        ctx.trim()
    # one giant component: every pair of 4 k x 4 k
    n = 4000
    s, t = rng.standard_normal((n, 64)).astype(np.float32), rng.standard_normal((n, 64)).astype(np.float32)
    kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(s, t)
    indptr, ind, _ = kz._pairs_within_radius(np.inf, True)[:3]
    rows.append(measure(ctx, ev, "4000x4000x64 radius = inf (one giant component)", indptr, ind, n, lambda: kz._pairs_within_radius(np.inf, True)))
    del kz, indptr, ind
    ctx.trim()
    # a path s - t - s - t ... of 10^6 nodes, source and target ids shuffled independently
    half = 500_000
    perm_s, perm_t = rng.permutation(half), rng.permutation(half)
    src, tgt = np.concatenate([perm_s, perm_s[1:]]), np.concatenate([perm_t, perm_t[:-1]])
    order = np.argsort(src, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=half))]).astype(np.int64)
    rows.append(measure(ctx, ev, "path of 10^6 nodes, shuffled ids", ctx.to_device(indptr), ctx.to_device(tgt[order].astype(np.int64)), half))
    # one hub row that every target is in, in front of 100 000 rows of one random target each
    n = 100_000
    indptr = np.concatenate([[0], n + np.arange(n + 1)]).astype(np.int64)
    ind = np.concatenate([np.arange(n), rng.integers(0, n, n)]).astype(np.int64)
    rows.append(measure(ctx, ev, "hub row of 100 000 targets + 100 000 rows of one", ctx.to_device(indptr), ctx.to_device(ind), n))
    if args.out:
        keys = [k for k in rows[0] if k != "case"]
        with open(args.out, "w") as f:
            f.write("| case | " + " | ".join(keys) + " |\n|" + "---|" * (len(keys) + 1) + "\n")
            for r in rows:
                cells = [f"{r[k]:.3f}" if isinstance(r.get(k), float) else str(r.get(k, "")) for k in keys]
                f.write(f"| {r['case']} | " + " | ".join(cells) + " |\n")


if __name__ == "__main__":
    main()
