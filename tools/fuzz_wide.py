"""GPU box: randomised shapes at 32 .. 64 slices (d = 497 .. 1024) -- the fp16 kernel's wide-row builds -- or, with a width range,
at 65 .. 128 slices (d = 1025 .. 2048: the parity-split builds).  Per case: the shared sweep (kz_knn_dual, forced) against two
kz_knn calls, bit for bit, and a row sample of both directions against the oracle.
   python3 tools/fuzz_wide.py [n_cases] [seed] [max_rows] [d_lo d_hi [k_max]]
A case is bad when the bits differ, the oracle disagrees or the first pass was not the fp16 one.  The shared sweep may still
decline a forced case for reasons other than the width (too few sample rows for lists of 128: k > 54 on small inputs); those
cases compare two pairs of ordinary searches, and the count of cases that did share the sweep is printed.
Prints one line per case and the count of bad cases; tests/test_gpu_wide_dims.py runs a fixed-seed slice of it (run())."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _case(rng, max_rows, d_lo=497, d_hi=1024, k_max=64, d_force=None):
    """(the draws are the same whatever the width range: d_force swaps the width of a case and keeps its rows, k and metric)"""
    na = int(rng.integers(1100, max_rows + 1))
    nb = int(rng.integers(1100, max_rows + 1))
    d = int(rng.integers(d_lo, d_hi + 1))
    if d_force:
        d = d_force
    k = int(rng.choice([k for k in (1, 2, 5, 10, 13, 27, 50, 64) if k <= k_max]))
    metric = str(rng.choice(["euclidean", "sqeuclidean", "cosine"]))
    dtype = np.float32 if rng.random() < 0.7 else np.float64
    kind = str(rng.choice(["uniform", "normal", "clustered", "dups"]))

    def gen(n):
        if kind == "uniform":
            return rng.random((n, d))
        if kind == "normal":
            return rng.standard_normal((n, d))
        if kind == "clustered":
            c = rng.standard_normal((6, d)) * 4
            return c[rng.integers(0, 6, n)] + 0.3 * rng.standard_normal((n, d)) * rng.random((n, 1)) * 3
        base = rng.random((max(n // 5, 4), d))
        return base[rng.integers(0, len(base), n)]

    return gen(na).astype(dtype), gen(nb).astype(dtype), d, k, metric, kind


def _oracle_rows_ok(q, y, dd, ii, k, metric, rows):
    """Every sampled row: the distances of the returned rows are the oracle's k smallest (ties may swap indices)."""
    from oracle import kiez_oracle as O
    q64, y64 = (q.astype(np.float64), y.astype(np.float64)) if metric == "cosine" else (q, y)
    od, oi = O.knn_exact(q64[rows], y64, k, metric)
    if np.array_equal(ii[rows], oi):
        return True
    return bool(np.allclose(dd[rows], od, rtol=1e-12, atol=0))


def run(seed=1, n_cases=20, max_rows=6000, verbose=False, d_lo=497, d_hi=1024, k_max=64, d_force=None):
    """Returns (the list of bad cases -- empty: all good --, the number of cases that ran the shared sweep)."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(seed)
    bad = []
    n_dual = 0
    for case in range(n_cases):
        a, b, d, k, metric, kind = _case(rng, max_rows, d_lo, d_hi, k_max, d_force)
        am, bm = N.DeviceMatrix(ctx, a, metric), N.DeviceMatrix(ctx, b, metric)
        try:
            ctx.set_option("dual_force", 0)
            d_ab, i_ab, s1 = N.knn(ctx, am, bm, k)
            d_ba, i_ba, _ = N.knn(ctx, bm, am, k)
            ctx.set_option("dual_force", 1)
            (xd, xi, s_ab), (yd, yi, _) = N.knn_dual(ctx, am, bm, k)
        finally:
            ctx.set_option("dual_force", 0)
        two = [x.numpy() for x in (d_ab, i_ab, d_ba, i_ba)]
        one = [x.numpy() for x in (xd, xi, yd, yi)]
        same = all(np.array_equal(u, v) for u, v in zip(two, one))
        ra = rng.choice(len(a), min(64, len(a)), replace=False)
        rb = rng.choice(len(b), min(64, len(b)), replace=False)
        orc = _oracle_rows_ok(a, b, two[0], two[1], k, metric, ra) and _oracle_rows_ok(b, a, two[2], two[3], k, metric, rb)
        ok = same and orc and s1["first_pass"] == 2
        n_dual += s_ab["dual"] == 1
        line = (f"case {case}: {len(a)} x {len(b)} x {d} k={k} {metric} {a.dtype} {kind} first_pass={s1['first_pass']} "
                f"dual={s_ab['dual']} same_bits={same} oracle={orc} -> {'ok' if ok else 'BAD'}")
        if verbose:
            print(line, flush=True)
        if not ok:
            bad.append(line)
    return bad, n_dual


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    max_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 6000
    d_lo, d_hi = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (497, 1024)
    k_max = int(sys.argv[6]) if len(sys.argv) > 6 else 64
    bad, n_dual = run(seed, n, max_rows, verbose=True, d_lo=d_lo, d_hi=d_hi, k_max=k_max)
    print(f"fuzz_wide: {n} cases, {n_dual} through the shared sweep, {len(bad)} bad")
    sys.exit(1 if bad else 0)
