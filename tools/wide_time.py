"""GPU box: wide rows (d = 512 .. 1024; --widths 1024,1536,2048 for the parity-split builds) on the fp16 first pass against
float32 operands, same process, alternated.
   python3 tools/wide_time.py [--reps R] [--widths D,D,...] [--data uniform|gmm] [--big | --only-big] [--big-d D]
Per shape and precision (0 = fp16 pass, 1 = float32 operands): the step time (median of R), the main kernel's time
(main_kernel_ms, summed over both directions of a fit), its fraction of the dense fp16 peak (2 n_q n_i d / time / 2.5 PF) and
n_first_pass_fail; every step's result is checked against the oracle on a seeded row sample, and the two precisions against each
other (CSLS: bit for bit against the float32-operand run only).  One JSON line per shape."""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PEAK_FP16 = 2.5e15


DATA = "uniform"


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    if DATA == "uniform":
        return rng.random((n, d), dtype=np.float32)
    # L2-normalised mixture of 64 clusters (the `_gmm` rows of tests/test_gpu_wide_dims.py)
    centres = np.random.default_rng(6).standard_normal((64, d), dtype=np.float32)
    x = centres[rng.integers(0, 64, n)]
    x += np.float32(0.35) * rng.standard_normal((n, d), dtype=np.float32)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x


def _oracle_check(q, y, ind, k, rows):
    from oracle import kiez_oracle as O
    _, oi = O.knn_exact(q[rows], y, k, "euclidean")
    return bool(np.array_equal(ind[rows], oi))


def ordinary(ctx, n_q, n_i, d, reps, k=10):
    from kiez_amd import _native as N
    q, y = _data(n_q, d, 1), _data(n_i, d, 2)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    rows = np.random.default_rng(3).choice(n_q, 64, replace=False)
    res = {0: [], 1: []}
    out = {}
    for _ in range(reps + 1):   # (the first round warms both up and is not counted)
        for prec in (0, 1):
            ctx.set_option("precision", prec)
            ctx.sync()
            t0 = time.perf_counter()
            dd, ii, st = N.knn(ctx, qm, ym, k)
            ctx.sync()
            res[prec].append((time.perf_counter() - t0, st))
            out[prec] = (dd.numpy(), ii.numpy())
    ctx.set_option("precision", 0)
    same = bool(np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]))
    return _report("knn", n_q, n_i, d, k, res, same, _oracle_check(q, y, out[0][1], k, rows), 1)


def csls(ctx, n_s, n_t, d, reps, k=10):
    from kiez_amd import Kiez
    s, t = _data(n_s, d, 4), _data(n_t, d, 5)
    res = {0: [], 1: []}
    out = {}
    for _ in range(reps + 1):
        for prec in (0, 1):
            ctx.set_option("precision", prec)
            ctx.sync()
            t0 = time.perf_counter()
            kz = Kiez(n_candidates=k, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
            kz.fit(s, t)
            dd, ii = kz.kneighbors(k)
            ctx.sync()
            a = kz.algorithm
            st = dict(a.last_stats)
            rev = getattr(a, "last_stats_reverse", None) or {}
            st["main_kernel_ms"] = st.get("main_kernel_ms", 0.0) + (rev.get("main_kernel_ms", 0.0) if st.get("dual") != 1 else 0.0)
            res[prec].append((time.perf_counter() - t0, st))
            out[prec] = (dd, ii)
    ctx.set_option("precision", 0)
    same = bool(np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]))
    # (the oracle's CSLS needs both full neighbour matrices in float64 numpy -- hours at these shapes: the fp16 run is checked
    #  against the float32-operand run bit for bit instead, and the ordinary searches above against the oracle)
    return _report("csls_fit_kneighbors", n_s, n_t, d, k, res, same, None, 2)


def _report(kind, n_q, n_i, d, k, res, same, oracle_ok, directions):
    line = {"kind": kind, "data": DATA, "n_q": n_q, "n_i": n_i, "d": d, "k": k, "same_bits": same, "oracle_sample_ok": oracle_ok}
    for prec, name in ((0, "fp16"), (1, "f32")):
        runs = res[prec][1:]
        # (the shared sweep computes each distance once for both directions)
        flops = 2.0 * n_q * n_i * d * (1 if runs[-1][1].get("dual") == 1 else directions)
        step = float(np.median([r[0] for r in runs])) * 1e3
        main = float(np.median([r[1].get("main_kernel_ms", 0.0) for r in runs]))
        line[name] = {"step_ms": round(step, 2), "main_kernel_ms": round(main, 2),
                      "fp16_peak_fraction": round(flops / (main * 1e-3) / PEAK_FP16, 3) if main > 0 else None,
                      "n_first_pass_fail": int(runs[-1][1].get("n_first_pass_fail", 0)),
                      "n_escalated_rows": int(runs[-1][1].get("n_escalated_rows", 0)),
                      "n_fallback_rows": int(runs[-1][1].get("n_fallback_rows", 0)), "first_pass": int(runs[-1][1].get("first_pass", -1)),
                      "dual": int(runs[-1][1].get("dual", 0))}
    line["speedup_step"] = round(line["f32"]["step_ms"] / line["fp16"]["step_ms"], 2)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--widths", default="512,768,1024", help="feature counts of the 100k x 100k shapes")
    ap.add_argument("--data", default="uniform", choices=["uniform", "gmm"])
    ap.add_argument("--big", action="store_true", help="also 250k x 1M CSLS at --big-d")
    ap.add_argument("--only-big", action="store_true")
    ap.add_argument("--big-d", type=int, default=768)
    args = ap.parse_args()
    global DATA
    DATA = args.data
    widths = [int(w) for w in args.widths.split(",")]
    warnings.simplefilter("ignore")
    from kiez_amd import _native as N
    ctx = N.Context.get()
    if not args.only_big:
        for d in widths:
            ordinary(ctx, 100_000, 100_000, d, args.reps)
        for d in widths:
            csls(ctx, 100_000, 100_000, d, args.reps)
    if args.big or args.only_big:
        csls(ctx, 250_000, 1_000_000, args.big_d, 1)


if __name__ == "__main__":
    main()
