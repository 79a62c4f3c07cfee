#!/usr/bin/env python
"""fit + kneighbors through the facade with and without `hubness_kwargs={"native_fit": True}` (kz_fit / kz_kneighbors against the
pipeline of primitives driven from Python), on inputs resident in HBM as DeviceArrays, result left on the device.

One step = Kiez.fit(source, target) + Kiez.kneighbors_device(k), timed by a host clock around a context synchronise.  The two
variants ALTERNATE inside one process after a warm-up of both, so that drift of the machine hits both alike; the report gives the
median, the minimum and the spread (interquartile range) of each and checks that both return the same bytes.

    python tools/native_fit_time.py --shape ea15k --steps 40 --warmup 5
    python tools/native_fit_time.py --ns 100000 --nt 100000 --d 128 --k 10 --hubness CSLS
    python tools/native_fit_time.py --shape ea15k --only native --steps 20      # one variant alone: the run to profile

Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = {"ea15k": (15000, 15000, 300), "c2": (100000, 100000, 128)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES), help="a named shape (ns, nt, d); overrides --ns / --nt / --d")
    ap.add_argument("--ns", type=int, default=15000)
    ap.add_argument("--nt", type=int, default=15000)
    ap.add_argument("--d", type=int, default=300)
    ap.add_argument("--n-candidates", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--hubness", default="CSLS")
    ap.add_argument("--method", default=None, help="LocalScaling / MutualProximity method")
    ap.add_argument("--metric", default="euclidean")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["default", "native"], default=None, help="run one variant alone (for a profiler)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.shape:
        args.ns, args.nt, args.d = SHAPES[args.shape]

    from kiez_amd import Kiez
    from kiez_amd import _native as N

    ctx = N.Context.get()
    rng = np.random.RandomState(args.seed)
    source = ctx.to_device(rng.rand(args.ns, args.d).astype(np.float32))
    target = ctx.to_device(rng.rand(args.nt, args.d).astype(np.float32))

    def make(native):
        kw = {"method": args.method} if args.method else {}
        if native:
            kw["native_fit"] = True
        return Kiez(n_candidates=args.n_candidates, algorithm="SklearnNN", algorithm_kwargs={"metric": args.metric}, hubness=args.hubness,
                    hubness_kwargs=kw)

    variants = {"default": make(False), "native": make(True)}
    if args.only:
        variants = {args.only: variants[args.only]}

    def step(kz):
        ctx.sync()
        t0 = time.perf_counter()
        kz.fit(source, target)
        out = kz.kneighbors_device(args.k)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    results = {}
    for _ in range(args.warmup):
        for name, kz in variants.items():
            _, out = step(kz)
            results[name] = tuple(a.numpy() for a in out)
    same = None
    if len(results) == 2:
        same = all(a.tobytes() == b.tobytes() for a, b in zip(results["default"], results["native"]))
    if "native" in variants and variants["native"].hubness._fitted is None:
        raise SystemExit("the native fit did not run (the plan refused this configuration)")
    times = {name: [] for name in variants}
    for _ in range(args.steps):
        for name, kz in variants.items():   # alternated: one step of each, in turn
            ms, _ = step(kz)
            times[name].append(ms)

    def summary(v):
        v = np.asarray(v)
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        return {"median_ms": round(float(med), 4), "min_ms": round(float(v.min()), 4), "iqr_ms": round(float(q3 - q1), 4), "steps": int(v.size)}

    out = {"tool": "native_fit_time", "ns": args.ns, "nt": args.nt, "d": args.d, "n_candidates": args.n_candidates, "k": args.k,
           "hubness": args.hubness, "method": args.method, "metric": args.metric, "warmup": args.warmup, "same_bytes": same}
    for name, v in times.items():
        out[name] = summary(v)
    if len(times) == 2:
        out["native_minus_default_median_ms"] = round(out["native"]["median_ms"] - out["default"]["median_ms"], 4)
    if "native" in variants:
        info = variants["native"].hubness._fitted.info
        out["plan"] = {k: info[k] for k in ("search", "larger_first", "tail", "fused", "n_searches")}
        out["plan"]["dual"] = info["stats_forward"]["dual"]
    print(json.dumps(out))
    return 0 if same in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
