"""Time of braycurtis, seuclidean, correlation and hamming (the VALU route of kz_family_dist_kernel + the exact selection) at
15 k x 15 k x 300 and 100 k x 100 k x 128 in both dtypes, with manhattan beside them, and scikit-learn's brute-force search on the
16 host cores a GPU job may use for the 15 k shape.

    python tools/metric_time.py [nosk]
    rocprofv3 --kernel-trace --stats -d <dir> -o metric -- python tools/metric_time.py nosk     # kernel times (kz_family_dist_kernel)

Wall times are of one kz_knn call after a warm-up call (k = 10)."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402

with_sklearn = not (len(sys.argv) > 1 and sys.argv[1] == "nosk")
ctx = N.Context.get()
rng = np.random.default_rng(0)
for n, d in ((15000, 300), (100000, 128)):
    for dtype in (np.float32, np.float64):
        s = rng.standard_normal((n, d)).astype(dtype)
        t = rng.standard_normal((n, d)).astype(dtype)
        V = rng.uniform(0.5, 2.0, d)
        for metric in ("manhattan", "braycurtis", "seuclidean", "correlation", "hamming"):
            si, ti = (np.round(s), np.round(t)) if metric == "hamming" else (s, t)
            Vm = V if metric == "seuclidean" else None
            sm, tm = N.DeviceMatrix(ctx, si, metric, V=Vm), N.DeviceMatrix(ctx, ti, metric, V=Vm)
            N.knn(ctx, sm, tm, 10)
            ctx.sync()
            t0 = time.perf_counter()
            N.knn(ctx, sm, tm, 10)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            line = f"{n} x {n} x {d} {np.dtype(dtype).name} {metric}: {ms:.1f} ms ({n * n * d / ms / 1e6:.1f} G feature-pairs/s)"
            if with_sklearn and n <= 15000 and metric != "manhattan":
                from sklearn.neighbors import NearestNeighbors
                kw = {"metric_params": {"V": V}} if metric == "seuclidean" else {}
                nn = NearestNeighbors(n_neighbors=10, metric=metric, algorithm="brute", n_jobs=16, **kw).fit(ti)
                t0 = time.perf_counter()
                nn.kneighbors(si)
                line += f"   scikit-learn (16 cores): {(time.perf_counter() - t0) * 1e3:.0f} ms"
            print(line, flush=True)
            del sm, tm
