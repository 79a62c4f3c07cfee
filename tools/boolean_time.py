"""Time of the boolean metrics (bit-packed rows, kz_bool_dist_kernel + the exact selection) against hamming -- the count-per-feature
metric on float tiles (kz_family_dist_kernel) -- on the same 0/1 data: 15 k x 15 k x 300, 100 k x 100 k x 128 and
100 k x 100 k x 1024, float32, k = 10.

    python tools/boolean_time.py [out.jsonl] [shape=0|1|2]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/boolean_time.py shape=1
                              # kernel times of one shape: kz_bool_dist_kernel, kz_family_dist_kernel, kz_exact_chunk_kernel / kz_exact_select_kernel

Per shape the metrics alternate in one process: a warm-up call each, then ROUNDS timed calls each in turn, every one ended by a
synchronise; the line reports the median and the minimum.  One JSON line per shape and metric (appended to out.jsonl if given).
`shape=i`: that shape only."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402

ROUNDS = 3
args = sys.argv[1:]
only = next((int(a[6:]) for a in args if a.startswith("shape=")), None)
out = next((a for a in args if not a.startswith("shape=")), None)
ctx = N.Context.get()
rng = np.random.default_rng(0)
for shape, (n, d) in enumerate(((15000, 300), (100000, 128), (100000, 1024))):
    if only is not None and shape != only:
        continue
    s = (rng.random((n, d), dtype=np.float32) < 0.5).astype(np.float32)
    t = (rng.random((n, d), dtype=np.float32) < 0.5).astype(np.float32)
    metrics = ("hamming", "jaccard", "russellrao", "yule")
    mats, ms = {}, {m: [] for m in metrics}
    for m in metrics:
        t0 = time.perf_counter()
        mats[m] = (N.DeviceMatrix(ctx, s, m), N.DeviceMatrix(ctx, t, m))
        ctx.sync()
        ms[m + "_create"] = (time.perf_counter() - t0) * 1e3
        N.knn(ctx, *mats[m], 10)      # (warm-up)
        ctx.sync()
    for _ in range(ROUNDS):
        for m in metrics:
            t0 = time.perf_counter()
            N.knn(ctx, *mats[m], 10)
            ctx.sync()
            ms[m].append((time.perf_counter() - t0) * 1e3)
    for m in metrics:
        rec = {"shape": [n, n, d], "dtype": "float32", "k": 10, "metric": m, "ms_median": round(float(np.median(ms[m])), 2),
               "ms_min": round(min(ms[m]), 2), "ms_all": [round(v, 2) for v in ms[m]], "create_both_ms": round(ms[m + "_create"], 1),
               "hamming_over_this": round(float(np.median(ms["hamming"]) / np.median(ms[m])), 2)}
        print(json.dumps(rec), flush=True)
        if out:
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
    del mats
