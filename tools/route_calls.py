"""A fixed set of kz_knn / kz_knn_dual calls that reaches every stage of kz_knn_impl and every route of kz_route.h, for comparing two
builds of the library (KIEZ_AMD_LIB) call by call: results, statistics and -- under `rocprofv3 --kernel-trace` -- launches.

    python tools/route_calls.py run <out.jsonl>            one line per call: integer statistics, sha1 of the distance / index bits
    python tools/route_calls.py launches <kernel_trace.csv> <out.jsonl>
                                                           one line per call: launches, sha1 of the sorted multiset of
                                                           (kernel, grid, workgroup, LDS) -- calls are delimited in the trace by
                                                           kz_max_abs_diff_kernel, which no search launches
    python tools/route_calls.py compare <a.jsonl> <b.jsonl> [ignored fields ...]

profiles/knn_impl_refactor.md has the numbers of the split of kz_knn_impl."""
import csv
import hashlib
import json
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RANGE_GROUPING = ("n_range_pairs", "n_range_group_rows")   # differ between two runs of ONE build (atomics decide the grouping)


def _uniform(n, d, seed, dtype=np.float32):
    return np.random.default_rng(seed).random((n, d)).astype(dtype)


def _crowded(n_q, n_i, d, n_rows, n_near, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    q, y = rng.random((n_q, d)).astype(np.float32), rng.random((n_i, d)).astype(np.float32)
    point = rng.random(d)
    y[rng.choice(n_i, n_near, replace=False)] = (point + 1e-4 * rng.standard_normal((n_near, d))).astype(np.float32)
    q[rng.choice(n_q, n_rows, replace=False)] = (point + 1e-3 * rng.standard_normal((n_rows, d))).astype(np.float32)
    return q.astype(dtype), y.astype(dtype)


def _tight(n, d, seed):   # 40 tight clusters far from the centre, rows shuffled (bench.py "hard")
    rng = np.random.default_rng(seed)
    centres = np.random.default_rng(5).standard_normal((40, d)) * 3
    return (centres[rng.integers(0, 40, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)


def calls():
    """(name, options, metric, data builder, k, kind) -- kind: 'knn', 'self' (exclude_self) or 'dual'."""
    out = []
    u = lambda nq, ni, d=32, dt=np.float32: (lambda: (_uniform(nq, d, 1, dt), _uniform(ni, d, 2, dt)))
    # every row to the exact kernels, per element type and metric class
    for dt in (np.float32, np.float64):
        for metric in ("sqeuclidean", "cosine", "manhattan"):
            out.append(("all exact %s %s" % (np.dtype(dt).name, metric), {"eps_scale": 1e30}, metric, u(3001, 9000, 32, dt), 10, "knn"))
    # a handful / a hundred uncertified rows, each exact-kernel variant, three index sizes
    for er in (0, 3):
        for rows in (20, 100):
            for ni in (3001, 9000, 21000):
                out.append(("exact_rows %d, %d rows, %d" % (er, rows, ni), {"exact_rows": er, "spec_rows": 0},
                            "euclidean", (lambda rows=rows, ni=ni: _crowded(2000, ni, 32, rows, 40, 7)), 10, "knn"))
    # exact-only, long-k route on lists of 128 and as lists of 16
    out.append(("k 600", {}, "euclidean", u(700, 9000), 600, "knn"))
    out.append(("k 600 cosine f64", {}, "cosine", u(700, 9000, 32, np.float64), 600, "knn"))
    out.append(("k 600 self", {}, "euclidean", (lambda: (_uniform(3000, 32, 3),) * 2), 600, "self"))
    out.append(("k 200 lists of 128", {"short_ord": 0}, "euclidean", u(1500, 40000), 200, "knn"))
    out.append(("k 160 lists of 16", {"short_ord_min_tiles": 4}, "euclidean", u(1500, 40000), 160, "knn"))
    # speculative rescue
    for dt, ni in ((np.float32, 9000), (np.float64, 9000), (np.float32, 70001)):
        out.append(("rescue %s %d" % (np.dtype(dt).name, ni), {}, "euclidean", (lambda dt=dt, ni=ni: _crowded(4096, ni, 32, 20, 40, 8, dt)), 10, "knn"))
    # the plain search per tier; short-list route, and what it leaves
    out.append(("fp16", {}, "euclidean", u(5000, 20000, 64), 10, "knn"))
    out.append(("split-bf16 k 50", {"precision": 2}, "cosine", u(5000, 20000, 64), 50, "knn"))
    out.append(("float32 operands", {"precision": 1}, "euclidean", u(5000, 20000, 64), 10, "knn"))
    out.append(("short lists k 30", {"short_ord_min_tiles": 8}, "euclidean", u(2000, 40000), 30, "knn"))
    out.append(("short lists k 30 eps 40", {"short_ord_min_tiles": 8, "eps_scale": 40.0}, "euclidean", u(2000, 40000), 30, "knn"))
    out.append(("self k 20 short lists", {"short_ord_min_tiles": 8}, "euclidean", (lambda: (_uniform(20000, 40, 3),) * 2), 20, "self"))
    # the cases of tests/test_gpu_route_stats.py
    out.append(("tier change between chunks", {"short_ord_min_tiles": 8, "chunk_rows": 4096, "eps_scale": 1e9}, "euclidean", u(8192, 9000), 30, "knn"))
    out.append(("more lists", {}, "euclidean", (lambda: _crowded(4096, 9000, 32, 100, 40, 3)), 10, "knn"))
    out.append(("exact direct", {"precision": 2, "spec_rows": 0}, "euclidean", (lambda: _crowded(4096, 9000, 32, 20, 40, 4)), 10, "knn"))
    # tier probe with the gate lowered: tight clusters (ladder -> wide route; wide route off -> hard verdict), uniform rows (floor)
    tight = lambda: (_tight(20000, 64, 7), _tight(21000, 64, 8))
    out.append(("probe, tight", {"probe_min_pairs": 1.0}, "euclidean", tight, 10, "knn"))
    out.append(("probe, tight, no wide route", {"probe_min_pairs": 1.0, "wide_lists": 0}, "euclidean", tight, 10, "knn"))
    out.append(("probe, uniform", {"probe_min_pairs": 1.0}, "euclidean", u(20000, 21000, 64), 10, "knn"))
    out.append(("no probe, tight (ladder after the fact)", {"tier_probe": 0}, "euclidean", tight, 10, "knn"))
    # shared sweep with and without the nested sample, and on short lists
    out.append(("shared sweep, nested", {"dual_force": 1}, "euclidean", u(30000, 31000, 64), 10, "dual"))
    out.append(("shared sweep, classic", {"dual_force": 1, "dual_nested": 0}, "euclidean", u(30000, 31000, 64), 10, "dual"))
    out.append(("shared sweep k 50", {"dual_force": 1, "dual_short_min_tiles": 8}, "euclidean", u(30000, 31000, 64), 50, "dual"))
    return out


DEFAULTS = {"eps_scale": 1.0, "exact_rows": 3, "spec_rows": 64, "short_ord": 1, "short_ord_min_tiles": 48, "precision": 0, "chunk_rows": 0,
            "probe_min_pairs": 5e10, "wide_lists": 32, "tier_probe": 1024, "dual_force": 0, "dual_nested": 1, "dual_short_min_tiles": 128}


def run(path):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    mark = ctx.to_device(np.zeros(4))
    with open(path, "w") as f:
        for name, opts, metric, data, k, kind in calls():
            q, y = data()
            qm = N.DeviceMatrix(ctx, q, metric)
            ym = qm if y is q else N.DeviceMatrix(ctx, y, metric)
            for o, v in DEFAULTS.items():
                ctx.set_option(o, opts.get(o, v))
            N.max_abs_diff(ctx, mark, mark)
            if kind == "dual":
                res = N.knn_dual(ctx, qm, ym, k)
            else:
                res = (N.knn(ctx, qm, ym, k, exclude_self=kind == "self"),)
            N.max_abs_diff(ctx, mark, mark)
            rec = {"call": name}
            for j, (d, i, st) in enumerate(res):
                rec["stats%d" % j] = {key: v for key, v in st.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool)}
                rec["dist%d" % j] = hashlib.sha1(d.numpy().tobytes()).hexdigest()
                rec["ind%d" % j] = hashlib.sha1(i.numpy().tobytes()).hexdigest()
            f.write(json.dumps(rec) + "\n")
            f.flush()
            del qm, ym
        for o, v in DEFAULTS.items():
            ctx.set_option(o, v)


def launches(trace, path):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [c[0] for c in calls()]
    shape_cols = [c for c in rows[0] if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
    assert len(shape_cols) >= 3, list(rows[0])
    segs, cur, marks = [], None, 0
    for r in rows:
        if "kz_max_abs_diff_kernel" in r["Kernel_Name"]:
            marks += 1
            if cur is None:
                cur = []
            else:
                segs.append(cur)
                cur = None
        elif cur is not None:
            cur.append((r["Kernel_Name"],) + tuple(r[c] for c in shape_cols))
    assert len(segs) == len(names) and marks == 2 * len(names), (len(segs), marks, len(names))
    with open(path, "w") as f:
        for name, seg in zip(names, segs):
            multiset = sorted(Counter(seg).items())
            f.write(json.dumps({"call": name, "launches": len(seg), "kernels": len(multiset),
                                "multiset": hashlib.sha1(json.dumps(multiset).encode()).hexdigest()}) + "\n")


def compare(a, b, ignore):
    ra, rb = [json.loads(l) for l in open(a)], [json.loads(l) for l in open(b)]
    bad = 0 if len(ra) == len(rb) else 1
    for x, y in zip(ra, rb):
        for key in sorted(set(x) | set(y)):
            vx, vy = x.get(key), y.get(key)
            if isinstance(vx, dict) and isinstance(vy, dict):
                vx = {k: v for k, v in vx.items() if k not in ignore}
                vy = {k: v for k, v in vy.items() if k not in ignore}
            if vx != vy:
                bad += 1
                print("DIFFERENT", x["call"], key, vx, vy)
    print("%d / %d calls, %d differences%s" % (len(ra), len(rb), bad, (" (ignoring " + ", ".join(ignore) + ")") if ignore else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "launches":
        launches(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], tuple(sys.argv[4:])))
