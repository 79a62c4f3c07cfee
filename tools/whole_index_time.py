"""Time of kz_knn_reduced (CSLS, k = 10, float32 euclidean) beside kz_gold_ranks_reduced with a gold id on every row -- the same value
work with a count where the first has a selection -- and, for context, the candidate-list route (fit + kneighbors of Kiez with CSLS,
n_candidates = 10) on the same data.  A pair of HIP events around each call, one warm-up, the median of `--reps` (>= 5) calls: every
timed call ends with a synchronise of the context's stream, so the events -- recorded on the otherwise idle null stream before the
call and after it -- enclose all of its device work.  One JSON line per shape.

    python tools/whole_index_time.py [--out FILE] [--cases small|large|all] [--reps N] [--native-only]

`--native-only` is the run to put under `rocprofv3 --kernel-trace --stats`: the two native calls alone, so that the trace's per-kernel
totals split into the distance kernel, the count kernel and the two selection kernels.
"""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import _native as N  # noqa: E402

CASES = {"small": [(15_000, 300)], "large": [(100_000, 128)]}
CASES["all"] = CASES["small"] + CASES["large"]


class Events:
    """A pair of HIP events on the null stream, recorded around a call that synchronises its own stream before it returns."""

    def __init__(self):
        # the HIP runtime the library itself is linked to and has loaded (one runtime per process)
        N.load()
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
        if len(paths) != 1:
            raise RuntimeError(f"expected one loaded libamdhip64.so, found {paths}")
        self.hip = C.CDLL(paths[0])
        self.start, self.stop = C.c_void_p(), C.c_void_p()
        for ev in (self.start, self.stop):
            self._ok(self.hip.hipEventCreate(C.byref(ev)))

    @staticmethod
    def _ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP event call failed with status {rc}")

    def ms(self, fn):
        self._ok(self.hip.hipEventRecord(self.start, None))
        fn()
        self._ok(self.hip.hipEventRecord(self.stop, None))
        self._ok(self.hip.hipEventSynchronize(self.stop))
        out = C.c_float(0.0)
        self._ok(self.hip.hipEventElapsedTime(C.byref(out), self.start, self.stop))
        return float(out.value)


def median_ms(ev, fn, reps):
    fn()   # warm-up: code objects, the pool's buffers
    return statistics.median(ev.ms(fn) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--native-only", action="store_true", help="skip the candidate-list fit + kneighbors")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    lines = []
    for n, d in CASES[args.cases]:
        s, t = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
        gold = ctx.to_device(rng.integers(0, n, n).astype(np.int64))
        # (states of the data's own scale: means near the typical distance)
        scale = float(np.sqrt(2.0 * d))
        q_a, t_a = (ctx.to_device(scale * (0.5 + 0.5 * rng.random(n))) for _ in range(2))
        knn_ms = median_ms(ev, lambda: N.knn_reduced(ctx, sm, tm, 10, N.RANK_CSLS, q_a, t_a), reps)
        rank_ms = median_ms(ev, lambda: N.gold_ranks_reduced(ctx, sm, tm, gold, N.RANK_CSLS, q_a, t_a), reps)
        # the two agree: the rank of the row at column 9 is 9
        _, ind = N.knn_reduced(ctx, sm, tm, 10, N.RANK_CSLS, q_a, t_a)
        last = ctx.to_device(np.ascontiguousarray(ind.numpy()[:, 9]))
        assert (N.gold_ranks_reduced(ctx, sm, tm, last, N.RANK_CSLS, q_a, t_a).numpy() == 9).all()
        line = {"metric": "euclidean", "dtype": "float32", "n_query": n, "n_index": n, "d": d, "k": 10, "kind": "csls", "reps": reps,
                "knn_reduced_ms": round(knn_ms, 2), "gold_ranks_reduced_ms": round(rank_ms, 2),
                "knn_reduced_over_gold_ranks_reduced": round(knn_ms / rank_ms, 3),
                "pairs_per_s_knn_reduced": round(n * n / knn_ms * 1e3, 0)}
        if not args.native_only:
            from kiez_amd import Kiez

            def candidate_lists():
                kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
                kz.fit(s, t).kneighbors_device(10)
                ctx.sync()
            line["candidate_list_fit_kneighbors_ms"] = round(median_ms(ev, candidate_lists, reps), 2)   # (includes both uploads)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
