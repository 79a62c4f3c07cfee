#!/usr/bin/env python3
"""Golden vectors for the exact gold ranks (kz_gold_ranks, Kiez.gold_ranks, evaluate.rank_metrics) by RUNNING THE REAL REFERENCE
(build container only).

    python tools/gen_golden_ranks.py      # writes tests/golden/full_ranks.npz

The reference reaches a rank only through a full-length neighbour list: SklearnNN(n_candidates = n_target) and kiez.evaluate.hits
on it.  One two-sided float64 input whose target is a noisy permutation of the source among distractor rows (the gold ranks spread
from 0 to the tens), euclidean and cosine; per metric the reference's full lists (int16) and its hits(k = [1, 5, 10, n_target]).
Some source rows have no gold pair, and the gold dict holds one pair whose key is no source row (it counts in the denominator
only).  The fixtures of the other generators are not touched.  numpy's SIMD dispatch is disabled as in tools/gen_golden.py.
"""
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

_DISABLE = "AVX2 FMA3 AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if os.environ.get("NPY_DISABLE_CPU_FEATURES") != _DISABLE:
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=_DISABLE)
    sys.exit(subprocess.call([sys.executable, *sys.argv], env=env))

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT))
import ref_loader  # noqa: E402

from tests import rank_restate as RR  # noqa: E402

OUT = ROOT / "tests" / "golden"
N_S, N_T, D = 48, 64, 6
METRICS = ("euclidean", "cosine")


def main():
    R = ref_loader.load_reference()
    spec = importlib.util.spec_from_file_location("kiez_eval_metrics", ref_loader.REF / "kiez" / "evaluate" / "eval_metrics.py")
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)

    rng = np.random.RandomState(1234)
    source = rng.randn(N_S, D)
    perm = rng.permutation(N_T)[:N_S]
    target = rng.randn(N_T, D)                                   # (rows outside perm: distractors)
    target[perm] = source + 0.9 * rng.randn(N_S, D)              # noise of the data's own scale: many gold rows are not the nearest
    gold = {int(i): int(perm[i]) for i in range(N_S) if i % 7 != 3}   # (rows 3, 10, 17, ...: no gold pair)
    gold[N_S + 5] = 0                                            # a key that is no source row: denominator only
    ks = [1, 5, 10, N_T]
    out = {"source": source, "target": target, "gold_keys": np.array(list(gold.keys()), dtype=np.int64),
           "gold_vals": np.array(list(gold.values()), dtype=np.int64), "ks": np.array(ks, dtype=np.int64),
           "metrics": np.array(METRICS)}
    gold_vec = np.full(N_S, -1, dtype=np.int64)
    for a, b in gold.items():
        if a < N_S:
            gold_vec[a] = b
    for metric in METRICS:
        nn = R.SklearnNN(n_candidates=N_T, metric=metric, algorithm="brute")
        nn.fit(source, target)
        dist, ind = nn.kneighbors(k=N_T, return_distance=True)
        assert ind.shape == (N_S, N_T) and all(sorted(r) == list(range(N_T)) for r in ind.tolist())
        h = ev.hits(ind, gold, k=list(ks))
        out[f"{metric}__ind"] = ind.astype(np.int16)
        out[f"{metric}__hits"] = np.array([h[k] for k in ks], dtype=np.float64)
        pos = RR.positions(ind, gold_vec)
        print(metric, "hits", h, "ranks: max", int(pos.max()), "mean", float(pos[pos >= 0].mean()), "zeros", int((pos == 0).sum()))
        assert pos.max() >= 10 and (pos == 0).sum() >= 5         # (ranks from 0 to the tens; change the draw if not)
        assert np.min(np.diff(np.sort(dist, axis=1), axis=1)) > 1e-9   # (no near-ties: the list order is the order by exact value)
    np.savez_compressed(OUT / "full_ranks.npz", **out)
    print("wrote", OUT / "full_ranks.npz", (OUT / "full_ranks.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
