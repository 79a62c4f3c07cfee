#!/usr/bin/env python3
"""Golden vectors for the gold ranks under a hubness reduction (kz_gold_ranks_reduced, Kiez.gold_ranks(reduced=True)) by RUNNING THE
REAL REFERENCE (build container only).

    python tools/gen_golden_reduced_ranks.py      # writes tests/golden/reduced_ranks.npz

The reference reaches a reduced rank only inside a candidate list, so the lists are the whole index: n_candidates = n_target, and
the rank of a gold row is its position in the reference's kneighbors(k = n_target) after CSLS, LocalScaling 'standard', NICDM or
MutualProximity 'normal'.  One two-sided float64 input (the target: noisy copies of source rows among unrelated rows), euclidean and
cosine; per metric and kind the reference's sorted index matrix (int16) and a per-row `clear` mask: the gold's reduced distance
differs from both its neighbours in the reference's sorted list by more than 1e-9, so that its position does not hang on the last
bits of exp / erfc.  The fixtures of the other generators are not touched.  numpy's SIMD dispatch is disabled as in
tools/gen_golden.py.
"""
import os
import subprocess
import sys
import warnings
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
N_S, N_T, N_COPY, D = 100, 80, 60, 8
METRICS = ("euclidean", "cosine")
SEED = 4321
CLEAR_GAP = 1e-9
MIN_CLEAR = 0.9


def main():
    R = ref_loader.load_reference()
    kinds = {"csls": (R.CSLS, {}), "ls": (R.LocalScaling, {"method": "standard"}), "nicdm": (R.LocalScaling, {"method": "nicdm"}),
             "mp_normal": (R.MutualProximity, {"method": "normal"})}
    rng = np.random.RandomState(SEED)
    source = rng.randn(N_S, D)
    rows = rng.permutation(N_T)[:N_COPY]                         # target rows that are copies; the others are unrelated
    target = rng.randn(N_T, D)
    target[rows] = source[:N_COPY] + 0.9 * rng.randn(N_COPY, D)  # noise of the data's own scale: many gold rows are not the nearest
    gold = np.full(N_S, -1, dtype=np.int64)                      # (source rows N_COPY..: no copy, no gold)
    gold[:N_COPY] = rows
    gold[3:N_COPY:7] = -1                                        # (and some copies without a gold pair)
    out = {"source": source, "target": target, "gold": gold, "metrics": np.array(METRICS), "kinds": np.array(list(kinds))}
    n_gold = int((gold >= 0).sum())
    for metric in METRICS:
        for kind, (cls, kw) in kinds.items():
            hub = cls(nn_algo=R.SklearnNN(n_candidates=N_T, metric=metric, algorithm="brute"), **kw)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                hub.fit(source, target)
                dist, ind = hub.kneighbors(N_T)
            assert ind.shape == (N_S, N_T) and all(sorted(r) == list(range(N_T)) for r in ind.tolist())
            assert np.all(np.diff(dist, axis=1) >= 0) and np.all(np.isfinite(dist))
            pos = RR.positions(ind, gold)
            p = np.where(pos >= 0, pos, 0)
            r = np.arange(N_S)
            wg = dist[r, p]
            below = np.where(p > 0, wg - dist[r, np.maximum(p - 1, 0)], np.inf)
            above = np.where(p < N_T - 1, dist[r, np.minimum(p + 1, N_T - 1)] - wg, np.inf)
            clear = (pos >= 0) & (below > CLEAR_GAP) & (above > CLEAR_GAP)
            share = clear.sum() / n_gold
            print(metric, kind, "clear", int(clear.sum()), "of", n_gold, "ranks: max", int(pos.max()), "zeros", int((pos == 0).sum()))
            assert share >= MIN_CLEAR, f"{metric} {kind}: only {share:.0%} of the gold rows are clear -- pick another seed"
            assert pos.max() >= 10 and (pos == 0).sum() >= 5     # (ranks from 0 to the tens; change the draw if not)
            out[f"{metric}__{kind}__ind"] = ind.astype(np.int16)
            out[f"{metric}__{kind}__clear"] = clear
    np.savez_compressed(OUT / "reduced_ranks.npz", **out)
    print("wrote", OUT / "reduced_ranks.npz", (OUT / "reduced_ranks.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
