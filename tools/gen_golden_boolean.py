#!/usr/bin/env python3
"""Golden vectors of scipy's seven boolean metrics (jaccard, dice, rogerstanimoto, russellrao, sokalmichener, sokalsneath, yule) by
RUNNING THE REAL REFERENCE (build container only).

    python tools/gen_golden_boolean.py      # writes tests/golden/boolean_*.npz and tests/golden/boolean_MANIFEST.json

Same layout as tools/gen_golden_metrics.py's fixtures (inputs, configuration, the reference's outputs per hubness kind and k, the
intermediates dist/ind_t2s, dist/ind_s2t and the unsorted transform; DisSimLocal refuses these distances: its error is recorded).
The inputs are drawn ONCE (d = 509: 16 image words, the last one partly filled) and shared by the metrics: float32 rows with two
sources and float64 rows with a single source per metric, dice with all-false rows (NaN, ranked last; no hubness reduction) and
jaccard on np.bool_ arrays.  The fixtures of the other generators are not touched.  numpy's SIMD dispatch is disabled as in
tools/gen_golden.py.

Values are ratios of small integers: ties at the K-th place are common and scikit-learn's order among ties is unstable, so the GPU
test compares rescaled results only on rows whose candidate set is the reference's.  This script prints, per case, how many rows
have the candidate set of the device order (value, index row; tests/boolean_restate.py); the test asserts at least MIN_COMPARABLE.
"""
import json
import os
import platform
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
from ref_loader import load_reference  # noqa: E402

from tests import boolean_restate as BR  # noqa: E402

OUT = ROOT / "tests" / "golden"
R = load_reference()
warnings.simplefilter("ignore")

HUBNESS = [
    ("none", None, {}),
    ("csls", "CSLS", {}),
    ("mp_normal", "MutualProximity", {"method": "normal"}),
    ("mp_empiric", "MutualProximity", {"method": "empiric"}),
    ("ls", "LocalScaling", {"method": "standard"}),
    ("nicdm", "LocalScaling", {"method": "nicdm"}),
    ("dsl", "DisSimLocal", {}),
]
CLS = {None: R.NoHubnessReduction, "CSLS": R.CSLS, "MutualProximity": R.MutualProximity,
       "LocalScaling": R.LocalScaling, "DisSimLocal": R.DisSimLocal}
MIN_COMPARABLE = 45
CASES = []
COMPARABLE = {}


def run_case(name, source, target, K, ks, metric, hubness=HUBNESS):
    out = {"source": source, "K": np.int64(K), "ks": np.array([(-1 if k is None else k) for k in ks]),
           "metric": np.array(metric), "p": np.int64(2), "algorithm": np.array("brute")}
    if target is not None:
        out["target"] = target
    for tag, hname, kw in hubness:
        try:
            hub = CLS[hname](nn_algo=R.SklearnNN(n_candidates=K, metric=metric, algorithm="brute"), **kw)
        except ValueError as e:  # DisSimLocal
            out[f"{tag}__raises"] = np.array(str(e))
            continue
        hub.fit(source, target)
        if hname is not None:
            tgt = source if target is None else target
            d_t2s, i_t2s = hub.nn_algo.kneighbors(k=K, query=tgt, s_to_t=False, return_distance=True)
            d_s2t, i_s2t = hub.nn_algo.kneighbors(query=None, k=K, return_distance=True)
            tr, _ = hub.transform(d_s2t.copy(), i_s2t.copy(), hub.nn_algo.source_.copy())
            out[f"{tag}__dist_t2s"], out[f"{tag}__ind_t2s"] = d_t2s, i_t2s
            out[f"{tag}__dist_s2t"], out[f"{tag}__ind_s2t"] = d_s2t, i_s2t
            out[f"{tag}__transformed"] = tr
        for k in ks:
            d, i = hub.kneighbors(k)
            ktag = "None" if k is None else str(k)
            out[f"{tag}__k{ktag}__dist"], out[f"{tag}__k{ktag}__ind"] = d, i
    np.savez_compressed(OUT / f"{name}.npz", **out)
    CASES.append(name)
    if "csls__ind_s2t" in out:
        # rows whose K candidates are, as a set, those of the device order (value, index row)
        _, di = BR.knn(metric, source, source if target is None else target, K, exclude_self=target is None)
        same = int(sum(set(a) == set(b) for a, b in zip(di, out["csls__ind_s2t"])))
        COMPARABLE[name] = same
        assert same >= MIN_COMPARABLE, (name, same)   # (change the draw and record it in the manifest; the floor stays)
        print("wrote", name, "comparable rows:", same, "of", len(di))
    else:
        print("wrote", name)


def main():
    rng = np.random.RandomState(71)
    d = 509
    s = rng.rand(90, d) < 0.5
    t = rng.rand(70, d) < 0.5
    s1 = rng.rand(90, d) < 0.5
    for metric in BR.BOOLEAN_METRICS:
        run_case(f"boolean_{metric}_float32_two", s.astype(np.float32), t.astype(np.float32), 8, [8, 3], metric)
        run_case(f"boolean_{metric}_float64_single", s1.astype(np.float64), None, 8, [8, 2], metric)
    # dice: all-false rows (0 / 0 = NaN between two of them: ranked after every finite value) in a small index
    es, et = (rng.rand(20, 40) < 0.3).astype(np.float64), (rng.rand(12, 40) < 0.3).astype(np.float64)
    es[4] = 0.0
    et[[2, 9]] = 0.0
    run_case("boolean_dice_empty_rows", es, et, 12, [12, 4], "dice", hubness=HUBNESS[:1])
    # jaccard on np.bool_ arrays (the device uploads them as float32)
    run_case("boolean_jaccard_bool_two", s, t, 8, [8, 3], "jaccard")
    import scipy
    import sklearn
    manifest = {"generator": "tools/gen_golden_boolean.py",
                "reference": "dobraczka/kiez v0.5.0, hot-path modules loaded by file path (tools/ref_loader.py)",
                "python": platform.python_version(), "numpy": np.__version__, "scipy": scipy.__version__,
                "scikit-learn": sklearn.__version__, "NPY_DISABLE_CPU_FEATURES": _DISABLE,
                "draw": "np.random.RandomState(71), d = 509: s = rand(90, d) < 0.5, t = rand(70, d) < 0.5, s1 = rand(90, d) < 0.5",
                "min_comparable_rows": MIN_COMPARABLE, "comparable_rows": COMPARABLE, "cases": CASES}
    (OUT / "boolean_MANIFEST.json").write_text(json.dumps(manifest, indent=2) + "\n")


if __name__ == "__main__":
    main()
