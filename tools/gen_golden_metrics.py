#!/usr/bin/env python3
"""Golden vectors of the metrics beyond the Minkowski family (braycurtis, seuclidean, correlation, hamming) by RUNNING THE REAL
REFERENCE (build container only).

    python tools/gen_golden_metrics.py      # writes tests/golden/metrics_*.npz and tests/golden/metrics_MANIFEST.json

Same layout as tools/gen_golden.py's fixtures (inputs, configuration, the reference's outputs per hubness kind and k, the
intermediates dist/ind_t2s, dist/ind_s2t and the unsorted transform), plus `V` for seuclidean (metric_params={"V": V}).  Every
metric x {float32, float64} x {single source, two sources} with every hubness kind the device runs on these distances
(DisSimLocal refuses them: its error is recorded), scikit-learn's brute-force route; plus correlation with a constant index row and
one small-d float32 braycurtis case on scikit-learn's "auto" route (a ball tree there: float64 values, compared to one float32 ulp).
The existing fixtures and tests/golden/MANIFEST.json are not touched.  numpy's SIMD dispatch is disabled as in tools/gen_golden.py.
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

sys.path.insert(0, str(Path(__file__).resolve().parent))
from ref_loader import load_reference  # noqa: E402

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden"
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
CASES = []


def run_case(name, source, target, K, ks, metric, V=None, sk_algorithm="brute"):
    out = {"source": source, "K": np.int64(K), "ks": np.array([(-1 if k is None else k) for k in ks]),
           "metric": np.array(metric), "p": np.int64(2), "algorithm": np.array(sk_algorithm)}
    if target is not None:
        out["target"] = target
    if V is not None:
        out["V"] = V
    for tag, hname, kw in HUBNESS:
        algo_kw = dict(n_candidates=K, metric=metric, algorithm=sk_algorithm)
        if V is not None:
            algo_kw["metric_params"] = {"V": V}
        try:
            hub = CLS[hname](nn_algo=R.SklearnNN(**algo_kw), **kw)
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
    print("wrote", name)


def main():
    rng = np.random.RandomState(61)
    for metric in ("braycurtis", "seuclidean", "correlation", "hamming"):
        for dt in (np.float32, np.float64):
            d = 13
            if metric == "hamming":   # (few distinct values per feature: mismatches are not certain)
                s, t = rng.randint(0, 3, (90, d)).astype(dt), rng.randint(0, 3, (70, d)).astype(dt)
            else:
                s, t = rng.randn(90, d).astype(dt), rng.randn(70, d).astype(dt)
            V = rng.uniform(0.5, 2.0, d) if metric == "seuclidean" else None
            tag = f"metrics_{metric}_{np.dtype(dt).name}"
            run_case(f"{tag}_two", s, t, 8, [8, 3], metric, V)
            run_case(f"{tag}_single", s, None, 8, [8, 2], metric, V)
    # correlation: a constant index row (its distance is NaN: ranked after every finite value) in a small index
    s, t = rng.randn(40, 9), rng.randn(12, 9)
    t[5] = 0.25
    run_case("metrics_correlation_constant_row", s, t, 12, [12, 4], "correlation")
    # braycurtis, float32, d = 10 on scikit-learn's "auto" route (ball tree: float64 values of the upcast inputs)
    s, t = rng.rand(80, 10).astype(np.float32), rng.rand(60, 10).astype(np.float32)
    run_case("metrics_braycurtis_float32_auto", s, t, 6, [6, 2], "braycurtis", sk_algorithm="auto")
    import scipy
    import sklearn
    manifest = {"generator": "tools/gen_golden_metrics.py",
                "reference": "dobraczka/kiez v0.5.0, hot-path modules loaded by file path (tools/ref_loader.py)",
                "python": platform.python_version(), "numpy": np.__version__, "scipy": scipy.__version__,
                "scikit-learn": sklearn.__version__, "NPY_DISABLE_CPU_FEATURES": _DISABLE, "cases": CASES}
    (OUT / "metrics_MANIFEST.json").write_text(json.dumps(manifest, indent=2) + "\n")


if __name__ == "__main__":
    main()
