"""scipy's seven boolean metrics (CPU): the restatement of tests/boolean_restate.py -- the expressions the device follows -- equals
scikit-learn's pairwise_distances bit for bit, the public interface accepts the seven names, and the fixtures are the manifest's."""
import json
import warnings
import zlib

import numpy as np
import pytest

from tests import boolean_restate as BR
from tests.golden_util import GOLDEN


def _rows(rng, n, d, density, dtype):
    x = rng.random((n, d)) < density
    x[0] = False          # an all-false row (dice, sokalsneath: NaN against another one)
    x[1] = True           # an all-true row
    if dtype == np.bool_:
        return x
    v = np.where(x, rng.uniform(-3.0, 3.0, (n, d)), 0.0).astype(dtype)
    v[x & (v == 0)] = 1.0
    if d > 2:
        v[2, 0] = -0.0    # (x != 0: -0.0 is false)
    return v


@pytest.mark.parametrize("metric", BR.BOOLEAN_METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.bool_])
def test_restatement_is_scikit_learn_bit_for_bit(metric, dtype):
    from sklearn.metrics import pairwise_distances
    rng = np.random.default_rng(zlib.crc32(f"{metric} {np.dtype(dtype).name}".encode()))
    for d in (5, 13, 64, 200, 1000):
        for density in (0.05, 0.5, 0.9):
            x, y = _rows(rng, 14, d, density, dtype), _rows(rng, 37, d, density, dtype)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")     # (DataConversionWarning: the rows are cast to bool)
                ref = pairwise_distances(x, y, metric=metric)
            got = BR.ranking_values(metric, x, y)
            assert ref.dtype == np.float64 and got.dtype == np.float64
            np.testing.assert_array_equal(got, ref, err_msg=f"{metric} {dtype} d={d} density={density}")
            if metric in ("dice", "sokalsneath"):
                assert np.isnan(got[0, 0])
            else:
                assert np.isfinite(got).all()


def test_restated_knn_order():
    rng = np.random.default_rng(1)
    x, y = _rows(rng, 9, 40, 0.3, np.float64), _rows(rng, 30, 40, 0.3, np.float64)
    d, i = BR.knn("dice", x, y, 30)
    assert np.isnan(d[0, -1]) and i[0, -1] == 0 and np.isfinite(d[0, :-1]).all()      # (NaN after every finite value)
    key = np.nan_to_num(d, nan=np.inf)
    assert (np.diff(key, axis=1) >= 0).all()
    tied = np.diff(key, axis=1) == 0
    assert (np.diff(i, axis=1)[tied] > 0).all()                                       # (ties by index row)


def test_the_seven_names_resolve():
    from kiez_amd.neighbors import SklearnNN, canonical_metric
    for m in BR.BOOLEAN_METRICS:
        assert canonical_metric(m) == m
        assert m in SklearnNN.valid_metrics
        assert SklearnNN(metric=m)._metric_c == m
    assert SklearnNN.valid_metrics == sorted(SklearnNN.valid_metrics)


def test_native_metric_ids():
    from kiez_amd import _native as N
    assert (N.KZ_JACCARD, N.KZ_DICE, N.KZ_ROGERSTANIMOTO, N.KZ_RUSSELLRAO, N.KZ_SOKALMICHENER, N.KZ_SOKALSNEATH, N.KZ_YULE) == \
        (10, 11, 12, 13, 14, 15, 16)
    assert [N.METRIC_IDS[m] for m in BR.BOOLEAN_METRICS] == [10, 11, 12, 13, 14, 15, 16]
    assert tuple(N.BOOLEAN_METRICS) == BR.BOOLEAN_METRICS
    assert len(set(N.METRIC_IDS.values())) == len(N.METRIC_IDS) == 17


def test_header_lists_the_ids():
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "kiez_amd.h").read_text()
    for i, m in enumerate(BR.BOOLEAN_METRICS):
        assert f"KZ_{m.upper()} = {10 + i}" in text


def test_dissimlocal_refuses_them():
    from kiez_amd import Kiez
    from kiez_amd.distributed import ShardedKiez
    from kiez_amd.neighbors import SklearnNN
    for m in BR.BOOLEAN_METRICS:
        with pytest.raises(ValueError, match="only supports"):
            Kiez(algorithm=SklearnNN(metric=m), hubness="DisSimLocal")
        with pytest.raises(ValueError, match="only supports"):
            ShardedKiez(n_candidates=5, algorithm_kwargs={"metric": m}, hubness="DisSimLocal", engine=object(), comm=object())
        with pytest.raises(NotImplementedError, match="metric_params"):
            SklearnNN(metric=m, metric_params={"w": [1.0]})
        assert ShardedKiez(n_candidates=5, algorithm_kwargs={"metric": m}, engine=object(), comm=object()).metric == m


def test_non_float_rows_go_up_as_float32():
    from kiez_amd.neighbors import SklearnNN
    b = np.array([[True, False], [False, False]])
    for arr in (b, b.astype(np.int64), b.astype(np.float16), b.astype(np.uint8)):
        up = SklearnNN(metric="jaccard")._prepare(arr)
        assert up.dtype == np.float32 and np.array_equal(up != 0, b)
        assert SklearnNN(metric="hamming")._prepare(arr).dtype == np.float64          # (every other metric: as before)
    assert SklearnNN(metric="yule")._prepare(b.astype(np.float64)).dtype == np.float64


def test_manifest_lists_exactly_the_fixtures():
    manifest = json.loads((GOLDEN / "boolean_MANIFEST.json").read_text())
    assert sorted(manifest["cases"]) == sorted(p.stem for p in GOLDEN.glob("boolean_*.npz"))
    expect = {f"boolean_{m}_{t}" for m in BR.BOOLEAN_METRICS for t in ("float32_two", "float64_single")}
    expect |= {"boolean_dice_empty_rows", "boolean_jaccard_bool_two"}
    assert set(manifest["cases"]) == expect
    assert manifest["min_comparable_rows"] == 45
    assert all(v >= 45 for v in manifest["comparable_rows"].values()) and len(manifest["comparable_rows"]) == 15
    for p in GOLDEN.glob("boolean_*"):
        assert p.stat().st_size < 1 << 20
        assert not p.name.startswith("metrics_")
