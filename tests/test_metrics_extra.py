"""braycurtis, seuclidean, correlation and hamming (CPU): the restatements of tests/metric_restate.py -- the expressions the device
kernels follow -- equal scikit-learn's brute-force search bit for bit, and the public interface accepts the four names."""
import numpy as np
import pytest

from tests import metric_restate as MR

DIMS = list(range(1, 17)) + [127, 128, 129, 300, 301]


def _rows(rng, n, d, dtype, kind):
    if kind == "gauss":
        x = rng.standard_normal((n, d))
    else:
        x = rng.integers(-2, 3, (n, d)).astype(np.float64)     # integer values: exact ties everywhere
        if kind == "special":
            x[1] = 0.0                                          # a zero row
            x[2] = 1.5                                          # a constant row (correlation: NaN)
    return x.astype(dtype)


@pytest.mark.parametrize("metric", MR.EXTRA_METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_is_scikit_learn_bit_for_bit(metric, dtype):
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(abs(hash((metric, np.dtype(dtype).name))) % 2 ** 32)
    k = 8
    for d in DIMS:
        for kind in ("gauss", "int", "special"):
            x, y = _rows(rng, 12, d, dtype, kind), _rows(rng, 40, d, dtype, kind)
            V = rng.uniform(0.3, 3.0, d) if metric == "seuclidean" else None
            kw = {"metric_params": {"V": V}} if V is not None else {}
            sd, si = NearestNeighbors(n_neighbors=k, algorithm="brute", metric=metric, **kw).fit(y).kneighbors(x)
            out = MR.output_distance(metric, MR.ranking_values(metric, x, y, V), dtype)
            # the restated distance of every pair scikit-learn returned, bit for bit ...
            np.testing.assert_array_equal(np.take_along_axis(out, si, axis=1), sd, err_msg=f"{metric} {dtype} d={d} {kind}")
            # ... and scikit-learn returned the k smallest (NaN after every finite value)
            srt = np.sort(np.where(np.isnan(out), np.inf, out), axis=1)[:, :k]
            np.testing.assert_array_equal(np.where(np.isnan(sd), np.inf, sd), srt, err_msg=f"{metric} {dtype} d={d} {kind}")
            rd, ri = MR.knn(metric, x, y, k, V=V)
            np.testing.assert_array_equal(rd, sd)


def test_the_four_names_resolve():
    from kiez_amd.neighbors import SklearnNN, canonical_metric
    for m in MR.EXTRA_METRICS:
        assert canonical_metric(m) == m
        assert m in SklearnNN.valid_metrics
    nn = SklearnNN(metric="braycurtis")
    assert nn._metric_c == "braycurtis"
    SklearnNN(metric="correlation")
    SklearnNN(metric="hamming")
    SklearnNN(metric="seuclidean", metric_params={"V": [1.0, 2.0, 3.0]})


def test_native_metric_ids():
    from kiez_amd import _native as N
    assert (N.KZ_BRAYCURTIS, N.KZ_SEUCLIDEAN, N.KZ_CORRELATION, N.KZ_HAMMING) == (6, 7, 8, 9)
    assert {N.METRIC_IDS[m] for m in MR.EXTRA_METRICS} == {6, 7, 8, 9}
    assert "kz_matrix_set_seuclidean_v" in {s[0] for s in N.SYMBOLS}


def test_seuclidean_errors():
    from kiez_amd import Kiez
    from kiez_amd.neighbors import SklearnNN
    with pytest.raises(TypeError, match="V"):
        SklearnNN(metric="seuclidean")
    with pytest.raises(TypeError, match="V"):
        Kiez(algorithm="SklearnNN", algorithm_kwargs={"metric": "seuclidean"})
    with pytest.raises(NotImplementedError, match="metric_params"):
        SklearnNN(metric="seuclidean", metric_params={"V": [1.0], "w": [1.0]})
    for bad in ([1.0, 0.0], [1.0, -2.0], [1.0, np.inf], [np.nan, 1.0]):
        with pytest.raises(ValueError, match="finite and > 0"):
            SklearnNN(metric="seuclidean", metric_params={"V": bad})
    nn = SklearnNN(metric="seuclidean", metric_params={"V": [1.0, 2.0]})
    with pytest.raises(ValueError, match="entries"):                # (checked before anything touches the device)
        nn.fit(np.zeros((5, 3)))


def test_what_still_fails():
    from kiez_amd import Kiez
    from kiez_amd.neighbors import SklearnNN
    with pytest.raises(ValueError, match="not implemented"):
        SklearnNN(metric="canberra")
    with pytest.raises(NotImplementedError, match="metric_params"):
        SklearnNN(p=3, metric_params={"w": [1.0, 2.0]})
    with pytest.raises(NotImplementedError, match="metric_params"):
        SklearnNN(metric="braycurtis", metric_params={"V": [1.0, 2.0]})
    for m in MR.EXTRA_METRICS:
        kw = {"metric_params": {"V": [1.0]}} if m == "seuclidean" else {}
        with pytest.raises(ValueError, match="only supports"):
            Kiez(algorithm=SklearnNN(metric=m, **kw), hubness="DisSimLocal")


def test_sharded_kiez_takes_V():
    from kiez_amd.distributed import ShardedKiez
    with pytest.raises(TypeError, match="V"):
        ShardedKiez(n_candidates=5, algorithm_kwargs={"metric": "seuclidean"}, engine=object(), comm=object())
    sk = ShardedKiez(n_candidates=5, algorithm_kwargs={"metric": "seuclidean", "metric_params": {"V": [1.0, 2.0]}}, engine=object(),
                     comm=object())
    assert sk.V.tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="only supports"):
        ShardedKiez(n_candidates=5, algorithm_kwargs={"metric": "hamming"}, hubness="DisSimLocal", engine=object(), comm=object())
