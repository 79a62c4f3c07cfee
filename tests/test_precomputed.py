"""metric='precomputed', the parts that need no GPU: the restatement (tests/precomputed_restate.py) against scikit-learn's
NearestNeighbors(metric="precomputed"), the binding of kz_matrix_create_precomputed, the metric list, construction, and the refusals
that come before any device work.  The device side: tests/test_gpu_precomputed.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import precomputed_restate as PR

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_agrees_with_scikit_learn(dtype):
    """scikit-learn's order among equal values is not defined: every row is a permutation of a grid, distinct by construction."""
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(7)
    n_q, n_index, k = 37, 129, 10
    D = PR.grid_rows(rng, n_q, n_index, dtype)
    assert D.dtype == dtype
    for row in D:
        assert np.unique(row).size == n_index          # (asserted, not assumed: the comparison below is exact)
    nn = NearestNeighbors(n_neighbors=k, metric="precomputed", algorithm="brute")
    nn.fit(np.zeros((n_index, n_index), dtype=dtype))   # (a dummy square matrix: fit only records n_samples_fit)
    sk_dist, sk_ind = nn.kneighbors(D, n_neighbors=k)
    dist, ind = PR.knn(D, k)
    np.testing.assert_array_equal(ind, sk_ind)
    np.testing.assert_array_equal(dist, sk_dist.astype(np.float64))
    assert sk_dist.dtype == dtype                      # scikit-learn returns the matrix' dtype: what SklearnNN._out_dtype mirrors
    # the other direction is the same statement on the transpose
    Dt = PR.grid_rows(rng, n_index, n_q, dtype)         # columns are not permutations here: use the rows of the transpose
    dist_t, ind_t = PR.knn(np.ascontiguousarray(Dt.T), 5, s_to_t=False)
    dist_r, ind_r = PR.knn_rows(Dt, 5)
    np.testing.assert_array_equal(ind_t, ind_r)
    np.testing.assert_array_equal(dist_t, dist_r)


def test_restatement_orders_ties_by_column_and_ranks_are_positions():
    rng = np.random.default_rng(3)
    D = rng.integers(0, 5, size=(9, 40)).astype(np.float64)
    dist, ind = PR.knn(D, 40)
    for i in range(9):
        pairs = list(zip(dist[i], ind[i]))
        assert pairs == sorted(pairs)
    gold = rng.integers(0, 40, size=9)
    gold[::3] = -1
    r = PR.ranks(D, gold)
    for i in range(9):
        assert r[i] == (-1 if gold[i] < 0 else int(np.nonzero(ind[i] == gold[i])[0][0]))


def test_out_dtype_follows_the_matrix():
    from kiez_amd.neighbors import SklearnNN

    class _M:
        def __init__(self, dtype):
            self.dtype = np.dtype(dtype)
    nn = SklearnNN(metric="precomputed")
    assert nn._out_dtype(_M(np.float32)) == np.float32 and nn._out_dtype(_M(np.float64)) == np.float64


def test_symbol_is_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    assert re.search(r"\bKZ_YULE = 16, KZ_PRECOMPUTED = 17\b", header)
    assert N.KZ_PRECOMPUTED == 17 and "precomputed" not in N.METRIC_IDS     # (kz_matrix_create keeps refusing the id)
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint kz_matrix_create_precomputed\s*\(([^)]*)\)", stripped)
    assert decl, "kz_matrix_create_precomputed is not declared in include/kiez_amd.h"
    assert len(decl.group(1).split(",")) == 8
    bound = {s[0]: s for s in N.SYMBOLS}
    assert len(bound["kz_matrix_create_precomputed"][2]) == 8
    assert len(bound["kz_matrix_create"][2]) == 8                           # (keeps its signature)
    lib = N.load()
    assert hasattr(lib, "kz_matrix_create_precomputed")
    assert re.search(r"^#define KZ_ABI_VERSION 7$", header, flags=re.M)
    assert N.ABI_VERSION == 7 and lib.kz_abi_version() == 7                 # (purely additive)
    makefile = (ROOT / "kiez_amd" / "csrc" / "Makefile").read_text()
    assert "kz_precomputed.hip" in makefile and "kz_precomputed.h " in makefile


def test_valid_metrics_sorted_and_contain_precomputed():
    from kiez_amd.neighbors import SklearnNN, canonical_metric
    assert SklearnNN.valid_metrics == sorted(SklearnNN.valid_metrics)
    assert "precomputed" in SklearnNN.valid_metrics
    assert canonical_metric("precomputed") == "precomputed"


def test_construction():
    """Raises ValueError without the feature: canonical_metric refused the name."""
    from kiez_amd import Kiez
    from kiez_amd.neighbors import SklearnNN
    nn = SklearnNN(n_candidates=7, metric="precomputed")
    assert nn._metric_c == "precomputed" and nn.metric == "precomputed"
    for hubness in (None, "CSLS", "LocalScaling", "MutualProximity"):
        kz = Kiez(n_candidates=7, algorithm="SklearnNN", algorithm_kwargs={"metric": "precomputed"}, hubness=hubness)
        assert kz.algorithm._metric_c == "precomputed"


def test_refusals_come_before_the_device(monkeypatch):
    from kiez_amd import Kiez, Sinkhorn
    from kiez_amd import _native as N
    from kiez_amd.distributed import ShardedKiez
    from kiez_amd.hubness_reduction import DisSimLocal
    from kiez_amd.neighbors import SklearnNN

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N.Context, "__init__", no_device)
    D = np.zeros((4, 3))
    # fit(D, target): one matrix only
    nn = SklearnNN(n_candidates=2, metric="precomputed")
    with pytest.raises(ValueError, match="ONE distance matrix"):
        nn.fit(D, np.zeros((3, 3)))
    assert not hasattr(nn, "source_index")
    for hubness in (None, "CSLS", Sinkhorn):
        with pytest.raises(ValueError, match="ONE distance matrix"):
            Kiez(n_candidates=2, algorithm_kwargs={"metric": "precomputed"}, hubness=hubness).fit(D, np.zeros((3, 3)))
    # DisSimLocal needs embeddings
    with pytest.raises(ValueError, match="DisSimLocal only supports squared Euclidean"):
        DisSimLocal(nn_algo=SklearnNN(n_candidates=2, metric="precomputed"))
    with pytest.raises(ValueError, match="DisSimLocal only supports squared Euclidean"):
        Kiez(n_candidates=2, algorithm_kwargs={"metric": "precomputed"}, hubness="DisSimLocal")
    # one GPU
    with pytest.raises(ValueError, match="one GPU"):
        ShardedKiez(n_candidates=2, algorithm_kwargs={"metric": "precomputed"}, hubness=None)
    with pytest.raises(ValueError, match="one GPU"):
        ShardedKiez(n_candidates=2, algorithm_kwargs={"metric": "precomputed"}, hubness="CSLS")
    # no metric parameters
    with pytest.raises(NotImplementedError, match="metric_params"):
        SklearnNN(metric="precomputed", metric_params={"V": np.ones(3)})
