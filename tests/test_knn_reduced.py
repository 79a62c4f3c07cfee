"""Neighbour lists by the hubness-reduced distance over the whole index, the parts that need no GPU: the binding of kz_knn_reduced,
the numpy restatement (tests/whole_index_restate.py) on ties, NaN, infinities and signed zeros and against the ranks of
tests/reduced_rank_restate.py, and the errors that come before anything touches a device.  The device side:
tests/test_gpu_knn_reduced.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import reduced_rank_restate as RD
from tests import whole_index_restate as WI

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    assert re.search(r"^#define KZ_KNN_REDUCED_MAX_K 512$", header, flags=re.M)
    assert N.KNN_REDUCED_MAX_K == 512
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint kz_knn_reduced\s*\(", header), "kz_knn_reduced is not declared in include/kiez_amd.h"
    bound = {s[0]: s for s in N.SYMBOLS}
    assert len(bound["kz_knn_reduced"][2]) == 13
    assert len(bound["kz_gold_ranks_reduced"][2]) == 12      # (the rank call keeps its signature)
    lib = N.load()
    assert hasattr(lib, "kz_knn_reduced")
    assert lib.kz_abi_version() == 7                         # (purely additive)
    assert list(inspect.signature(N.knn_reduced).parameters) == ["ctx", "query", "index", "k", "kind", "q_state", "t_state", "q_begin",
                                                                 "q_count"]


def test_restatement_edge_cases():
    nan, inf = np.nan, np.inf
    # ties go by smaller row
    w, ind = WI.topk(np.array([[3.0, 1.0, 1.0, 0.5, 1.0]]), 4)
    np.testing.assert_array_equal(ind, [[3, 1, 2, 4]])
    np.testing.assert_array_equal(w, [[0.5, 1.0, 1.0, 1.0]])
    # NaN and +inf tie by row and come last; a NaN is returned as NaN
    w, ind = WI.topk(np.array([[nan, 2.0, inf, nan, -1.0, inf]]), 6)
    np.testing.assert_array_equal(ind, [[4, 1, 0, 2, 3, 5]])
    np.testing.assert_array_equal(w, [[-1.0, 2.0, nan, inf, nan, inf]])
    assert WI.non_decreasing(w)
    # -inf is an ordinary smallest value
    w, ind = WI.topk(np.array([[0.0, -inf, -5.0, -inf]]), 3)
    np.testing.assert_array_equal(ind, [[1, 3, 2]])
    # -0.0 == +0.0: by row, whichever sign comes first
    w, ind = WI.topk(np.array([[0.0, -0.0, 0.0, -0.0, -1e-300]]), 5)
    np.testing.assert_array_equal(ind, [[4, 0, 1, 2, 3]])
    assert not WI.non_decreasing(np.array([[1.0, nan, 2.0]])) and WI.non_decreasing(np.array([[-inf, -0.0, 0.0, nan, inf]]))


@pytest.mark.parametrize("kind", RD.KINDS)
def test_position_in_the_restated_list_is_the_restated_rank(kind):
    """For every column c, the rank of tests/reduced_rank_restate.py of the row at column c is c -- with duplicates, NaN states and,
    for CSLS, infinite ones."""
    rng = np.random.default_rng(5)
    n_q, n_i, k = 12, 40, 40
    d = rng.random((n_q, n_i)) * 3.0
    d[:, 7] = d[:, 3]                                          # equal distances ...
    q_state = tuple(rng.random(n_q) + 0.5 for _ in range(2 if kind == "mp_normal" else 1))
    t_state = tuple(rng.random(n_i) + 0.5 for _ in range(2 if kind == "mp_normal" else 1))
    for s in t_state:
        s[7] = s[3]                                            # ... and equal states: equal w
    t_state[0][11] = t_state[0][30] = np.nan
    if kind == "csls":
        t_state[0][5], t_state[0][20], t_state[0][21] = np.inf, -np.inf, -np.inf
    w, ind = WI.knn_reduced(kind, d, q_state, t_state, k)
    assert WI.non_decreasing(w) and all(sorted(r) == list(range(n_i)) for r in ind.tolist())
    assert np.isnan(w).sum() == 2 * n_q
    for c in range(k):
        np.testing.assert_array_equal(RD.ranks(kind, d, q_state, t_state, ind[:, c]), np.full(n_q, c), err_msg=f"column {c}")
    assert (np.abs(np.argmax(ind == 3, axis=1) - np.argmax(ind == 7, axis=1)) == 1).all()       # the tie sits side by side, 3 first
    assert (np.argmax(ind == 3, axis=1) < np.argmax(ind == 7, axis=1)).all()


def test_errors_that_come_before_the_device():
    from kiez_amd import Kiez
    from kiez_amd.hubness_reduction import HubnessReduction
    from kiez_amd.neighbors import NotFittedError, SklearnNN

    def kiez(hubness):
        return Kiez(n_candidates=3, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hubness)
    kz = kiez("CSLS")
    # k is a required positive int
    with pytest.raises(TypeError):
        kz.kneighbors_whole_index()
    for bad in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="positive integer"):
            kz.kneighbors_whole_index(bad)
        with pytest.raises(ValueError, match="positive integer"):
            kiez(None).kneighbors_whole_index(bad)
    # unfitted
    with pytest.raises(NotFittedError):
        kz.kneighbors_whole_index(2)
    with pytest.raises(NotFittedError):
        kz.kneighbors_whole_index_device(2)
    with pytest.raises(NotFittedError):
        kiez(None).kneighbors_whole_index(2)
    # a single-source fit, without the device: what fit(source) leaves behind
    nn = kz.algorithm
    nn.source_index = nn.target_index = object()
    nn.source_ = nn.target_ = np.zeros((4, 3))
    nn.source_equals_target = True
    with pytest.raises(NotImplementedError, match="two-sided"):
        kz.kneighbors_whole_index(2)
    # a user-written reduction has no value outside its list
    class UserReduction(HubnessReduction):
        def _fit(self, *a):
            pass

        def transform(self, neigh_dist, neigh_ind, query):
            return neigh_dist, neigh_ind
    with pytest.raises(NotImplementedError, match="device-native"):
        UserReduction(nn_algo=SklearnNN(n_candidates=3, metric="euclidean")).kneighbors_whole_index(2)
    assert "WHOLE" in Kiez.kneighbors_whole_index.__doc__ and "n_candidates" in Kiez.kneighbors_whole_index.__doc__
    assert list(inspect.signature(Kiez.kneighbors).parameters) == ["self", "k", "return_distance"]     # (kneighbors keeps its signature)
    assert list(inspect.signature(Kiez.kneighbors_whole_index).parameters) == ["self", "k", "return_distance"]
