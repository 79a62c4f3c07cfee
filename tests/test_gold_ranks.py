"""Exact gold ranks, the parts that need no GPU: the binding of kz_gold_ranks / kz_rank_stats, the host semantics of
evaluate.rank_metrics, the numpy restatement of the rank (tests/rank_restate.py) against scikit-learn's full-length brute-force
lists and against the reference's own lists and hits (tests/golden/full_ranks.npz, tools/gen_golden_ranks.py), and the errors of
unfitted / single-source use.  The device side: tests/test_gpu_gold_ranks.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rank_restate as RR

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "full_ranks.npz"


def _values(q, y, metric):
    """float64 values the search ranks by, restated in numpy (inputs converted to float64 first, as the exact kernels do)."""
    q, y = np.asarray(q, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if metric == "euclidean":
        return ((q[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    if metric == "manhattan":
        return np.abs(q[:, None, :] - y[None, :, :]).sum(axis=2)
    assert metric == "cosine"
    qn, yn = q / np.linalg.norm(q, axis=1)[:, None], y / np.linalg.norm(y, axis=1)[:, None]
    return 1.0 - qn @ yn.T


def test_symbols_are_declared_and_bound():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {s[0]: s for s in N.SYMBOLS}
    for name in ("kz_gold_ranks", "kz_rank_stats"):
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/kiez_amd.h"
        assert name in bound, f"{name} has no ctypes prototype"
    assert len(bound["kz_gold_ranks"][2]) == 7
    lib = N.load()
    assert hasattr(lib, "kz_gold_ranks") and hasattr(lib, "kz_rank_stats")
    assert lib.kz_abi_version() == 7                  # (purely additive)
    assert callable(N.gold_ranks) and callable(N.rank_stats)


@pytest.fixture()
def host_reduction(monkeypatch):
    """rank_metrics with the device reduction (kz_rank_stats) replaced by its numpy restatement: the host semantics alone."""
    from kiez_amd import evaluate as E
    monkeypatch.setattr(E, "_rank_stats", lambda ranks, ks, ctx: RR.rank_stats(np.asarray(ranks), ks))
    return E


def test_rank_metrics_host_semantics(host_reduction):
    E = host_reduction
    ranks = np.array([0, 4, -1, 9, 10, 0, 123456, -1], dtype=np.int64)
    # six pairs have a rank, two rows have none; the dict also holds two pairs whose keys are no rows: len(gold) = 8
    gold = {0: 5, 1: 7, 3: 2, 4: 4, 5: 0, 6: 9, 100: 1, 101: 3}
    m = E.rank_metrics(ranks, gold, k=[10, 1, 5, 200000])
    assert list(m["hits"]) == [1, 5, 10, 200000]
    assert m["hits"] == {1: 2 / 8, 5: 3 / 8, 10: 4 / 8, 200000: 6 / 8}
    assert m["n_ranked"] == 6 and m["n_gold"] == 8
    assert m["mr"] == (1 + 5 + 10 + 11 + 1 + 123457) / 6
    assert m["mrr"] == pytest.approx((1 + 1 / 5 + 1 / 10 + 1 / 11 + 1 + 1 / 123457) / 6, rel=1e-15)
    # default k, array gold (-1: none): the denominator is the number of gold ids
    m = E.rank_metrics(ranks, np.array([5, 7, -1, 2, 4, 0, 9, -1]))
    assert m["hits"] == {1: 2 / 6, 5: 3 / 6, 10: 4 / 6} and m["n_gold"] == 6
    # nothing ranked
    m = E.rank_metrics(np.array([-1, -1], dtype=np.int64), {0: 1, 1: 0}, k=[1])
    assert m["hits"] == {1: 0.0} and m["n_ranked"] == 0 and np.isnan(m["mr"]) and np.isnan(m["mrr"])


def test_rank_metrics_rejects_what_is_no_rank_vector():
    from kiez_amd import evaluate as E
    with pytest.raises(ValueError, match="one-dimensional"):
        E.rank_metrics(np.zeros((2, 2), dtype=np.int64), {0: 1})
    with pytest.raises(ValueError, match="one-dimensional"):
        E.rank_metrics(np.array([0.5, 1.0]), {0: 1})


def test_rank_metrics_agrees_with_hits_semantics(host_reduction):
    """hits@k from ranks = the reference's hits on the full-length list, on the literal example of its docstring."""
    E = host_reduction
    nn_ind = np.array([[1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 6]])
    gold = {0: 2, 1: 4, 2: 3, 3: 4}
    ranks = RR.positions(nn_ind, np.array([2, 4, 3, 4]))
    assert E.rank_metrics(ranks, gold)["hits"] == {1: 0.5, 5: 1.0, 10: 1.0}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "manhattan"])
def test_restatement_is_the_position_in_sklearns_full_list(metric, dtype):
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.RandomState(42)          # (the reference's own fixture shapes, tests/conftest.py)
    q = rng.rand(20, 5).astype(dtype)
    y = rng.rand(50, 5).astype(dtype)
    gold = (7 * np.arange(20) + 3) % 50
    ind = NearestNeighbors(n_neighbors=50, algorithm="brute", metric=metric).fit(y).kneighbors(q, return_distance=False)
    rank = RR.gold_ranks(_values(q, y, metric), gold)
    np.testing.assert_array_equal(rank, RR.positions(ind, gold))
    np.testing.assert_array_equal(RR.full_order(_values(q, y, metric)), ind)


def test_restatement_edge_cases():
    nan = np.nan
    vals = np.array([[3.0, 1.0, 1.0, nan, 0.5, nan],
                     [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    # ties by smaller row; NaN as +inf, by row
    np.testing.assert_array_equal(RR.gold_ranks(np.repeat(vals[:1], 6, axis=0), np.arange(6)), [3, 1, 2, 4, 0, 5])
    np.testing.assert_array_equal(RR.gold_ranks(vals, [2, 4]), [2, 4])
    np.testing.assert_array_equal(RR.gold_ranks(vals, [RR.NO_GOLD, 6]), [-1, -1])
    np.testing.assert_array_equal(RR.gold_ranks(vals, [-1, 5]), [-1, 5])


def test_restatement_against_the_reference_golden(host_reduction):
    E = host_reduction
    g = np.load(GOLDEN)
    source, target = g["source"], g["target"]
    n_s, n_t = source.shape[0], target.shape[0]
    gold = {int(a): int(b) for a, b in zip(g["gold_keys"], g["gold_vals"])}
    gold_vec = E._gold_vector(gold, n_s)
    assert (gold_vec == RR.NO_GOLD).sum() >= 5 and max(gold) >= n_s          # rows without gold; a key that is no row
    ks = [int(k) for k in g["ks"]]
    assert ks == [1, 5, 10, n_t]
    for metric in g["metrics"]:
        ind = g[f"{metric}__ind"].astype(np.int64)
        pos = RR.positions(ind, gold_vec)
        assert pos.max() >= 10 and (pos == 0).any()                           # ranks from 0 to the tens
        rank = RR.gold_ranks(_values(source, target, str(metric)), gold_vec)
        np.testing.assert_array_equal(rank, pos)
        m = E.rank_metrics(rank, gold, k=ks)
        np.testing.assert_array_equal([m["hits"][k] for k in ks], g[f"{metric}__hits"])
        assert m["n_gold"] == len(gold) and m["n_ranked"] == (pos >= 0).sum()
        assert m["mr"] == pytest.approx((pos[pos >= 0] + 1).mean(), rel=1e-15)


def test_unfitted_and_single_source_use_raise():
    """Both checks come before anything touches a device."""
    from kiez_amd.neighbors import NotFittedError, SklearnNN
    nn = SklearnNN(n_candidates=3, metric="euclidean")
    with pytest.raises(NotFittedError, match="not fitted"):
        nn.gold_ranks({0: 1})
    # a single-source fit, without the device: what fit(source) leaves behind
    nn.source_index = nn.target_index = object()
    nn.source_ = nn.target_ = np.zeros((4, 3))
    nn.source_equals_target = True
    with pytest.raises(NotImplementedError, match="two-sided"):
        nn.gold_ranks({0: 1})
    from kiez_amd import Kiez
    assert "SEARCH METRIC" in Kiez.gold_ranks.__doc__ and "SEARCH METRIC" in SklearnNN.gold_ranks.__doc__
    with pytest.raises(NotFittedError):
        Kiez(algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}).gold_ranks({0: 1})
