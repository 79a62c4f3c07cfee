"""Gold ranks under a hubness reduction, the parts that need no GPU: the binding of kz_gold_ranks_reduced, the numpy restatement of
the reduced rank (tests/reduced_rank_restate.py) on ties, NaN and rows without gold and against the positions in the REFERENCE's own
full-length reduced lists (tests/golden/reduced_ranks.npz, tools/gen_golden_reduced_ranks.py), and the errors that come before
anything touches a device.  The device side: tests/test_gpu_reduced_ranks.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rank_restate as RR
from tests import reduced_rank_restate as RD

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "reduced_ranks.npz"
NO = RR.NO_GOLD


def distances(q, y, metric):
    """float64 distances as the search returns them for float64 input, restated in numpy."""
    q, y = np.asarray(q, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if metric == "euclidean":
        return np.sqrt(((q[:, None, :] - y[None, :, :]) ** 2).sum(axis=2))
    assert metric == "cosine"
    qn, yn = q / np.linalg.norm(q, axis=1)[:, None], y / np.linalg.norm(y, axis=1)[:, None]
    return 1.0 - qn @ yn.T


def test_symbol_is_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    for j, name in enumerate(("KZ_RANK_CSLS", "KZ_RANK_LS", "KZ_RANK_NICDM", "KZ_RANK_MP_NORMAL")):
        assert re.search(rf"^#define {name} {j + 1}$", header, flags=re.M), name
    assert (N.RANK_CSLS, N.RANK_LS, N.RANK_NICDM, N.RANK_MP_NORMAL) == (1, 2, 3, 4)
    assert [RD.kind_id(k) for k in RD.KINDS] == [1, 2, 3, 4]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint kz_gold_ranks_reduced\s*\(", header), "kz_gold_ranks_reduced is not declared in include/kiez_amd.h"
    bound = {s[0]: s for s in N.SYMBOLS}
    assert len(bound["kz_gold_ranks_reduced"][2]) == 12
    assert len(bound["kz_gold_ranks"][2]) == 7        # (the plain call keeps its signature)
    lib = N.load()
    assert hasattr(lib, "kz_gold_ranks_reduced")
    assert lib.kz_abi_version() == 7                  # (purely additive)
    assert callable(N.gold_ranks_reduced)
    assert list(inspect.signature(N.gold_ranks_reduced).parameters) == ["ctx", "query", "index", "gold_dev", "kind", "q_state",
                                                                         "t_state", "q_begin", "q_count"]


def test_restatement_edge_cases():
    nan = np.nan
    # CSLS with zero states: w = 2 d -- ties go by smaller row, NaN ranks as +inf by row, no gold gives -1
    d = np.array([[3.0, 1.0, 1.0, nan, 0.5, nan]])
    zq, zt = (np.zeros(6),), (np.zeros(6),)
    np.testing.assert_array_equal(RD.ranks("csls", np.repeat(d, 6, axis=0), zq, zt, np.arange(6)), [3, 1, 2, 4, 0, 5])
    np.testing.assert_array_equal(RD.ranks("csls", np.repeat(d, 6, axis=0), zq, zt, [NO, -1, 6, 0, 1, 2]), [-1, -1, -1, 3, 1, 2])
    # the index-side state decides between equal distances: row 2 has the larger mean, so the smaller CSLS value
    t = (np.array([0.0, 0.0, 0.5, 0.0, 0.0, 0.0]),)
    np.testing.assert_array_equal(RD.ranks("csls", d, (np.zeros(1),), t, [1]), [2])
    np.testing.assert_array_equal(RD.ranks("csls", d, (np.zeros(1),), t, [2]), [1])
    # a NaN state makes every w of the row NaN: all tie at +inf, the rank is the gold id
    np.testing.assert_array_equal(RD.ranks("csls", np.repeat(d, 3, axis=0), (np.full(3, nan),), zt, [0, 3, 5]), [0, 3, 5])
    # MP normal saturates at exactly 1.0 far beyond both lists: those pairs tie and go by row
    far = np.array([[0.1, 50.0, 60.0, 70.0]])
    w = RD.reduce("mp_normal", far, (np.array([1.0]), np.array([0.2])), (np.ones(4), np.full(4, 0.2)))
    assert w[0, 0] < 1.0 and (w[0, 1:] == 1.0).all()
    np.testing.assert_array_equal(RD.ranks("mp_normal", np.repeat(far, 3, axis=0), (np.ones(3), np.full(3, 0.2)),
                                           (np.ones(4), np.full(4, 0.2)), [3, 2, 1]), [3, 2, 1])
    # the bracket: everything strictly below w_g - tol counts, everything up to w_g + tol may
    lo, hi = RD.bracket(np.array([[0.0, 1.0, 1.0 + 1e-13, 2.0]]), [1], 1e-12)
    assert (lo[0], hi[0]) == (1, 2)


def test_restatement_is_the_position_in_the_references_reduced_list():
    g = np.load(GOLDEN)
    source, target, gold = g["source"], g["target"], g["gold"]
    n_s, n_t = source.shape[0], target.shape[0]
    assert (n_s, n_t, source.shape[1]) == (100, 80, 8) and source.dtype == np.float64
    assert (gold < 0).sum() >= 40 and (gold >= 0).sum() >= 50                  # rows without gold
    assert list(g["kinds"]) == list(RD.KINDS) and list(g["metrics"]) == ["euclidean", "cosine"]
    for metric in g["metrics"]:
        d = distances(source, target, str(metric))
        for kind in RD.KINDS:
            ind, clear = g[f"{metric}__{kind}__ind"].astype(np.int64), g[f"{metric}__{kind}__clear"]
            assert ind.shape == (n_s, n_t) and clear.sum() >= 0.9 * (gold >= 0).sum()      # the generator's condition
            # the reference's lists hold the whole index (n_candidates = n_target): the state is that of all distances
            q_state, t_state = RD.state(kind, RD.lists(d, n_t)), RD.state(kind, RD.lists(d.T, n_t))
            rank = RD.ranks(kind, d, q_state, t_state, gold)
            pos = RR.positions(ind, gold)
            np.testing.assert_array_equal(rank == -1, gold < 0)
            np.testing.assert_array_equal(rank[clear], pos[clear], err_msg=f"{metric} {kind}")
            assert pos[clear].max() >= 10 and (pos[clear] == 0).any()          # ranks from 0 to the tens


def test_errors_that_come_before_the_device():
    from kiez_amd import Kiez
    from kiez_amd.hubness_reduction import CSLS, HubnessReduction
    from kiez_amd.neighbors import NotFittedError, SklearnNN
    # reduced=True ranks one direction only
    kz = Kiez(n_candidates=3, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
    with pytest.raises(ValueError, match="s_to_t"):
        kz.gold_ranks({0: 1}, s_to_t=False, reduced=True)
    with pytest.raises(NotFittedError):
        kz.gold_ranks({0: 1}, reduced=True)
    with pytest.raises(NotFittedError):
        Kiez(n_candidates=3, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}).gold_ranks({0: 1}, reduced=True)
    # a single-source fit, without the device: what fit(source) leaves behind
    nn = kz.algorithm
    nn.source_index = nn.target_index = object()
    nn.source_ = nn.target_ = np.zeros((4, 3))
    nn.source_equals_target = True
    with pytest.raises(NotImplementedError, match="two-sided"):
        kz.gold_ranks({0: 1}, reduced=True)
    # a user-written reduction has no native rank
    class UserReduction(HubnessReduction):
        def _fit(self, *a):
            pass

        def transform(self, neigh_dist, neigh_ind, query):
            return neigh_dist, neigh_ind
    with pytest.raises(NotImplementedError, match="device-native"):
        UserReduction(nn_algo=SklearnNN(n_candidates=3, metric="euclidean")).gold_ranks({0: 1})
    assert "SEARCH METRIC" in Kiez.gold_ranks.__doc__ and "reduced=True" in Kiez.gold_ranks.__doc__
    assert "reduced=True" in SklearnNN.gold_ranks.__doc__
    assert "exactly 1.0" in HubnessReduction.gold_ranks.__doc__ and CSLS._no_rank_reason is None
