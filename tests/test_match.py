"""One-to-one matching, the part that needs no GPU: the ABI entry and the public signatures, the numpy restatement against itself
(Gale-Shapley == greedy on sorted rows, stability, independence of the proposal order, the ordering rule, a displacement chain
written out by hand) and the errors that are raised before the device is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import match_restate as MR

ROOT = Path(__file__).resolve().parent.parent

# A = 0, B = 1, C = 2 propose to X = 0, Y = 1.  A takes X, B takes Y; C loses Y to B (0.7 > 0.5), takes X from A (0.8 < 0.9); A takes Y
# from B (0.3 < 0.5); B loses X to C (0.95 > 0.8) and stays unmatched.
CHAIN_DIST = np.array([[0.9, 0.3], [0.5, 0.95], [0.7, 0.8]])
CHAIN_IND = np.array([[0, 1], [1, 0], [1, 0]], dtype=np.int64)
CHAIN_MATCH = np.array([1, -1, 0], dtype=np.int64)
CHAIN_COL = np.array([1, -1, 1], dtype=np.int64)


def random_lists(rng, n_q, n_index, k, ascending=True, dtype=np.float64, pad=0.0, ties=False):
    """Random lists: ids drawn per row without repetition where n_index allows, values sorted per row (`ascending`) or left in
    random column order; `pad`: the share of entries turned into no-pairs (-1, n_index, INT_MAX); `ties`: few distinct values."""
    if k <= n_index:
        ind = np.argsort(rng.random((n_q, n_index)), axis=1)[:, :k].astype(np.int64)
    else:
        ind = rng.integers(0, n_index, (n_q, k), dtype=np.int64)
    dist = (rng.integers(0, 4, (n_q, k)) / 4.0 if ties else rng.standard_normal((n_q, k))).astype(dtype)
    if ascending:
        dist = np.sort(dist, axis=1)
    if pad:
        holes = rng.random((n_q, k)) < pad
        ind[holes] = rng.choice(np.array([-1, n_index, 0x7fffffff], dtype=np.int64), int(holes.sum()))
    return dist, ind


def assert_same(a, b, what=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"match {what}")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"col {what}")


def test_entry_point_is_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kiez_amd.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+kz_match_lists\s*\(([^)]*)\)", header)
    assert decl and decl.group(1).count(",") == 9
    bound = {s[0]: s for s in N.SYMBOLS}
    assert len(bound["kz_match_lists"][2]) == 10 and bound["kz_match_lists"][1] is ctypes.c_int
    lib = N.load()
    assert hasattr(lib, "kz_match_lists")
    assert lib.kz_abi_version() == 7


def test_public_signatures():
    from kiez_amd import Kiez, matching
    sig = inspect.signature(matching.one_to_one)
    assert list(sig.parameters) == ["dist", "ind", "n_target", "return_distance", "ctx"]
    assert sig.parameters["return_distance"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["return_distance"].default is True
    assert sig.parameters["ctx"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ctx"].default is None
    sig = inspect.signature(Kiez.match)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("k", None), ("whole_index", False), ("return_distance", True)]
    sig = inspect.signature(Kiez.match_device)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("k", None), ("whole_index", False)]
    import kiez_amd
    assert kiez_amd.matching is matching


@pytest.mark.parametrize("n_q,n_index,k", [(1, 1, 1), (40, 40, 40), (90, 20, 20), (20, 90, 7), (300, 300, 10), (50, 10, 30)])
def test_gale_shapley_is_greedy_on_sorted_rows(n_q, n_index, k):
    for seed, ties, pad in ((0, False, 0.0), (1, True, 0.0), (2, False, 0.2), (3, True, 0.2)):
        dist, ind = random_lists(np.random.default_rng(seed), n_q, n_index, k, ties=ties, pad=pad)
        gs = MR.gale_shapley(dist, ind, n_index)
        assert_same(gs, MR.greedy(dist, ind, n_index), f"seed {seed}")
        assert MR.blocking_pairs(dist, ind, n_index, gs) == []


@pytest.mark.parametrize("n_q,n_index,k", [(40, 40, 40), (90, 20, 20), (20, 90, 7), (300, 300, 10), (50, 10, 30)])
def test_gale_shapley_is_stable_and_order_free_on_shuffled_columns(n_q, n_index, k):
    for seed, ties, pad in ((0, False, 0.0), (1, True, 0.0), (2, False, 0.2), (3, True, 0.2)):
        dist, ind = random_lists(np.random.default_rng(seed), n_q, n_index, k, ascending=False, ties=ties, pad=pad)
        gs = MR.gale_shapley(dist, ind, n_index)
        assert MR.blocking_pairs(dist, ind, n_index, gs) == []
        assert_same(gs, MR.gale_shapley(dist, ind, n_index, descending=True), f"seed {seed}")
        m = gs[0][gs[0] >= 0]
        assert len(np.unique(m)) == len(m)
        assert (ind[np.arange(n_q), gs[1]][gs[0] >= 0] == m).all()


def test_blocking_pairs_finds_one():
    # the chain case with B left on Y: A, displaced from X by C, prefers Y and Y prefers A
    assert MR.blocking_pairs(CHAIN_DIST, CHAIN_IND, 2, (np.array([-1, 1, 0]), np.array([-1, 0, 1]))) == [(0, 1)]


def test_displacement_chain():
    for descending in (False, True):
        match, col = MR.gale_shapley(CHAIN_DIST, CHAIN_IND, 2, descending=descending)
        np.testing.assert_array_equal(match, CHAIN_MATCH)
        np.testing.assert_array_equal(col, CHAIN_COL)
    assert MR.blocking_pairs(CHAIN_DIST, CHAIN_IND, 2, (CHAIN_MATCH, CHAIN_COL)) == []


def test_ordering_rule():
    inf, nan = np.inf, np.nan
    k = MR.key(np.array([-inf, -2.0, -0.0, 0.0, 1.0, inf, nan]))
    assert k[0] < k[1] < k[2] == k[3] < k[4] < k[5] == k[6] and k.dtype == np.uint64
    assert MR.key(np.float32(-1.5)) == MR.key(-1.5)
    one = np.zeros((3, 1), dtype=np.int64)
    # all values equal: the smallest source row
    np.testing.assert_array_equal(MR.gale_shapley(np.full((3, 1), 1.0), one, 1)[0], [0, -1, -1])
    # NaN ties with +inf and loses to it only by row; any finite value beats both
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[nan], [inf], [inf]]), one, 1)[0], [0, -1, -1])
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[inf], [nan], [nan]]), one, 1)[0], [0, -1, -1])
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[nan], [inf], [1e308]]), one, 1)[0], [-1, -1, 0])
    # -0.0 ties with +0.0: by row
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[0.0], [-0.0], [0.0]]), one, 1)[0], [0, -1, -1])
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[1e-300], [0.0], [-0.0]]), one, 1)[0], [-1, 0, -1])
    # -inf wins
    np.testing.assert_array_equal(MR.gale_shapley(np.array([[-1e308], [-0.0], [-inf]]), one, 1)[0], [-1, -1, 0])


def test_argument_errors_come_before_the_device(monkeypatch):
    from kiez_amd import _native as N
    from kiez_amd import matching

    def no_device(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N, "load", no_device)
    d, i = np.zeros((4, 3)), np.zeros((4, 3), dtype=np.int64)
    bad = [(d[0], i[0], 5), (d[:, :, None], i[:, :, None], 5), (d, i[:, :2], 5), (d, i[:3], 5),      # not 2-D, unequal shapes
           (d, i.astype(np.float64), 5), (d, i.astype(bool), 5),                                      # ind not integer
           (d.astype(np.int64), i, 5), (d.astype(complex), i, 5),                                     # dist not floating point
           (d, i, 0), (d, i, -3), (d, i, 2.0), (d, i, True), (d, i, None), (d, i, "7")]               # n_target not a positive int
    for dist, ind, n_target in bad:
        with pytest.raises(ValueError):
            matching.one_to_one(dist, ind, n_target)
    with pytest.raises(AssertionError, match="the device was touched"):    # (valid arguments do go to the device)
        matching.one_to_one(d, i, 5)


def test_unfitted_and_missing_k():
    from kiez_amd import Kiez, NotFittedError
    for hubness in (None, "CSLS"):
        with pytest.raises(NotFittedError):
            Kiez(hubness=hubness).match(3)
        with pytest.raises(NotFittedError):
            Kiez(hubness=hubness).match_device(3)
        with pytest.raises(ValueError) as want:
            Kiez(hubness=hubness).kneighbors_whole_index(None)
        with pytest.raises(ValueError) as got:
            Kiez(hubness=hubness).match(whole_index=True)
        assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
