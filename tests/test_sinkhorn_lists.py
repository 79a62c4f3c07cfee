"""Sinkhorn and the inverted softmax on the candidate lists, the parts that need no GPU: the binding of the four entry points of
kz_softmin_lists.hip, the chunk constant, the `support` argument and its constructor errors, and the numpy restatement
(tests/sinkhorn_lists_restate.py): its two forms against each other and the hits@1 figures the documentation quotes.  The device side:
tests/test_gpu_sinkhorn_lists.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sinkhorn_lists_restate as LR
from tests import sinkhorn_restate as SR

ROOT = Path(__file__).resolve().parent.parent

# (n_s, n_t, eps, L, noise): tests/test_gpu_sinkhorn.py's FIT_CASES
FIT_CASES = [(200, 200, 0.1, 50, 0.3), (180, 257, 0.05, 50, 0.3), (300, 300, 0.02, 100, 1.0)]


def test_symbols_are_declared_bound_and_exported():
    from kiez_amd import _native as N
    from kiez_amd import matching
    text = (ROOT / "include" / "kiez_amd.h").read_text()
    chunk = re.search(r"^#define KZ_SOFTMIN_LIST_CHUNK (\d+)\b", text, flags=re.M)
    assert chunk and int(chunk.group(1)) == N.SOFTMIN_LIST_CHUNK
    source = (ROOT / "kiez_amd" / "csrc" / "kz_softmin_lists.hip").read_text()
    assert re.search(rf"constexpr int KZ_SL_CHUNK = {N.SOFTMIN_LIST_CHUNK};", source)
    assert "static_assert(KZ_SL_CHUNK == KZ_SOFTMIN_LIST_CHUNK" in source
    assert "kz_softmin_lists.hip" in (ROOT / "kiez_amd" / "csrc" / "Makefile").read_text()
    assert "NaN" in text[text.index("CANDIDATE LISTS"):text.index("int kz_lists_transpose")]           # (the header says what "no pair" gives)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {s[0]: s for s in N.SYMBOLS}
    lib = N.load()
    for name, n_args in (("kz_lists_transpose", 10), ("kz_softmin_list_rows", 10), ("kz_softmin_list_cols", 10), ("kz_sinkhorn_lists", 14)):
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/kiez_amd.h"
        assert len(bound[name][2]) == n_args
        assert hasattr(lib, name)
    assert len(bound["kz_softmin_rows"][2]) == 9 and N.SOFTMIN_CHUNK == 4096                             # (the whole-index call keeps its own)
    assert re.search(r"^#define KZ_ABI_VERSION 7$", text, flags=re.M)
    assert N.ABI_VERSION == 7 and lib.kz_abi_version() == 7                                              # (purely additive)
    assert list(inspect.signature(N.lists_transpose).parameters) == ["ctx", "dist", "ind", "n_index"]
    assert list(inspect.signature(N.softmin_list_rows).parameters) == ["ctx", "dist", "ind", "n_index", "eps", "off", "shift"]
    assert list(inspect.signature(N.softmin_list_cols).parameters) == ["ctx", "view", "eps", "off", "shift"]
    assert list(inspect.signature(N.sinkhorn_lists).parameters) == ["ctx", "dist", "ind", "n_index", "eps", "n_iter", "tol"]
    sig = inspect.signature(matching.sinkhorn_lists)
    assert list(sig.parameters) == ["dist", "ind", "n_target", "temperature", "n_iter", "tol", "ctx", "return_info"]
    assert [sig.parameters[p].default for p in ("temperature", "n_iter", "tol", "ctx", "return_info")] == [0.05, 10, None, None, False]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("temperature", "n_iter", "tol", "ctx", "return_info"))


def test_support_is_validated_before_the_device_and_the_defaults_stay(monkeypatch):
    from kiez_amd import InvertedSoftmax, Kiez, Sinkhorn, matching
    from kiez_amd import _native as N
    from kiez_amd.hubness_reduction import HubnessReduction
    from kiez_amd.neighbors import SklearnNN

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N.Context, "__init__", no_device)
    nn = lambda: SklearnNN(n_candidates=5, metric="cosine")   # noqa: E731
    for cls in (Sinkhorn, InvertedSoftmax):
        assert inspect.signature(cls.__init__).parameters["support"].default == "index"
        assert cls(nn_algo=nn()).support == "index" and cls(support="candidates", nn_algo=nn()).support == "candidates"
        assert Kiez(hubness=cls, hubness_kwargs={"support": "candidates"}).hubness.support == "candidates"
        for bad in ("lists", "Index", "", None, 1, True, b"index", ("index",)):
            with pytest.raises(ValueError, match="support"):
                cls(support=bad, nn_algo=nn())
            with pytest.raises(ValueError, match="support"):
                Kiez(hubness=cls, hubness_kwargs={"support": bad})
        for support in ("index", "candidates"):
            assert "temperature = 0.05" in repr(cls(support=support, nn_algo=nn())) and support in repr(cls(support=support, nn_algo=nn()))
            with pytest.raises(ValueError, match="two-sided data only"):
                cls(support=support, nn_algo=nn()).fit(np.zeros((4, 3)))
        # everything that ranks stays the base class's
        for inherited in ("kneighbors", "kneighbors_device", "kneighbors_whole_index", "kneighbors_whole_index_device", "gold_ranks",
                          "gold_ranks_device"):
            assert getattr(cls, inherited) is getattr(HubnessReduction, inherited)
    # the defaults of both classes are unchanged
    hub = Sinkhorn(nn_algo=nn())
    assert (hub.temperature, hub.n_iter, hub.tol, hub.support) == (0.05, 10, None, "index")
    assert list(inspect.signature(Sinkhorn.__init__).parameters)[:4] == ["self", "temperature", "n_iter", "tol"]
    assert InvertedSoftmax(nn_algo=nn()).temperature == 0.05
    # matching.sinkhorn_lists: the list checks of one_to_one and its own, all before the device
    d, i = np.zeros((4, 2)), np.zeros((4, 2), dtype=np.int64)
    for kw, what in (({"temperature": 0}, "temperature"), ({"temperature": np.nan}, "temperature"), ({"temperature": True}, "temperature"),
                     ({"n_iter": 0}, "n_iter"), ({"n_iter": 2.0}, "n_iter"), ({"tol": -1e-9}, "tol"), ({"tol": "0.1"}, "tol")):
        with pytest.raises(ValueError, match=what):
            matching.sinkhorn_lists(d, i, 3, **kw)
    with pytest.raises(ValueError, match="n_target"):
        matching.sinkhorn_lists(d, i, 0)
    with pytest.raises(ValueError, match="one shape"):
        matching.sinkhorn_lists(d, i[:3], 3)
    with pytest.raises(ValueError, match="integer row ids"):
        matching.sinkhorn_lists(d, d, 3)


def _case_lists(case, K):
    n_s, n_t, eps, L, noise = case
    s, t, gold = SR.alignment_case(n_s, n_t, noise)
    D = 1.0 - s @ t.T
    return D, gold, LR.candidate_lists(D, K)


def test_transposition_is_a_stable_sort():
    rng = np.random.default_rng(11)
    n_q, k, n_t = 37, 6, 9
    ind = rng.integers(-1, n_t + 2, (n_q, k)).astype(np.int64)
    ind[3] = 4                                                  # a target repeated inside a row
    ind[5] = [-1, n_t, np.iinfo(np.int32).max, -7, n_t + 1, -1]   # a row without a pair
    ind[ind == 2] = 3                                           # an empty column
    dist = rng.standard_normal((n_q, k))
    colptr, col_row, col_val = LR.transpose(dist, ind, n_t)
    ok = LR.pairs(ind, n_t)
    assert colptr[0] == 0 and colptr[-1] == ok.sum() == col_row.size == col_val.size and colptr[2] == colptr[3]
    for j in range(n_t):
        rows, cols = np.nonzero(ok & (ind == j))                # (row-major: ascending flat position)
        np.testing.assert_array_equal(col_row[colptr[j]:colptr[j + 1]], rows)
        np.testing.assert_array_equal(col_val[colptr[j]:colptr[j + 1]], dist[rows, cols])
    assert (col_row[colptr[4]:colptr[5]] == 3).sum() == k


def test_restatement_forms_agree():
    """The list / CSC form against the masked matrix through tests/sinkhorn_restate.py: one soft-min and whole iterations, on the fit
    cases' lists and on lists with padding, an empty row and empty columns.  (The two forms add the same terms with the masked
    form's exact zeros in between: numpy's pairwise sum groups them differently, so the bracket, not the bits.)"""
    for case in FIT_CASES:
        n_s, n_t, eps, L, _ = case
        for K in (10, 5):
            D, gold, (d, i) = _case_lists(case, K)
            f, g, done, change = LR.sinkhorn_potentials(d, i, n_t, eps, L)
            fm, gm = LR.sinkhorn_potentials_masked(d, i, n_t, eps, L)
            assert done == L and change is not None
            np.testing.assert_array_equal(np.isnan(g), np.isnan(gm))
            assert not np.isnan(f).any() and not np.isnan(fm).any()
            assert (np.abs(f - fm) <= 2 * L * SR.bracket(fm, eps)).all()
            live = ~np.isnan(g)
            assert (np.abs(g - gm)[live] <= 2 * L * SR.bracket(gm[live], eps)).all()
            assert np.isnan(g).sum() == (7 if (case, K) == (FIT_CASES[1], 5) else 0)
            # the inverted softmax: one column step without the constant
            g1 = LR.inverted_softmax_potential(d, i, n_t, eps)
            want = SR.softmin(LR.masked_matrix(d, i, n_t), eps, axis=0)
            np.testing.assert_array_equal(np.isnan(g1), np.isinf(want))
            assert (np.abs(g1 - want)[live] <= SR.bracket(want[live], eps)).all()
    rng = np.random.default_rng(5)
    n_q, k, n_t, eps = 40, 7, 23, 0.3
    ind = np.stack([rng.permutation(n_t + 6)[:k] - 3 for _ in range(n_q)]).astype(np.int64)   # ids in [-3, n_t + 3): padding, no repeats
    ind[9] = -1
    ind[ind == 11] = n_t
    dist = rng.standard_normal((n_q, k))
    dist[2, 1], dist[4, 0] = np.nan, np.inf
    off_t, off_q = rng.standard_normal(n_t), rng.standard_normal(n_q)
    D = LR.masked_matrix(dist, ind, n_t)
    rows = LR.softmin_rows(dist, ind, n_t, eps, off=off_t, shift=0.5)
    want = SR.softmin(D - off_t[None, :], eps, axis=1) + 0.5
    assert np.isnan(rows[9]) and want[9] == np.inf and np.isnan(rows).sum() == 1
    np.testing.assert_allclose(np.delete(rows, 9), np.delete(want, 9), rtol=1e-13, atol=1e-13)
    cols = LR.softmin_cols(*LR.transpose(dist, ind, n_t), eps, off=off_q, shift=-0.25)
    want = SR.softmin(D - off_q[:, None], eps, axis=0) - 0.25
    assert np.isnan(cols[11]) and want[11] == np.inf
    empty = np.isinf(D).all(axis=0)
    np.testing.assert_array_equal(np.isnan(cols), empty)
    np.testing.assert_allclose(cols[~empty], want[~empty], rtol=1e-13, atol=1e-13)
    # the change read-out ignores NaN differences
    assert LR.max_abs_diff(np.array([1.0, np.nan, 3.0]), np.array([1.5, 2.0, np.nan])) == 0.5
    assert LR.max_abs_diff(np.array([np.nan]), np.array([1.0])) == 0.0


def test_hits_at_1_depends_on_the_number_of_candidates():
    """The figures README, DESIGN section 3.1i and the class docstring quote: K is a parameter of the approximation."""
    def hits(case, K):
        n_s, n_t, eps, L, _ = case
        D, gold, (d, i) = _case_lists(case, K)
        f, g, _, _ = LR.sinkhorn_potentials(d, i, n_t, eps, L)
        return round(float((LR.topk_lists(LR.list_w(d, i, f, g), i, 1)[1][:, 0] == gold).mean()), 3)

    def hits_whole(case):
        n_s, n_t, eps, L, _ = case
        D, gold, _ = _case_lists(case, 1)
        f, g = SR.sinkhorn_potentials(D, eps, L)
        return round(float((SR.w(D, f, g).argmin(axis=1) == gold).mean()), 3), round(float((D.argmin(axis=1) == gold).mean()), 3)
    assert hits_whole(FIT_CASES[2]) == (0.803, 0.723)
    assert hits(FIT_CASES[2], 10) == 0.803 and hits(FIT_CASES[2], 5) == 0.780
    assert hits_whole(FIT_CASES[1]) == (1.0, 1.0)
    assert hits(FIT_CASES[1], 10) == 0.989 and hits(FIT_CASES[1], 5) == 0.911


def test_early_stopping_of_the_restatement():
    """The list form of the (200, 200, eps 0.1) case stops at iteration 40 at tol = 1e-3 (tests/test_gpu_sinkhorn_lists.py asserts the
    same of the device): the change at 39 is still above the tolerance, by 5e-6."""
    case = FIT_CASES[0]
    n_s, n_t, eps, L, _ = case
    D, gold, (d, i) = _case_lists(case, 10)
    f, g, done, change = LR.sinkhorn_potentials(d, i, n_t, eps, L, tol=1e-3)
    assert done == 40 and change <= 1e-3
    f39, g39, done39, change39 = LR.sinkhorn_potentials(d, i, n_t, eps, 39)
    assert done39 == 39 and change39 > 1e-3 + 1e-6
    f40, g40, _, change40 = LR.sinkhorn_potentials(d, i, n_t, eps, 40)
    np.testing.assert_array_equal(f, f40)
    np.testing.assert_array_equal(g, g40)
    assert change == change40 == np.abs(g40 - g39).max()
    assert LR.sinkhorn_potentials(d, i, n_t, eps, 1, tol=1e-3)[2:] == (1, None)
