"""The numpy restatement of the neighbour-pair calls (tests/pairs_restate.py) against dense boolean matrices (F | R, F & R, R),
and the argument errors `neighbor_pairs`, `match_pairs`, `assign_pairs` and `matching.combine_lists` raise on the host before any
device call.  No GPU."""
import numpy as np
import pytest

from tests import pairs_restate as PR

INT_MAX = 2 ** 31 - 1


def planted_lists(rng, n_source, n_target, k_f, k_r):
    """Random list arrays with everything the set step must survive: -1, INT_MAX and >= n padding, ids repeated inside a row."""
    fwd = rng.integers(0, n_target, size=(n_source, k_f), dtype=np.int64)
    rev = rng.integers(0, n_source, size=(n_target, k_r), dtype=np.int64)
    for a, n in ((fwd, n_target), (rev, n_source)):
        a[rng.random(a.shape) < 0.15] = -1
        a[rng.random(a.shape) < 0.10] = INT_MAX
        a[rng.random(a.shape) < 0.05] = n
        a[rng.random(a.shape) < 0.05] = n + 7
        if a.shape[1] > 1:   # a repeat of the row's first entry
            rows = rng.random(a.shape[0]) < 0.5
            a[rows, -1] = a[rows, 0]
    return fwd, rev


def dense(fwd, rev, n_source, n_target):
    """(F, R) as boolean matrices [n_source, n_target], by fancy indexing: no set, no loop over entries."""
    F = np.zeros((n_source, n_target), dtype=bool)
    R = np.zeros((n_source, n_target), dtype=bool)
    i, c = np.nonzero((fwd >= 0) & (fwd < n_target))
    F[i, fwd[i, c]] = True
    j, c = np.nonzero((rev >= 0) & (rev < n_source))
    R[rev[j, c], j] = True
    return F, R


def csr_of(mask):
    indptr = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(mask.sum(axis=1))
    return indptr, np.nonzero(mask)[1].astype(np.int64)


@pytest.mark.parametrize("n_source,n_target,k_f,k_r", [(37, 53, 3, 5), (20, 9, 7, 1), (5, 130, 65, 3), (1, 1, 1, 1), (64, 64, 4, 4)])
def test_restatement_is_the_dense_set_algebra(n_source, n_target, k_f, k_r):
    rng = np.random.default_rng(n_source * 1000 + n_target)
    fwd, rev = planted_lists(rng, n_source, n_target, k_f, k_r)
    F, R = dense(fwd, rev, n_source, n_target)
    want = {"forward": F, "reverse": R, "union": F | R, "mutual": F & R}
    got = {}
    for mode in PR.MODES:
        indptr, ind = PR.combine(fwd, rev, mode)
        w_indptr, w_ind = csr_of(want[mode])
        np.testing.assert_array_equal(indptr, w_indptr, err_msg=mode)
        np.testing.assert_array_equal(ind, w_ind, err_msg=mode)
        assert indptr.dtype == np.int64 and ind.dtype == np.int64
        got[mode] = np.diff(indptr)
    np.testing.assert_array_equal(got["union"] + got["mutual"], got["forward"] + got["reverse"])   # |A u B| + |A n B| = |A| + |B|, per row
    # one-sided modes read one array
    np.testing.assert_array_equal(PR.combine(fwd, None, "forward", n_target=n_target)[1], csr_of(F)[1])
    np.testing.assert_array_equal(PR.combine(None, rev, "reverse", n_source=n_source)[1], csr_of(R)[1])


def test_restatement_empty_results_and_no_rows():
    fwd = np.array([[0, 1], [1, 0], [-1, -1]], dtype=np.int64)       # sources 0, 1 list targets 0, 1
    rev = np.array([[2, 2], [2, -1], [0, 1], [1, 0]], dtype=np.int64)  # targets 0, 1 list source 2; targets 2, 3 list sources 0, 1
    indptr, ind = PR.combine(fwd, rev, "mutual")                       # disjoint: every row empty
    np.testing.assert_array_equal(indptr, [0, 0, 0, 0])
    assert ind.shape == (0,) and ind.dtype == np.int64
    indptr, ind = PR.combine(fwd, rev, "union")
    np.testing.assert_array_equal(indptr, [0, 4, 8, 10])
    np.testing.assert_array_equal(ind, [0, 1, 2, 3, 0, 1, 2, 3, 0, 1])
    indptr, ind = PR.combine(np.empty((0, 3), dtype=np.int64), np.full((4, 2), -1, dtype=np.int64), "union")   # n_source = 0
    np.testing.assert_array_equal(indptr, [0])
    assert ind.shape == (0,)


def test_restated_values_and_row_sort():
    """value = table[i, j]; the row order is (value, target row) with NaN last and -0.0 == +0.0."""
    table = np.array([[3.0, -0.0, 0.0, np.nan, 1.0], [np.nan, np.nan, -np.inf, np.inf, 2.0]])
    indptr, ind = np.array([0, 5, 9], dtype=np.int64), np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], dtype=np.int64)
    val = PR.values(indptr, ind, table)
    np.testing.assert_array_equal(val, [3.0, -0.0, 0.0, np.nan, 1.0, np.nan, np.nan, -np.inf, np.inf])
    s_ind, s_val = PR.sort_rows(indptr, ind, val)
    np.testing.assert_array_equal(s_ind, [1, 2, 4, 0, 3, 2, 0, 1, 3])   # row 1: -inf, then NaN / +inf tie as +inf and go by target row
    assert np.signbit(s_val[0]) and not np.signbit(s_val[1]) and np.isnan(s_val[4])
    np.testing.assert_array_equal(PR.row_of(indptr), [0, 0, 0, 0, 0, 1, 1, 1, 1])
    back = PR.table_from_csr(np.array([0, 2, 3]), np.array([4, 0, 2]), np.array([1.0, 3.0, -np.inf]), 5)
    np.testing.assert_array_equal(back, [[3.0, np.nan, np.nan, np.nan, 1.0], [np.nan, np.nan, -np.inf, np.nan, np.nan]])


def test_mode_and_k_are_checked_on_the_host():
    """A mode outside the four, a bool or non-int k: ValueError -- before the fit state is looked at, so also on an unfitted
    instance; a valid call on an unfitted instance: NotFittedError."""
    from kiez_amd import Kiez
    from kiez_amd.neighbors import NotFittedError
    for hubness in (None, "CSLS"):
        kz = Kiez(n_candidates=5, hubness=hubness)
        calls = [kz.neighbor_pairs, kz.neighbor_pairs_device, kz.match_pairs, kz.match_pairs_device, kz.assign_pairs, kz.assign_pairs_device,
                 kz.algorithm.neighbor_pairs, kz.algorithm.neighbor_pairs_device, kz.hubness.neighbor_pairs, kz.hubness.neighbor_pairs_device]
        for call in calls:
            for reduced in ({}, {"reduced": True}) if call.__self__ is kz else ({},):
                for bad in ("both", "Union", None, 2, b"union"):
                    with pytest.raises(ValueError, match="mode must be one of"):
                        call(3, mode=bad, **reduced)
                for bad in (True, np.bool_(False), 0, -2, 2.0, "3", [3]):
                    with pytest.raises(ValueError, match="positive integer k"):
                        call(bad, mode="mutual", **reduced)
                for k in (None, 3, np.int64(7)):
                    with pytest.raises(NotFittedError):
                        call(k, mode="union", **reduced)


def test_combine_lists_is_checked_on_the_host():
    from kiez_amd import matching
    fwd, rev = np.zeros((3, 2), dtype=np.int64), np.zeros((4, 2), dtype=np.int64)
    with pytest.raises(ValueError, match="mode must be one of"):
        matching.combine_lists(fwd, rev, mode="all")
    with pytest.raises(TypeError):
        matching.combine_lists(fwd, rev)   # mode is required, by keyword
    with pytest.raises(ValueError, match="2-D array of ids"):
        matching.combine_lists(fwd[0], rev, mode="union")
    with pytest.raises(ValueError, match="at least one column"):
        matching.combine_lists(fwd[:, :0], rev, mode="union")
    with pytest.raises(ValueError, match="integer row ids"):
        matching.combine_lists(fwd.astype(np.float64), rev, mode="union")
    with pytest.raises(ValueError, match="integer row ids"):
        matching.combine_lists(fwd, rev.astype(bool), mode="mutual")
    with pytest.raises(ValueError, match="n_target must be a positive integer"):
        matching.combine_lists(fwd, rev, mode="union", n_target=0)
    with pytest.raises(ValueError, match="n_source must be a non-negative integer"):
        matching.combine_lists(fwd, rev, mode="union", n_source=True)
    with pytest.raises(ValueError, match="one row per source row"):
        matching.combine_lists(fwd, rev, mode="union", n_source=5)
    with pytest.raises(ValueError, match="name n_source and n_target"):
        matching.combine_lists(fwd, None, mode="forward")


def test_union_is_a_support_of_the_dual_potentials():
    from kiez_amd.hubness_reduction import InvertedSoftmax, Sinkhorn
    from kiez_amd.neighbors import SklearnNN
    for cls in (Sinkhorn, InvertedSoftmax):
        assert "union" in cls._SUPPORTS
        red = cls(nn_algo=SklearnNN(n_candidates=5), support="union")
        assert red.support == "union" and "union" in repr(red)
        with pytest.raises(ValueError, match="support must be one of"):
            cls(nn_algo=SklearnNN(n_candidates=5), support="mutual")
