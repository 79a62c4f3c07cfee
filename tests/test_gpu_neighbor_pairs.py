"""The neighbour pairs of both directions as a CSR (kz_lists_combine, kz_pairs_values, kz_csr_sort_rows; `neighbor_pairs`,
`match_pairs`, `assign_pairs`, `matching.combine_lists`) on the device.

Two oracles, both the library's own and already tested.  VALUES: at these sizes `radius_neighbors(inf, reduced=..., sort_results=False)`
returns every pair, and a pair's value must equal its entry of that table bit for bit.  MEMBERSHIP: the numpy restatement of the set
step (tests/pairs_restate.py, checked against dense boolean matrices in tests/test_neighbor_pairs.py) applied to the two `kneighbors`
results."""
import ctypes as C
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import pairs_restate as PR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
INT_MAX = 2 ** 31 - 1


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def _kiez(hubness=None, metric="euclidean", n_candidates=5, **kw):
    from kiez_amd import Kiez
    return Kiez(n_candidates=n_candidates, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=kw or None)


def _raw_lists(kz, k):
    """The raw lists of the two searches as `kneighbors` returns them -> (forward ind [n_s, k], reverse ind [n_t, k]).  The queries are
    named, so the shared sweep's cached forward lists are not touched."""
    nn = kz.algorithm
    fwd = nn.kneighbors(k=k, query=nn.source_, return_distance=False)
    rev = nn.kneighbors(k=k, query=nn.target_, s_to_t=False, return_distance=False)
    return fwd, rev


def _table(kz, reduced):
    """The value of EVERY pair, from the library's own whole-index call: a dense [n_source, n_target] table."""
    indptr, ind, val = kz.radius_neighbors(np.inf, reduced=reduced, sort_results=False)
    n_t = kz.algorithm.target_.shape[0]
    assert ind.size == (indptr.size - 1) * n_t, "the data has NaN values: the table is incomplete"
    return PR.table_from_csr(indptr, ind, val, n_t)


def _assert_pairs(got, fwd, rev, table, mode, sort_results=True, exact_order=True, where=""):
    """`got` = (indptr, ind, dist) against the restated set step on the raw lists and the table's values, bit for bit.
    exact_order=False (values cast to float32 AFTER the sort: two values may round to one): a row as a set of (id, value), ascending."""
    indptr, ind, val = got
    n_s, n_t = table.shape
    w_indptr, w_ind = PR.combine(fwd, rev, mode, n_s, n_t)
    w_val = PR.values(w_indptr, w_ind, table)
    assert indptr.dtype == ind.dtype == np.int64 and val.dtype == table.dtype, where
    np.testing.assert_array_equal(indptr, w_indptr, err_msg=where)
    if sort_results and exact_order:
        w_ind, w_val = PR.sort_rows(w_indptr, w_ind, w_val)
    if sort_results and not exact_order:
        assert (np.diff(val)[np.diff(PR.row_of(indptr)) == 0] >= 0).all(), where
        order = np.lexsort((ind, PR.row_of(indptr)))
        ind, val = ind[order], val[order]
    np.testing.assert_array_equal(ind, w_ind, err_msg=where)
    np.testing.assert_array_equal(_bits(val), _bits(w_val), err_msg=where)
    return np.diff(indptr)


# ---- the facade, plain values ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """37 x 53 x 8, float64, euclidean, k = 3: the fitted instances (with and without a reduction), the raw lists and the table."""
    rng = np.random.default_rng(5)
    source, target = rng.standard_normal((37, 8)), rng.standard_normal((53, 8))
    kz = _kiez("CSLS").fit(source, target)
    plain = _kiez(None).fit(source, target)
    fwd, rev = _raw_lists(kz, 3)
    table = _table(kz, False)
    for a in (fwd, rev, table):
        a.setflags(write=False)
    return kz, plain, fwd, rev, table


@pytest.mark.parametrize("mode", PR.MODES)
def test_four_modes_ids_values_and_row_order(small, mode):
    kz, plain, fwd, rev, table = small
    counts = {}
    res = kz.neighbor_pairs(3, mode=mode)
    assert all(isinstance(a, np.ndarray) for a in res) and res[0].shape == (38,)
    counts = _assert_pairs(res, fwd, rev, table, mode, where=mode)
    # by target row alone
    res_u = kz.neighbor_pairs(3, mode=mode, sort_results=False)
    _assert_pairs(res_u, fwd, rev, table, mode, sort_results=False, where=mode + " unsorted")
    rows = PR.row_of(res_u[0])
    assert (np.diff(res_u[1])[np.diff(rows) == 0] > 0).all()
    # without values, on the device, again (the same bytes), and from an instance that indexed the target only
    for got in (kz.neighbor_pairs(3, mode=mode, return_distance=False), kz.neighbor_pairs(3, mode=mode)[:2]):
        assert len(got) == 2
        np.testing.assert_array_equal(got[0], res[0])
        np.testing.assert_array_equal(got[1], res[1])
    for other in (kz.neighbor_pairs_device(3, mode=mode), kz.algorithm.neighbor_pairs_device(3, mode), kz.neighbor_pairs(3, mode=mode),
                  plain.neighbor_pairs(3, mode=mode), plain.neighbor_pairs(3, mode=mode, reduced=True)):
        for a, b in zip(other, res):
            a = a.numpy() if hasattr(a, "numpy") else a
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # |union| + |mutual| = |F| + |R|, per row
    if mode == "union":
        n = {m: np.diff(kz.neighbor_pairs(3, mode=m, return_distance=False)[0]) for m in PR.MODES}
        np.testing.assert_array_equal(n["union"] + n["mutual"], n["forward"] + n["reverse"])
        np.testing.assert_array_equal(n["forward"], np.full(37, 3))
        assert n["reverse"].sum() == 53 * 3 and (n["mutual"] > 0).any() and (n["mutual"] < 3).any()
        np.testing.assert_array_equal(counts, n["union"])
    # k = None is n_candidates, without a warning; k is not clamped to n_candidates
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res5 = kz.neighbor_pairs(mode=mode)
        res9 = kz.neighbor_pairs(9, mode=mode)
    fwd5, rev5 = _raw_lists(kz, 5)
    _assert_pairs(res5, fwd5, rev5, table, mode, where=mode + " k=None")
    fwd9, rev9 = _raw_lists(kz, 9)
    _assert_pairs(res9, fwd9, rev9, table, mode, where=mode + " k=9")


# ---- the set step alone ----------------------------------------------------------------------------------------------------------------
def _planted(rng, n_s, n_t, k_f, k_r):
    from tests.test_neighbor_pairs import planted_lists
    return planted_lists(rng, n_s, n_t, k_f, k_r)


@pytest.mark.parametrize("k_f,k_r", [(1, 7), (5, 64), (65, 3), (130, 130)])
def test_combine_lists_on_planted_lists(ctx, k_f, k_r):
    """Padding (-1, INT_MAX, >= n), repeats, k_f != k_r, against numpy bit for bit; 300 x 400 rows: up to 91 000 entries = 356 tiles
    of the prefix sum, beyond the 256 one round of its second level takes."""
    from kiez_amd import matching
    rng = np.random.default_rng(100 * k_f + k_r)
    n_s, n_t = 300, 400
    fwd, rev = _planted(rng, n_s, n_t, k_f, k_r)
    fwd_dev, rev_dev = ctx.to_device(fwd), ctx.to_device(rev)
    for mode in PR.MODES:
        want = PR.combine(fwd, rev, mode)
        got = matching.combine_lists(fwd, rev, mode=mode)
        dev = matching.combine_lists(fwd_dev, rev_dev, mode=mode)
        assert all(isinstance(a, np.ndarray) for a in got) and not any(isinstance(a, np.ndarray) for a in dev)
        for a, b, c in zip(got, dev, want):
            assert a.dtype == c.dtype == np.int64
            assert a.tobytes() == c.tobytes() == b.numpy().tobytes(), mode
    one = matching.combine_lists(fwd, None, mode="forward", n_target=n_t)
    np.testing.assert_array_equal(one[1], PR.combine(fwd, rev, "forward")[1])
    one = matching.combine_lists(None, rev_dev, mode="reverse", n_source=n_s)
    np.testing.assert_array_equal(one[1].numpy(), PR.combine(fwd, rev, "reverse")[1])
    # int32 ids from anywhere
    np.testing.assert_array_equal(matching.combine_lists(fwd.astype(np.int32), rev.astype(np.int32), mode="union")[1], PR.combine(fwd, rev, "union")[1])


def test_combine_lists_empty_results(ctx):
    from kiez_amd import matching
    # mutual of disjoint lists: every row empty, total 0, zero-length arrays
    fwd = np.array([[0, 1], [1, 0], [-1, -1]], dtype=np.int64)
    rev = np.array([[2, 2], [2, -1], [0, 1], [1, 0]], dtype=np.int64)
    indptr, ind = matching.combine_lists(fwd, rev, mode="mutual")
    np.testing.assert_array_equal(indptr, [0, 0, 0, 0])
    assert ind.shape == (0,) and ind.dtype == np.int64
    indptr, ind = matching.combine_lists(fwd, rev, mode="union")
    np.testing.assert_array_equal(indptr, [0, 4, 8, 10])
    np.testing.assert_array_equal(ind, [0, 1, 2, 3, 0, 1, 2, 3, 0, 1])
    # all padding
    indptr, ind = matching.combine_lists(np.full((5, 3), -1), np.full((6, 2), INT_MAX), mode="union")
    np.testing.assert_array_equal(indptr, np.zeros(6))
    assert ind.shape == (0,)
    # n_source = 0
    for mode in PR.MODES:
        indptr, ind = matching.combine_lists(np.empty((0, 3), dtype=np.int64), np.full((4, 2), -1, dtype=np.int64), mode=mode, n_source=0,
                                             n_target=4)
        np.testing.assert_array_equal(indptr, [0])
        assert ind.shape == (0,) and indptr.dtype == ind.dtype == np.int64


def test_capacity_contract_of_the_native_call(ctx):
    """capacity 0, a capacity that ends inside a row, one exactly at a row end: indptr and the total are complete, the rows that end
    within the capacity are written and NOTHING else is -- sentinel-filled outputs."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(9)
    fwd, rev = _planted(rng, 40, 60, 6, 4)
    w_indptr, w_ind = PR.combine(fwd, rev, "union")
    total = int(w_indptr[-1])
    inside = int(w_indptr[17]) + 1
    assert w_indptr[17] < inside < w_indptr[18] and total > 100
    fwd_dev, rev_dev = ctx.to_device(fwd), ctx.to_device(rev)
    SENT = -77
    for capacity in (0, inside, int(w_indptr[18]), total, total + 5):
        indptr = ctx.to_device(np.full(41, SENT, dtype=np.int64))
        ind = ctx.to_device(np.full(total + 9, SENT, dtype=np.int64))
        h_total = C.c_int64(-1)
        rc = ctx.lib.kz_lists_combine(ctx.handle, fwd_dev.ptr, 40, 6, rev_dev.ptr, 60, 4, N.PAIR_MODES["union"], capacity, indptr.ptr,
                                      ind.ptr if capacity else None, C.byref(h_total))
        assert rc == 0 and h_total.value == total
        np.testing.assert_array_equal(indptr.numpy(), w_indptr)
        written = int(w_indptr[np.searchsorted(w_indptr, capacity, side="right") - 1])   # the last row end <= capacity
        got = ind.numpy()
        np.testing.assert_array_equal(got[:written], w_ind[:written], err_msg=f"capacity {capacity}")
        np.testing.assert_array_equal(got[written:], np.full(total + 9 - written, SENT), err_msg=f"capacity {capacity}")
    assert N.lists_combine(ctx, fwd_dev, rev_dev, "union", capacity=0)[2] == total
    # what the call refuses, before it writes
    indptr, ind = ctx.to_device(np.full(41, SENT, dtype=np.int64)), ctx.to_device(np.full(8, SENT, dtype=np.int64))
    h_total = C.c_int64(-1)
    for args in ((40, 0, 60, 4, 2, 8), (40, 6, 60, 4097, 2, 8), (40, 6, 0, 4, 2, 8), (40, 6, 60, 4, 4, 8), (40, 6, 60, 4, -1, 8),
                 (40, 6, 60, 4, 2, -1), (-1, 6, 60, 4, 2, 8)):
        n_q, k_f, n_t, k_r, mode, cap = args
        rc = ctx.lib.kz_lists_combine(ctx.handle, fwd_dev.ptr, n_q, k_f, rev_dev.ptr, n_t, k_r, mode, cap, indptr.ptr, ind.ptr, C.byref(h_total))
        assert rc != 0, args
    np.testing.assert_array_equal(indptr.numpy(), np.full(41, SENT))
    np.testing.assert_array_equal(ind.numpy(), np.full(8, SENT))
    with pytest.raises(ValueError, match="capacity"):
        N.lists_combine(ctx, fwd_dev, rev_dev, "union", capacity=-1)


# ---- rows beyond the LDS sort ----------------------------------------------------------------------------------------------------------
def test_hub_rows_of_4200_entries():
    """70 sources, 4 200 targets, d = 4, k = 2: sources 0 and 1 are the two nearest sources of EVERY target, so in "reverse" their rows
    hold 4 200 entries each (the radix branch of the row sort) and every other row is empty."""
    rng = np.random.default_rng(11)
    target = 0.01 * rng.standard_normal((4200, 4))
    source = 10.0 + rng.standard_normal((70, 4))
    source[0] = [0.5, 0.0, 0.0, 0.0]
    source[1] = [0.0, -0.6, 0.0, 0.0]
    kz = _kiez("CSLS").fit(source, target)
    fwd, rev = _raw_lists(kz, 2)
    assert set(np.unique(rev).tolist()) == {0, 1}
    table = _table(kz, False)
    for mode in ("reverse", "union"):
        counts = _assert_pairs(kz.neighbor_pairs(2, mode=mode), fwd, rev, table, mode, where=mode)
        assert counts[0] == counts[1] == 4200 and (counts[2:] == (0 if mode == "reverse" else 2)).all()
    table_w = _table(kz, True)
    _assert_pairs(kz.neighbor_pairs(2, mode="union", reduced=True), fwd, rev, table_w, "union", where="union reduced")
    # the matching over them: the two hubs take a target each, the CSR never leaves the device
    m_dist, m_ind = kz.match_pairs(2, mode="reverse")
    assert (m_ind[:2] >= 0).all() and m_ind[0] != m_ind[1] and (m_ind[2:] == -1).all()
    np.testing.assert_array_equal(m_dist[:2], table[[0, 1], m_ind[:2]])


# ---- the reduced kinds -----------------------------------------------------------------------------------------------------------------
def _reductions():
    from kiez_amd import Sinkhorn
    return [("CSLS", {}), ("LocalScaling", {"method": "standard"}), ("LocalScaling", {"method": "nicdm"}),
            ("MutualProximity", {"method": "normal"}), (Sinkhorn, {"temperature": 0.5, "n_iter": 5})]


@pytest.fixture(scope="module")
def rows_60_80():
    rng = np.random.default_rng(17)
    source, target = rng.standard_normal((60, 16)), rng.standard_normal((80, 16))
    source.setflags(write=False)
    target.setflags(write=False)
    return source, target


@pytest.mark.parametrize("which", range(5), ids=["csls", "ls", "nicdm", "mp_normal", "sinkhorn"])
def test_reduced_values_are_the_reduced_table(rows_60_80, which):
    hubness, kw = _reductions()[which]
    source, target = rows_60_80
    kz = _kiez(hubness, **kw).fit(source, target)
    fwd, rev = _raw_lists(kz, 5)
    table_w, table = _table(kz, True), _table(kz, False)
    assert not np.array_equal(table_w, table)
    for mode in PR.MODES:
        _assert_pairs(kz.neighbor_pairs(5, mode=mode, reduced=True), fwd, rev, table_w, mode, where=f"{mode} reduced")
    _assert_pairs(kz.neighbor_pairs(5, mode="union"), fwd, rev, table, "union", where="union plain")   # reduced=False: the search metric
    # "forward": a row IS transform's output for the same lists, as (id, value) sets
    nn = kz.algorithm
    fd, fi = nn.kneighbors(k=5, query=nn.source_)
    np.testing.assert_array_equal(fi, fwd)
    wd, wi = kz.hubness.transform(fd, fi, nn.source_)
    indptr, ind, val = kz.neighbor_pairs(5, mode="forward", reduced=True, sort_results=False)
    np.testing.assert_array_equal(indptr, 5 * np.arange(61))
    order = np.argsort(wi, axis=1, kind="stable")
    np.testing.assert_array_equal(ind.reshape(60, 5), np.take_along_axis(wi, order, axis=1))
    np.testing.assert_array_equal(_bits(val.reshape(60, 5)), _bits(np.take_along_axis(np.asarray(wd, dtype=np.float64), order, axis=1)))


def test_what_the_facade_refuses(rows_60_80):
    from kiez_amd.neighbors import NotFittedError
    source, target = rows_60_80
    for hubness, kw in (("MutualProximity", {"method": "empiric"}), ("DisSimLocal", {})):
        kz = _kiez(hubness, **kw).fit(source, target)
        for call in (kz.neighbor_pairs, kz.match_pairs, kz.assign_pairs):
            with pytest.raises(NotImplementedError, match="outside the list|own gather"):
                call(5, mode="union", reduced=True)
        assert kz.neighbor_pairs(5, mode="mutual")[1].size > 0   # (the plain call is served)
        with pytest.raises(ValueError, match="mode must be one of"):
            kz.neighbor_pairs(5, mode="all", reduced=True)
    for reduced in (False, True):
        single = _kiez("CSLS").fit(np.array(source))
        for call in (single.neighbor_pairs, single.match_pairs, single.assign_pairs):
            with pytest.raises(NotImplementedError, match="two-sided"):
                call(5, mode="union", reduced=reduced)
        with pytest.raises(NotFittedError):
            _kiez("CSLS").neighbor_pairs(5, reduced=reduced)
    kz = _kiez("CSLS").fit(source, target)
    with pytest.raises(ValueError, match="positive integer k"):
        kz.neighbor_pairs(True)
    with pytest.warns(UserWarning, match="larger than number of samples"):   # (the search's own check, per direction)
        indptr, ind = kz.neighbor_pairs(70, mode="reverse", return_distance=False)   # 70 > 60 sources: every target lists them all
    np.testing.assert_array_equal(indptr, 80 * np.arange(61))


# ---- conversions -----------------------------------------------------------------------------------------------------------------------
CONVERSIONS = [("euclidean", np.float32, True), ("cosine", np.float32, False), ("euclidean", np.float16, True), ("manhattan", np.float64, True),
               ("jaccard", np.float32, True), ("precomputed", np.float32, False), ("precomputed", np.float64, True)]


@pytest.mark.parametrize("metric,dtype,exact_order", CONVERSIONS, ids=[f"{m}_{np.dtype(d).name}" for m, d, _ in CONVERSIONS])
def test_conversions_against_the_table(metric, dtype, exact_order):
    """One small case per conversion: float32 euclidean (the float32 rounding of the square root), float32 cosine and a float32
    precomputed matrix (values cast to float32 LAST: after the sort), float16 rows, the Minkowski family, a boolean metric."""
    rng = np.random.default_rng(23)
    if metric == "jaccard":
        source, target = (rng.random((40, 24)) < 0.3).astype(dtype), (rng.random((50, 24)) < 0.3).astype(dtype)
    else:
        source, target = rng.standard_normal((40, 12)).astype(dtype), rng.standard_normal((50, 12)).astype(dtype)
    out_dtype = np.float32 if metric in ("cosine", "precomputed") and dtype == np.float32 else np.float64
    for hubness in ("CSLS", None):
        if metric == "precomputed":
            D = np.abs(rng.standard_normal((40, 50))).astype(dtype)
            kz = _kiez(hubness, metric=metric).fit(D)
        else:
            kz = _kiez(hubness, metric=metric).fit(source, target)
        lists = _kiez("CSLS", metric=metric).fit(D) if metric == "precomputed" else _kiez("CSLS", metric=metric).fit(source, target)
        fwd, rev = _raw_lists(lists, 4)
        for reduced in (False, True):
            table = _table(kz, reduced)
            assert table.dtype == out_dtype
            if metric == "precomputed" and not reduced:
                np.testing.assert_array_equal(table, D)           # the value of a pair is the matrix entry
            for mode in ("union", "mutual"):
                res = kz.neighbor_pairs(4, mode=mode, reduced=reduced)
                _assert_pairs(res, fwd, rev, table, mode, exact_order=exact_order, where=f"{metric} {mode} reduced={reduced}")
            res = kz.neighbor_pairs(4, mode="reverse", reduced=reduced, sort_results=False)
            _assert_pairs(res, fwd, rev, table, "reverse", sort_results=False, where=f"{metric} reverse reduced={reduced}")


# ---- the one-to-one steps --------------------------------------------------------------------------------------------------------------
def test_match_pairs_and_assign_pairs(rows_60_80):
    from kiez_amd import matching
    source, target = rows_60_80
    kz = _kiez("CSLS").fit(source, target)
    fwd, rev = _raw_lists(kz, 5)
    F, R = PR.pair_sets(fwd, rev, 60, 80)
    for mode in ("union", "mutual", "reverse"):
        for reduced in (False, True):
            csr = kz.neighbor_pairs(5, mode=mode, reduced=reduced)
            m_dist, m_ind = kz.match_pairs(5, mode=mode, reduced=reduced)
            w_dist, w_ind = matching.one_to_one_csr(*csr, 80)
            np.testing.assert_array_equal(m_ind, w_ind)
            np.testing.assert_array_equal(_bits(m_dist), _bits(w_dist))
            np.testing.assert_array_equal(kz.match_pairs(5, mode=mode, reduced=reduced, return_distance=False), w_ind)
            a_dist, a_ind = kz.assign_pairs(5, mode=mode, reduced=reduced)
            v_dist, v_ind = matching.assignment_csr(*csr, 80)
            np.testing.assert_array_equal(a_ind, v_ind)
            np.testing.assert_array_equal(_bits(a_dist), _bits(v_dist))
            u = float(np.median(csr[2]))
            a_dist, a_ind = kz.assign_pairs(5, mode=mode, reduced=reduced, unmatched_cost=u)
            v_dist, v_ind = matching.assignment_csr(*csr, 80, unmatched_cost=u)
            np.testing.assert_array_equal(a_ind, v_ind)
            assert (a_dist[a_ind >= 0] <= u).all()
            for ind in (m_ind, a_ind):
                matched = ind[ind >= 0]
                assert matched.size > 0 and len(set(matched.tolist())) == matched.size
                if mode == "mutual":                              # every matched pair is a mutual nearest-neighbour pair
                    assert all(int(j) in (F[i] & R[i]) for i, j in enumerate(ind) if j >= 0)
            dev = kz.match_pairs_device(5, mode=mode, reduced=reduced)
            np.testing.assert_array_equal(dev[1].numpy(), m_ind)


# ---- the shared sweep's cache ----------------------------------------------------------------------------------------------------------
def test_cached_forward_lists_are_left_as_found(rows_60_80):
    from kiez_amd import _native as N
    source, target = rows_60_80
    kz = _kiez("CSLS", n_candidates=5).fit(source, target)
    nn = kz.algorithm
    cached = nn._forward
    assert cached is not None and cached[0] == 5                 # (the fit ran the shared sweep)
    calls = []
    real_knn, real_dual = N.knn, N.knn_dual

    def knn(*a, **k):
        calls.append(("knn", a[3]))
        return real_knn(*a, **k)

    def knn_dual(*a, **k):
        calls.append(("dual", a[3]))
        return real_dual(*a, **k)
    N.knn, N.knn_dual = knn, knn_dual
    try:
        kz.neighbor_pairs(5, mode="union", reduced=True)
        assert nn._forward is cached and calls == [("knn", 5)]    # the cached forward lists were read: the reverse search alone
        kz.neighbor_pairs(3, mode="mutual")
        assert nn._forward is cached and calls[1:] == [("dual", 3)]   # another k: one sweep for both directions, the cache untouched
        kz.neighbor_pairs(3, mode="forward")
        kz.match_pairs(5, mode="mutual", reduced=True)
        assert nn._forward is cached
        del calls[:]
        d5, i5 = kz.kneighbors(5)
        assert calls == [] and nn._forward is None                # served from the cache, which is handed out once
    finally:
        N.knn, N.knn_dual = real_knn, real_dual
    fresh_d, fresh_i = _kiez("CSLS", n_candidates=5).fit(source, target).kneighbors(5)
    np.testing.assert_array_equal(i5, fresh_i)
    np.testing.assert_array_equal(_bits(d5), _bits(fresh_d))


TENSOR_SCRIPT = r"""
import sys, warnings
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd import Kiez
warnings.simplefilter("ignore")
rng = np.random.default_rng(3)
s, t = rng.random((200, 16)).astype(np.float32), rng.random((260, 16)).astype(np.float32)
def kiez():
    return Kiez(n_candidates=6, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
base = kiez().fit(s, t)
want = {(m, r): base.neighbor_pairs(6, mode=m, reduced=r) for m in ("union", "mutual") for r in (False, True)}
for dev in ("cuda", "cpu"):
    kz = kiez().fit(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev))
    for (m, r), exp in want.items():
        got = kz.neighbor_pairs(6, mode=m, reduced=r)
        assert all(isinstance(a, torch.Tensor) and a.device.type == dev for a in got), [type(a) for a in got]
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float64
        for a, b in zip(got, exp):
            assert np.array_equal(a.cpu().numpy(), b), (dev, m, r)
    ids = kz.neighbor_pairs(6, mode="mutual", return_distance=False)
    assert len(ids) == 2 and all(isinstance(a, torch.Tensor) for a in ids)
    m_dist, m_ind = kz.match_pairs(6, mode="mutual")
    assert isinstance(m_ind, np.ndarray)       # (the matching calls stay numpy, as `match`)
print("PAIRS_TENSORS_OK")
"""


def test_fitted_on_tensors_subprocess():
    """Tensors in, tensors out on the source's device (torch has to be imported before the library is loaded: a process of its own)."""
    r = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PAIRS_TENSORS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
