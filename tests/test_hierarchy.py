"""The single-linkage hierarchy without a GPU: the numpy restatement (tests/hierarchy_restate.py) against scipy's minimum spanning tree
and connected components, `matching.Hierarchy`'s host logic, `evaluate.cluster_curve`'s default thresholds, and the argument checks
that raise before a device is touched."""
import numpy as np
import pytest

from tests import components_restate as CR
from tests import hierarchy_restate as HR


@pytest.fixture(scope="module")
def ties_positive():
    """300 x 280, three entries a row, strictly positive weights in eighths (scipy's csgraph reads a stored 0 as "no edge")."""
    g = HR.random_ties(positive=True)
    return g, HR.forest(*g)


def test_forest_weights_equal_scipys_minimum_spanning_tree(ties_positive):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    (indptr, ind, w, n_t), (source, target, value, entry, c) = ties_positive
    n_q = len(indptr) - 1
    rows = np.repeat(np.arange(n_q), np.diff(indptr))
    # duplicates kept at their minimum: a dense [n_q, n_t] minimum, inf where there is no pair
    best = np.full((n_q, n_t), np.inf)
    np.minimum.at(best, (rows, ind), w)
    r, col = np.nonzero(np.isfinite(best))
    A = sp.coo_matrix((best[r, col], (r, col + n_q)), shape=(n_q + n_t, n_q + n_t)).tocsr()
    mst = minimum_spanning_tree(A)
    assert value.shape[0] == mst.nnz == n_q + n_t - c > 500
    np.testing.assert_array_equal(np.sort(mst.data), value)     # (the sorted weights are the same for every spanning forest)
    assert c == CR.scipy_components(indptr, ind, n_t)[0]
    # the forest's own arrays: the edges are entries of the list, ascending by (value, entry)
    np.testing.assert_array_equal(ind[entry], target)
    np.testing.assert_array_equal(rows[entry], source)
    np.testing.assert_array_equal(w[entry], value)
    assert all((a, p) < (b, q) for a, p, b, q in zip(value[:-1], entry[:-1], value[1:], entry[1:]))


def test_every_prefix_has_the_components_of_the_thresholded_graph(ties_positive):
    (indptr, ind, w, n_t), (source, target, value, entry, c) = ties_positive
    n_q = len(indptr) - 1
    for t in np.unique(value):
        m = int(np.searchsorted(value, t, side="right"))
        sub_ptr, sub_ind = HR.restrict(indptr, ind, w, t)
        assert n_q + n_t - m == CR.scipy_components(sub_ptr, sub_ind, n_t)[0], t
        # and the labelling of the prefix IS the labelling of the thresholded list
        want = HR.cut(indptr, ind, w, n_t, t)
        got = CR.components(*CR.csr_of(source[:m], target[:m], n_q), n_t)
        for a, b in zip(got[:4], want[:4]):
            np.testing.assert_array_equal(a, b)


def test_order_key_orders_like_the_values():
    v = np.array([-np.inf, -3.0, -1e-300, -0.0, 0.0, 1e-300, 2.0, np.inf])
    k = HR.order_key(v)
    assert k[3] == k[4] and (np.diff(k[[0, 1, 2, 3, 5, 6, 7]].astype(object)) > 0).all()
    # -0.0 and +0.0 tie by position; -inf comes first; NaN is no edge
    src, tgt, val, ent, c = HR.forest([0, 3, 6], [0, 1, 2, 0, 1, 2], [0.0, np.nan, 5.0, -0.0, -np.inf, np.nan], 3)
    assert ent.tolist() == [4, 0, 3, 2] and c == 1
    assert np.signbit(val).tolist() == [True, False, True, False]


def _hierarchy():
    from kiez_amd.matching import Hierarchy
    # 3 sources, 3 targets: the path s0 - t0 - s1 - t1 and s2 - t2 apart
    return Hierarchy(3, 3, 2, [0, 1, 1, 2], [0, 0, 1, 2], [-1.0, -0.0, 0.0, 2.5], [0, 2, 3, 5])


def test_n_clusters_at_below_and_above_every_value():
    h = _hierarchy()
    for i, v in enumerate(h.value):
        at = int(np.count_nonzero(h.value <= v))
        assert h.n_clusters(v) == 6 - at
        assert h.n_clusters(np.nextafter(v, -np.inf)) == 6 - int(np.count_nonzero(h.value < v))
        assert h.n_clusters(np.nextafter(v, np.inf)) == 6 - at
    assert h.n_clusters(0.0) == h.n_clusters(-0.0) == 3            # both zeros fall on one side
    assert h.n_clusters(-np.inf) == 6 and h.n_clusters(np.inf) == h.n_components == 2
    assert h.n_clusters(np.float32(2.5)) == 2 and h.n_edges(-1) == 1


def test_a_nan_threshold_is_a_value_error_on_the_host():
    h = _hierarchy()
    for call in (h.n_clusters, h.n_edges, h.cut, h.cut_device):
        with pytest.raises(ValueError, match="NaN"):
            call(float("nan"))
    with pytest.raises(ValueError, match="real number"):
        h.cut("0.5")
    with pytest.raises(ValueError, match="real number"):
        h.n_clusters(True)


def test_hierarchy_checks_its_arrays():
    from kiez_amd.matching import Hierarchy
    with pytest.raises(ValueError, match="edges, got 2"):
        Hierarchy(3, 3, 2, [0, 1], [0, 0], [1.0, 2.0], [0, 1])
    with pytest.raises(ValueError, match="ascending"):
        Hierarchy(2, 1, 1, [0, 1], [0, 0], [2.0, 1.0], [0, 1])
    with pytest.raises(ValueError, match="ascending"):
        Hierarchy(2, 1, 1, [0, 1], [0, 0], [2.0, np.nan], [0, 1])
    with pytest.raises(ValueError, match="one length"):
        Hierarchy(2, 1, 1, [0, 1], [0], [1.0, 2.0], [0, 1])
    empty = Hierarchy(0, 4, 4, [], [], [], [])
    assert empty.n_clusters(np.inf) == 4 and empty.value.dtype == np.float64 and empty.entry.dtype == np.int64


def test_argument_checks_come_before_the_device(monkeypatch):
    """Every call below raises ValueError -- with or without a GPU in the machine: asking for a context fails the test."""
    from kiez_amd import _native as N
    from kiez_amd import matching

    def touched(cls, *args, **kwargs):
        pytest.fail("an argument check came after the device was asked for")
    monkeypatch.setattr(N.Context, "get", classmethod(touched))
    indptr, ind, dist = [0, 2, 3], [0, 1, 1], [0.5, 0.25, 1.0]
    for call in (lambda: matching.single_linkage_csr(indptr, ind, None, 2),
                 lambda: matching.single_linkage(None, [[0, 1]], 2),
                 lambda: matching.single_linkage_csr(indptr, ind, dist, 0),
                 lambda: matching.single_linkage_csr(indptr, ind, dist, 2.0),
                 lambda: matching.single_linkage_csr(indptr, ind, dist[:2], 2),
                 lambda: matching.single_linkage_csr([0, 2, 4], ind, dist, 2),
                 lambda: matching.single_linkage_csr([0, 2, 1, 3], ind, dist, 2),
                 lambda: matching.single_linkage_csr(indptr, [0.0, 1.0, 1.0], dist, 2),
                 lambda: matching.single_linkage_csr(indptr, ind, [1, 2, 3], 2),
                 lambda: matching.single_linkage([[0.5, 1.0]], [[0, 1, 1]], 2),
                 lambda: matching.single_linkage([0.5, 1.0], [0, 1], 2),
                 lambda: matching.single_linkage_csr(indptr, ind, dist, 2 ** 31 - 3)):
        with pytest.raises(ValueError):
            call()


def test_cluster_curve_takes_evenly_spaced_distinct_values_and_the_last(monkeypatch):
    from kiez_amd import evaluate
    from kiez_amd.matching import Hierarchy
    n = 200
    value = np.repeat(np.arange(100, dtype=np.float64), 2)[:n - 1]      # 100 distinct values, most of them twice
    h = Hierarchy(100, 100, 1, np.arange(n - 1) // 2, (np.arange(n - 1) + 1) // 2, value, np.arange(n - 1))
    seen = []

    def cut(t, return_sizes=False):       # the host stand-in of the device cut: the restatement on the prefix
        seen.append(t)
        m = h.n_edges(t)
        return CR.components(*CR.csr_of(h.source[:m], h.target[:m], 100), 100)[:2]
    monkeypatch.setattr(h, "cut", cut)
    gold = np.arange(100)
    curve = evaluate.cluster_curve(h, gold, max_points=8)
    assert curve["threshold"].shape == (8,) and curve["threshold"][-1] == 99.0 and curve["threshold"][0] == 0.0
    assert (np.diff(curve["threshold"]) > 0).all() and seen == curve["threshold"].tolist()
    assert set(curve) == {"threshold", "precision", "recall", "f1", "n_components", "n_pairs", "best"}
    np.testing.assert_array_equal(curve["n_components"], [h.n_clusters(t) for t in curve["threshold"]])
    assert curve["best"] == int(np.argmax(curve["f1"])) and curve["recall"][-1] == 1.0
    assert curve["n_pairs"].dtype == np.int64 and curve["n_pairs"][-1] == 100 * 100
    assert evaluate.cluster_curve(h, gold)["threshold"].shape == (64,)
    assert evaluate.cluster_curve(h, gold, max_points=1000)["threshold"].shape == (100,)
    given = evaluate.cluster_curve(h, gold, thresholds=[50.0, -1.0, np.inf])
    assert given["threshold"].tolist() == [50.0, -1.0, np.inf] and given["n_components"].tolist() == [h.n_clusters(50.0), 200, 1]
    with pytest.raises(ValueError, match="NaN"):
        evaluate.cluster_curve(h, gold, thresholds=[0.5, np.nan])
    with pytest.raises(ValueError, match="max_points"):
        evaluate.cluster_curve(h, gold, max_points=0)
