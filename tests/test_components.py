"""Entity clusters (connected components of a pair list), the part that needs no GPU: the numpy restatement
(tests/components_restate.py) against scipy's connected_components on every graph the GPU tests run, the conditions that keep those
graphs from being vacuous, the errors `matching.components*` raise before the device is touched, and `evaluate.cluster_metrics`."""
import numpy as np
import pytest

from tests import components_restate as CR


@pytest.fixture(scope="module")
def graphs():
    return CR.all_graphs()


def test_restatement_equals_scipy_on_every_graph(graphs):
    assert len(graphs) == 15
    for name, (indptr, ind, n_t) in graphs.items():
        n_q = len(indptr) - 1
        src, tgt, ns, nt, c = CR.components(indptr, ind, n_t)
        want_c, want = CR.scipy_components(indptr, ind, n_t)
        assert c == want_c, name
        np.testing.assert_array_equal(np.concatenate([src, tgt]), want, err_msg=name)
        # sizes: every node counted once, on its side
        assert ns.sum() == n_q and nt.sum() == n_t and ns.shape == nt.shape == (c,), name
        np.testing.assert_array_equal(ns, np.bincount(src, minlength=c), err_msg=name)
        np.testing.assert_array_equal(nt, np.bincount(tgt, minlength=c), err_msg=name)
        if n_q:
            assert src[0] == 0, name


def test_the_graphs_are_what_they_are_meant_to_be(graphs):
    sizes = CR.component_sizes(*graphs["mixed"])
    assert sizes.max() >= 100 and (sizes == 1).sum() >= 100 and ((sizes >= 2) & (sizes <= 10)).sum() >= 100
    sizes = CR.component_sizes(*graphs["near giant"])
    assert sizes.max() >= 3000 and graphs["near giant"][1].shape[0] == 3999
    indptr, ind, n_t = graphs["hub"]
    assert np.diff(indptr).max() == 5000 > 4096 and np.bincount(ind[:5000], minlength=7).min() >= 600   # a long row; ~700 listers each
    assert CR.components(indptr, ind, n_t)[4] == 1
    for name in ("path a", "path b"):
        src, tgt, ns, nt, c = CR.components(*graphs[name])
        assert c == 1 and not src.any() and not tgt.any() and ns[0] == nt[0] == 2000
    assert not np.array_equal(graphs["path a"][1], graphs["path b"][1])
    src, tgt, ns, nt, c = CR.components(*graphs["many chains"])
    assert c == 100 and (ns == 20).all() and (nt == 20).all()
    # degenerate: the answers by hand
    deg = CR.degenerate()
    np.testing.assert_array_equal(np.concatenate(CR.components(*deg["nnz = 0"])[:2]), np.arange(9))
    src, tgt, ns, nt, c = CR.components(*deg["n_q = 0"])
    np.testing.assert_array_equal(tgt, np.arange(6))
    assert src.shape == (0,) and c == 6 and not ns.any() and (nt == 1).all()
    assert [a.tolist() for a in CR.components(*deg["1 x 1 with the edge"])[:4]] == [[0], [0], [1], [1]]
    assert [a.tolist() for a in CR.components(*deg["1 x 1 without"])[:4]] == [[0], [1], [1, 0], [0, 1]]
    assert CR.components(*deg["every entry out of range"])[4] == 6
    src, tgt, ns, nt, c = CR.components(*deg["duplicates"])     # rows 0 and 1 share target 0; row 2 has target 2; target 3 alone
    assert src.tolist() == [0, 0, 1] and tgt.tolist() == [0, 0, 1, 2] and ns.tolist() == [2, 1, 0] and nt.tolist() == [2, 1, 1]
    for k in (1, 3, 64):
        ind, n_t = CR.fixed_lists(k)
        assert ind.shape == (300, k) and (ind == -1).any() and (ind == n_t).any()
        c = CR.components_lists(ind, n_t)[4]
        assert 100 < c < 500 - 50     # pairs exist, and not everything is one cluster


def test_permuting_a_row_changes_nothing(graphs):
    indptr, ind, n_t = graphs["mixed"]
    rng = np.random.default_rng(11)
    perm = ind.copy()
    for i in range(len(indptr) - 1):
        perm[indptr[i]:indptr[i + 1]] = rng.permutation(ind[indptr[i]:indptr[i + 1]])
    for a, b in zip(CR.components(indptr, ind, n_t)[:4], CR.components(indptr, perm, n_t)[:4]):
        np.testing.assert_array_equal(a, b)


def test_argument_errors_come_before_the_device(monkeypatch):
    from kiez_amd import Kiez, NotFittedError
    from kiez_amd import _native as N
    from kiez_amd import matching

    def no_device(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N, "load", no_device)
    indptr, ind = np.array([0, 2, 3]), np.array([0, 1, 1])
    for bad_ptr, bad_ind, n_target in [(indptr, ind, 0), (indptr, ind, 2.0), (indptr, ind, True), (indptr, ind.astype(np.float64), 3),
                                       (indptr, ind.reshape(3, 1), 3), (indptr.astype(np.float64), ind, 3), (indptr.reshape(1, 3), ind, 3),
                                       (np.zeros(0, dtype=np.int64), ind, 3),
                                       (np.array([1, 2, 3]), ind, 3), (np.array([0, 3, 2]), ind, 3), (np.array([0, 2, 4]), ind, 3),
                                       (indptr, ind, 2 ** 31 - 3)]:             # 2 source rows + 2^31 - 3 target rows: one node too many
        with pytest.raises(ValueError):
            matching.components_csr(bad_ptr, bad_ind, n_target)
    with pytest.raises(ValueError, match="limit is 2147483646"):
        matching.components_csr(indptr, ind, 2 ** 31 - 3, return_sizes=True)
    lists = np.array([[0, 1], [1, -1]])
    for bad, n_target in [(lists, 0), (lists, 1.5), (lists, False), (lists[0], 3), (lists.astype(np.float32), 3), (lists == 1, 3),
                          (np.zeros((4, 0), dtype=np.int64), 3), (lists, 2 ** 31 - 3)]:
        with pytest.raises(ValueError):
            matching.components(bad, n_target)
    # the facade: the producing call's own checks
    for call in (lambda kz: kz.components_radius(0.5), lambda kz: kz.components_pairs(3, mode="mutual", return_sizes=True)):
        with pytest.raises(NotFittedError):
            call(Kiez())


def test_the_interface():
    import inspect

    from kiez_amd import Kiez, matching
    sig = inspect.signature(matching.components_csr)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("n_target", inspect.Parameter.empty), ("return_sizes", False), ("ctx", None)]
    sig = inspect.signature(matching.components)
    assert [p.name for p in sig.parameters.values()] == ["ind", "n_target", "return_sizes", "ctx"]
    for name, want in (("components_radius", [("radius", inspect.Parameter.empty), ("reduced", False), ("return_sizes", False)]),
                       ("components_pairs", [("k", None), ("mode", "union"), ("reduced", False), ("return_sizes", False)])):
        for fn in (getattr(Kiez, name), getattr(Kiez, name + "_device")):
            assert [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]] == want


# ---- evaluate.cluster_metrics ----------------------------------------------------------------------------------------------------
def test_cluster_metrics_all_singletons():
    from kiez_amd.evaluate import cluster_metrics
    m = cluster_metrics(np.arange(4), np.arange(4, 9), {0: 0, 1: 1})
    assert m == {"precision": 0.0, "recall": 0.0, "f1": 0.0, "n_pairs": 0, "n_true": 0, "n_gold": 2, "n_components": 9}
    assert isinstance(m["n_pairs"], int)


def test_cluster_metrics_one_two_by_three_cluster():
    from kiez_amd.evaluate import cluster_metrics
    # sources 0, 1 and targets 0, 1, 2 are cluster 0; source 2 is cluster 1, target 3 cluster 2
    src, tgt = np.array([0, 0, 1]), np.array([0, 0, 0, 2])
    gold = {0: 1, 2: 3}                                    # (0, 1) lies in the cluster, (2, 3) joins two clusters
    m = cluster_metrics(src, tgt, gold)
    assert m["n_pairs"] == 6 and m["n_true"] == 1 and m["n_gold"] == 2 and m["n_components"] == 3
    assert m["precision"] == 1 / 6 and m["recall"] == 0.5 and m["f1"] == pytest.approx(2 * (1 / 6) * 0.5 / (1 / 6 + 0.5))
    # gold as the array with -1 for none: the same numbers
    assert cluster_metrics(src, tgt, np.array([1, -1, 3])) == m
    assert cluster_metrics(src.tolist(), tgt.astype(np.int32), np.array([1, -1, 3], dtype=np.int32)) == m


def test_cluster_metrics_gold_out_of_range_and_bad_input():
    from kiez_amd.evaluate import cluster_metrics
    src, tgt = np.array([0, 0, 1]), np.array([0, 0, 0, 2])
    # a gold target that is no target row, a gold key that is no source row: both count in n_gold only
    m = cluster_metrics(src, tgt, {0: 1, 1: 4, 7: 0})
    assert m["n_true"] == 1 and m["n_gold"] == 3 and m["recall"] == 1 / 3
    m = cluster_metrics(src, tgt, np.array([1, 4, 2 ** 40]))
    assert m["n_true"] == 1 and m["n_gold"] == 3
    m = cluster_metrics(src, tgt, {})
    assert m["recall"] == 0.0 and m["f1"] == 0.0 and m["n_gold"] == 0 and m["precision"] == 0.0
    with pytest.raises(ValueError):
        cluster_metrics(src.astype(np.float64), tgt, {})
    with pytest.raises(ValueError):
        cluster_metrics(src, tgt - 1, {})
    with pytest.raises(ValueError):
        cluster_metrics(src, tgt, np.array([1, -1]))       # one gold id per source row


def test_cluster_metrics_on_the_restatement(graphs):
    """n_pairs is the sum over the clusters of (source rows x target rows); every stored pair is an implied pair."""
    from kiez_amd.evaluate import cluster_metrics
    indptr, ind, n_t = graphs["mixed"]
    src, tgt, ns, nt, c = CR.components(indptr, ind, n_t)
    gold = np.full(len(indptr) - 1, -1)
    has = np.diff(indptr) > 0
    gold[has] = ind[indptr[:-1][has]]                      # the first listed target of every row that lists one: in its cluster
    m = cluster_metrics(src, tgt, gold)
    assert m["n_pairs"] == int((ns * nt).sum()) and m["n_components"] == c
    assert m["n_true"] == m["n_gold"] == int(has.sum()) and m["recall"] == 1.0
