"""The single-linkage hierarchy on the device (kz_forest_csr, kz_forest_lists, kz_components_edges; `matching.single_linkage_csr`,
`matching.single_linkage`, `Kiez.hierarchy_radius`, `Kiez.hierarchy_pairs`, `evaluate.cluster_curve`).  Every case checks two things:
the forest is bit for bit the four arrays and the count of the numpy restatement (tests/hierarchy_restate.py, checked against scipy in
tests/test_hierarchy.py), and `cut(t)` at every distinct forest value (many values: 16 evenly spaced ones plus the two ends) gives the
labels, sizes and count of `matching.components_csr` on the entries with value <= t."""
import ctypes as C

import numpy as np
import pytest

from tests import components_restate as CR
from tests import hierarchy_restate as HR

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


@pytest.fixture(scope="module")
def cases():
    return HR.csr_cases()


@pytest.fixture(scope="module")
def expected(cases):
    """The restatement's forest for every small case, computed once."""
    return {name: HR.forest(*g) for name, g in cases.items()}


def _assert_forest(h, want, where):
    source, target, value, entry, c = want
    for got, ref, what in ((h.source, source, "source"), (h.target, target, "target"), (h.entry, entry, "entry")):
        assert got.dtype == np.int64 and got.shape == ref.shape, (where, what, got.shape, ref.shape)
        np.testing.assert_array_equal(got, ref, err_msg=f"{where}: {what}")
    assert h.value.dtype == np.float64 and h.value.tobytes() == value.tobytes(), f"{where}: value"    # (bytes: -0.0 is not +0.0)
    assert h.n_components == c and h.value.shape[0] == h.n_source + h.n_target - c, where


def _assert_cuts(h, indptr, ind, dist, n_t, where, ts=None):
    from kiez_amd import matching
    ts = HR.thresholds(h.value) if ts is None else ts
    for t in ts:
        sub_ptr, sub_ind = HR.restrict(indptr, ind, dist, t)
        want = matching.components_csr(sub_ptr, sub_ind, n_t, return_sizes=True)
        got = h.cut(float(t), return_sizes=True)
        assert len(got) == 4
        for a, b, what in zip(got, want, ("source_label", "target_label", "n_source_in", "n_target_in")):
            assert a.dtype == np.int64 and a.tobytes() == b.tobytes(), (where, float(t), what)
        assert got[2].shape[0] == h.n_clusters(t), (where, float(t))
    return len(ts)


SMALL = ["random ties", "random ties f32", "all equal", "path increasing", "path random", "hubs", "mixed values", "n_q = 0", "nnz = 0",
         "one entry", "one entry, NaN"]


@pytest.mark.parametrize("name", SMALL)
def test_forest_and_cuts_equal_the_restatement(ctx, cases, expected, name):
    from kiez_amd import matching
    indptr, ind, dist, n_t = cases[name]
    h = matching.single_linkage_csr(indptr, ind, dist, n_t)
    _assert_forest(h, expected[name], name)
    assert 0 <= h.rounds <= 31
    if name.startswith("path"):
        assert h.n_components == 1 and h.value.shape[0] == 3999 and h.rounds >= 1
    if name == "mixed values":
        assert np.isinf(h.value).any() and np.signbit(h.value[h.value == 0.0]).any() and not np.isnan(h.value).any()
    _assert_cuts(h, indptr, ind, dist, n_t, name, ts=np.concatenate([HR.thresholds(h.value), [-np.inf, np.inf]]))
    # the restatement's own cut at the last value, and without sizes
    if h.value.shape[0]:
        t = float(h.value[-1])
        want = HR.cut(indptr, ind, dist, n_t, t)
        got = h.cut(t)
        assert len(got) == 2
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    # device arrays in: the same forest
    dev = matching.single_linkage_csr(ctx.to_device(indptr), ctx.to_device(ind), ctx.to_device(dist), n_t)
    _assert_forest(dev, expected[name], name + " (device)")


@pytest.mark.parametrize("k", [1, 3, 64])
def test_fixed_lists(ctx, k):
    from kiez_amd import matching
    dist, ind, n_t = HR.fixed_lists(k)
    h = matching.single_linkage(dist, ind, n_t)
    _assert_forest(h, HR.forest_lists(dist, ind, n_t), f"lists k={k}")
    indptr = k * np.arange(ind.shape[0] + 1, dtype=np.int64)
    assert _assert_cuts(h, indptr, ind.reshape(-1), dist.reshape(-1), n_t, f"lists k={k}") >= 3
    h32 = matching.single_linkage(ctx.to_device(dist.astype(np.float32)), ctx.to_device(ind), n_t)      # (quarters are exact in float32)
    _assert_forest(h32, HR.forest_lists(dist, ind, n_t), f"lists k={k} f32")


def test_more_than_a_million_nodes_and_entries(ctx):
    """1.1 million nodes with 1.1 million entries: every kernel takes its grid-stride loop (a grid is 4096 x 256 threads), the scan
    over the entries its second level, the sort its radix path."""
    from kiez_amd import matching
    indptr, ind, n_t = CR.random_graph(23, 600_000, 500_000, 1_100_000)
    dist = np.random.default_rng(24).integers(0, 1 << 20, ind.shape[0]) / 1024.0        # ties among 1.1 M draws of 2^20 values
    h = matching.single_linkage_csr(indptr, ind, dist, n_t)
    _assert_forest(h, HR.forest(indptr, ind, dist, n_t), "1.1 M")
    assert h.value.shape[0] > 500_000 and h.rounds <= 31
    assert _assert_cuts(h, indptr, ind, dist, n_t, "1.1 M") == 18       # 16 evenly spaced distinct values plus the two ends


def test_same_bytes_every_time_and_under_permutation(ctx, cases):
    from kiez_amd import matching
    rng = np.random.default_rng(32)

    def permuted(indptr, ind, dist):
        ind, dist = ind.copy(), dist.copy()
        for i in np.flatnonzero(np.diff(indptr) > 1):
            o = indptr[i] + rng.permutation(indptr[i + 1] - indptr[i])
            ind[indptr[i]:indptr[i + 1]], dist[indptr[i]:indptr[i + 1]] = ind[o], dist[o]
        return ind, dist
    for name in ("random ties", "hubs", "path random"):
        indptr, ind, dist, n_t = cases[name]
        a, b = matching.single_linkage_csr(indptr, ind, dist, n_t), matching.single_linkage_csr(indptr, ind, dist, n_t)
        for x, y in zip((a.source, a.target, a.value, a.entry), (b.source, b.target, b.value, b.entry)):
            assert x.tobytes() == y.tobytes(), name
        # with ties: another forest, the same cuts
        p_ind, p_dist = permuted(indptr, ind, dist)
        p = matching.single_linkage_csr(indptr, p_ind, p_dist, n_t)
        assert p.value.tobytes() == a.value.tobytes() and p.n_components == a.n_components
        for t in HR.thresholds(a.value):
            for x, y in zip(a.cut(float(t), return_sizes=True), p.cut(float(t), return_sizes=True)):
                assert x.tobytes() == y.tobytes(), (name, float(t))
    # distinct weights: the same forest edges
    indptr, ind, _, n_t = cases["random ties"]
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    keep = np.zeros(ind.shape[0], dtype=bool)         # one entry per pair: a pair stored twice would be two edges of two weights
    keep[np.unique(rows * n_t + ind, return_index=True)[1]] = True
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(indptr) - 1))]).astype(np.int64)
    ind = ind[keep]
    dist = rng.permutation(ind.shape[0]).astype(np.float64)
    a = matching.single_linkage_csr(ptr, ind, dist, n_t)
    p_ind, p_dist = permuted(ptr, ind, dist)
    p = matching.single_linkage_csr(ptr, p_ind, p_dist, n_t)
    assert not np.array_equal(p_ind, ind)
    for x, y in zip((a.source, a.target, a.value), (p.source, p.target, p.value)):
        assert x.tobytes() == y.tobytes()


def test_components_edges_directly(ctx, cases):
    """An edge list in arbitrary order with repeated edges and ids out of range, against `components_csr` of the same pairs."""
    from kiez_amd import _native as N
    from kiez_amd import matching
    indptr, ind, _, n_t = cases["random ties"]
    n_q = len(indptr) - 1
    rng = np.random.default_rng(33)
    rows = np.repeat(np.arange(n_q, dtype=np.int64), np.diff(indptr))
    want = matching.components_csr(indptr, ind, n_t, return_sizes=True)
    order = rng.permutation(np.concatenate([np.arange(ind.shape[0]), rng.integers(0, ind.shape[0], 200)]))
    src = np.concatenate([rows[order], [-1, n_q, 0, 2 ** 40, 5]])
    tgt = np.concatenate([ind[order], [0, 0, -1, 3, n_t]])
    s_dev, t_dev = ctx.to_device(src), ctx.to_device(tgt)
    got = N.components_edges(ctx, s_dev, t_dev, n_q, n_t, sizes=True)
    for a, b in zip(got[:4], want):
        assert a.numpy().tobytes() == b.tobytes()
    assert got[4] == want[2].shape[0] and len(N.components_edges(ctx, s_dev, t_dev, n_q, n_t)) == 3
    none = N.components_edges(ctx, s_dev, t_dev, n_q, n_t, count=0)
    np.testing.assert_array_equal(none[0].numpy(), np.arange(n_q))
    np.testing.assert_array_equal(none[1].numpy(), n_q + np.arange(n_t))
    with pytest.raises(ValueError, match="count"):
        N.components_edges(ctx, s_dev, t_dev, n_q, n_t, count=src.shape[0] + 1)
    with pytest.raises(ValueError, match="int64"):
        N.components_edges(ctx, ctx.to_device(src.astype(np.int32)), t_dev, n_q, n_t)


def test_limits_come_before_any_launch_and_nothing_is_written_behind_the_counts(ctx, cases, expected):
    SENT = -12345
    tiny = [ctx.to_device(np.full(2, SENT, dtype=np.int64)) for _ in range(7)]
    val = ctx.to_device(np.full(2, -7.0))
    m, c, rounds = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
    lib = ctx.lib
    tail = (tiny[2].ptr, tiny[3].ptr, val.ptr, tiny[4].ptr, C.byref(m), C.byref(c), C.byref(rounds))
    for n_q, n_t in ((2 ** 30, 2 ** 30 - 1), (2 ** 31 - 2, 1), (1, 2 ** 31 - 2), (0, 2 ** 31 - 1)):
        want = 3 if n_t < 2 ** 31 - 1 else 1
        assert lib.kz_forest_csr(ctx.handle, tiny[0].ptr, tiny[1].ptr, val.ptr, 1, n_q, 2, n_t, *tail) == want, (n_q, n_t)
        assert lib.kz_forest_lists(ctx.handle, val.ptr, 1, tiny[1].ptr, n_q, 1, n_t, *tail) == want, (n_q, n_t)
        assert lib.kz_components_edges(ctx.handle, tiny[0].ptr, tiny[1].ptr, 2, n_q, n_t, tiny[2].ptr, tiny[3].ptr, tiny[5].ptr, tiny[6].ptr,
                                       C.byref(c)) == want, (n_q, n_t)
    assert lib.kz_forest_lists(ctx.handle, val.ptr, 1, tiny[1].ptr, 2 ** 20, 2 ** 11, 5, *tail) == 3
    assert "2^31 - 2" in lib.kz_last_error().decode()
    assert lib.kz_forest_lists(ctx.handle, val.ptr, 1, tiny[1].ptr, 4, 0, 5, *tail) == 1                 # k = 0
    assert lib.kz_forest_lists(ctx.handle, val.ptr, 2, tiny[1].ptr, 1, 1, 5, *tail) == 1                 # a float16 list
    assert lib.kz_forest_csr(ctx.handle, tiny[0].ptr, tiny[1].ptr, val.ptr, 7, 1, 1, 5, *tail) == 1
    assert lib.kz_forest_csr(ctx.handle, tiny[0].ptr, tiny[1].ptr, val.ptr, 1, 1, 1, 5, None, *tail[1:]) == 1   # a null output
    assert (m.value, c.value, rounds.value) == (-1, -1, -1)
    for a in tiny:
        np.testing.assert_array_equal(a.numpy(), [SENT, SENT])
    np.testing.assert_array_equal(val.numpy(), [-7.0, -7.0])
    # a device indptr that decreases: refused before anything reads through it
    from kiez_amd import matching
    with pytest.raises(ValueError, match="indptr must start at 0, never decrease and end at nnz"):
        matching.single_linkage_csr(ctx.to_device(np.array([0, 2, 1, 3], dtype=np.int64)), ctx.to_device(np.array([0, 1, 1], dtype=np.int64)),
                                    ctx.to_device(np.array([0.5, 0.25, 1.0])), 3)
    # sentinel-filled outputs of full size: nothing behind m is written
    indptr, ind, dist, n_t = cases["random ties"]
    n_q, want = len(indptr) - 1, expected["random ties"]
    room = n_q + n_t - 1
    out = [ctx.to_device(np.full(room, SENT, dtype=np.int64)) for _ in range(3)]
    out_v = ctx.to_device(np.full(room, -7.0))
    ptr_dev, ind_dev, dist_dev = ctx.to_device(indptr), ctx.to_device(ind), ctx.to_device(dist)
    rc = lib.kz_forest_csr(ctx.handle, ptr_dev.ptr, ind_dev.ptr, dist_dev.ptr, 1, n_q, ind.shape[0], n_t, out[0].ptr, out[1].ptr, out_v.ptr,
                           out[2].ptr, C.byref(m), C.byref(c), None)
    assert rc == 0 and m.value == want[2].shape[0] < room and c.value == want[4]
    for a, ref in zip(out, (want[0], want[1], want[3])):
        np.testing.assert_array_equal(a.numpy(), np.concatenate([ref, np.full(room - m.value, SENT)]))
    np.testing.assert_array_equal(out_v.numpy(), np.concatenate([want[2], np.full(room - m.value, -7.0)]))
    # ... and kz_components_edges writes nothing behind C in its size arrays: a cut of that forest at its 200th edge
    t = want[2][199]
    sub_ptr, sub_ind = HR.restrict(indptr, ind, dist, t)
    count = int(np.searchsorted(want[2], t, side="right"))              # (the prefix of the cut at t: 200 edges or more, fewer than m)
    assert 200 <= count < m.value
    ref = matching.components_csr(sub_ptr, sub_ind, n_t, return_sizes=True)
    n_c = ref[2].shape[0]
    size_q, size_t = (ctx.to_device(np.full(n_q + n_t, SENT, dtype=np.int64)) for _ in range(2))
    label_q, label_t = ctx.to_device(np.full(n_q, SENT, dtype=np.int64)), ctx.to_device(np.full(n_t, SENT, dtype=np.int64))
    rc = lib.kz_components_edges(ctx.handle, out[0].ptr, out[1].ptr, count, n_q, n_t, label_q.ptr, label_t.ptr, size_q.ptr, size_t.ptr,
                                 C.byref(c))
    assert rc == 0 and c.value == n_c == n_q + n_t - count < n_q + n_t
    np.testing.assert_array_equal(label_q.numpy(), ref[0])
    np.testing.assert_array_equal(label_t.numpy(), ref[1])
    np.testing.assert_array_equal(size_q.numpy(), np.concatenate([ref[2], np.full(n_q + n_t - n_c, SENT)]))
    np.testing.assert_array_equal(size_t.numpy(), np.concatenate([ref[3], np.full(n_q + n_t - n_c, SENT)]))
    # one size array without the other: refused
    assert lib.kz_components_edges(ctx.handle, out[0].ptr, out[1].ptr, count, n_q, n_t, label_q.ptr, label_t.ptr, size_q.ptr, None,
                                   C.byref(c)) == 1


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_400():
    """A planted alignment: the targets are the sources plus noise, in another order."""
    rng = np.random.default_rng(42)
    source = rng.standard_normal((400, 16))
    perm = rng.permutation(400)
    target = np.empty_like(source)
    target[perm] = source + 0.15 * rng.standard_normal((400, 16))
    return source, target, perm


def _kiez(hubness, **kwargs):
    from kiez_amd import Kiez
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=hubness, hubness_kwargs=kwargs or None)


@pytest.mark.parametrize("hubness, kwargs", [("CSLS", {}), ("MutualProximity", {"method": "normal"})])
def test_facade_cuts_equal_the_calls_they_replace(rows_400, hubness, kwargs):
    from kiez_amd import matching
    source, target, _ = rows_400
    kz = _kiez(hubness, **kwargs).fit(source, target)
    values = kz.radius_neighbors(np.inf, reduced=True)[2]
    r = float(np.partition(values, 1600)[1600])                             # about four pairs per row
    h = kz.hierarchy_radius(r, reduced=True)
    assert isinstance(h, matching.Hierarchy) and (h.n_source, h.n_target) == (400, 400) and h.value.max() <= r
    for t in (float(np.partition(values, 300)[300]), float(np.partition(values, 800)[800]), float(np.partition(values, 1200)[1200]), r):
        want = kz.components_radius(t, reduced=True, return_sizes=True)
        got = h.cut(t, return_sizes=True)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), (hubness, t)
        assert h.n_clusters(t) == want[2].shape[0]
    indptr, ind, dist = kz.neighbor_pairs(10, mode="mutual", reduced=True)
    hp = kz.hierarchy_pairs(10, "mutual", reduced=True)
    _assert_forest(hp, HR.forest(indptr, ind, dist, 400), f"pairs {hubness}")
    assert _assert_cuts(hp, indptr, ind, dist, 400, f"pairs {hubness}") == 18
    dev = hp.cut_device(float(hp.value[-1]))
    assert len(dev) == 2 and not isinstance(dev[0], np.ndarray)
    np.testing.assert_array_equal(dev[0].numpy(), kz.components_pairs(10, "mutual", reduced=True)[0])


def test_cluster_curve_finds_the_best_cut(rows_400):
    from kiez_amd.evaluate import cluster_curve, cluster_metrics
    source, target, perm = rows_400
    kz = _kiez("CSLS").fit(source, target)
    values = kz.radius_neighbors(np.inf, reduced=True)[2]
    h = kz.hierarchy_radius(float(np.partition(values, 1600)[1600]), reduced=True)
    gold = perm.astype(np.int64)
    curve = cluster_curve(h, gold, max_points=32)
    assert curve["threshold"].shape == (32,) and curve["threshold"][-1] == h.value[-1]
    one_by_one = [cluster_metrics(*h.cut(float(t)), gold) for t in curve["threshold"]]
    f1 = [p["f1"] for p in one_by_one]
    assert curve["f1"].tolist() == f1 and curve["f1"][curve["best"]] == max(f1) and curve["best"] == f1.index(max(f1))
    assert curve["n_components"].tolist() == [h.n_clusters(t) for t in curve["threshold"]]
    assert curve["n_pairs"].tolist() == [p["n_pairs"] for p in one_by_one]
    assert max(f1) > 0.5 and max(f1) > f1[-1]                              # the planted alignment is found below the loosest cut


def test_what_the_facade_refuses(rows_400):
    source, target, _ = rows_400
    for reduced in (False, True):
        single = _kiez("CSLS").fit(np.array(source))
        for call in (lambda: single.hierarchy_radius(1.0, reduced=reduced), lambda: single.hierarchy_pairs(3, reduced=reduced)):
            with pytest.raises(NotImplementedError):
                call()
    from kiez_amd import Kiez
    for hubness, kwargs in (("MutualProximity", {"method": "empiric"}), ("DisSimLocal", None)):
        kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine" if kwargs else "euclidean"}, hubness=hubness,
                  hubness_kwargs=kwargs).fit(source, target)
        for ours, theirs in ((lambda: kz.hierarchy_radius(0.5, reduced=True), lambda: kz.components_radius(0.5, reduced=True)),
                             (lambda: kz.hierarchy_pairs(3, reduced=True), lambda: kz.components_pairs(3, reduced=True))):
            with pytest.raises(NotImplementedError) as want:
                theirs()
            with pytest.raises(NotImplementedError) as got:
                ours()
            assert str(got.value) == str(want.value)                         # refused in the same words
    with pytest.raises(ValueError, match="mode must be one of"):
        kz.hierarchy_pairs(3, mode="all")
    assert kz.hierarchy_radius(0.5).n_source == 400                          # (the plain call is served)
