"""Entity clusters on the device (kz_components_csr, kz_components_lists; `matching.components_csr`, `matching.components`,
`Kiez.components_radius`, `Kiez.components_pairs`) against the numpy restatement (tests/components_restate.py, checked against scipy
in tests/test_components.py): both label arrays, both size arrays and the count, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import components_restate as CR

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


@pytest.fixture(scope="module")
def graphs():
    return CR.all_graphs()


@pytest.fixture(scope="module")
def expected(graphs):
    """The restatement's answer for every graph, computed once."""
    return {name: CR.components(*g) for name, g in graphs.items()}


def _assert_same(got, want, where):
    assert len(got) == 4
    for a, b, what in zip(got, want[:4], ("source_label", "target_label", "n_source_in", "n_target_in")):
        assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == b.shape, (where, what, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{where}: {what}")


GRAPHS = ["mixed", "near giant", "hub", "path a", "path b", "many chains", "nnz = 0", "n_q = 0", "1 x 1 with the edge", "1 x 1 without",
          "every entry out of range", "duplicates"]


@pytest.mark.parametrize("name", GRAPHS)
def test_components_csr_equals_the_restatement(ctx, graphs, expected, name):
    from kiez_amd import matching
    indptr, ind, n_t = graphs[name]
    want = expected[name]
    got = matching.components_csr(indptr, ind, n_t, return_sizes=True)
    _assert_same(got, want, name)
    assert got[2].shape == (want[4],)
    # device arrays in: device arrays out, the same bytes; the native count
    from kiez_amd import _native as N
    dev = matching.components_csr(ctx.to_device(indptr), ctx.to_device(ind), n_t, return_sizes=True)
    assert all(isinstance(a, N.DeviceArray) for a in dev)
    _assert_same(tuple(a.numpy() for a in dev), want, name + " (device)")
    assert N.components_csr(ctx, ctx.to_device(indptr), ctx.to_device(ind), n_t)[2] == want[4]
    if name.startswith("path"):
        assert want[4] == 1 and not got[0].any() and not got[1].any()


@pytest.mark.parametrize("k", [1, 3, 64])
def test_fixed_lists_equal_the_csr_call(ctx, graphs, expected, k):
    from kiez_amd import matching
    ind, n_t = CR.fixed_lists(k)
    got = matching.components(ind, n_t, return_sizes=True)
    _assert_same(got, expected[f"lists k={k}"], f"lists k={k}")
    indptr, flat, _ = graphs[f"lists k={k}"]
    for a, b in zip(got, matching.components_csr(indptr, flat, n_t, return_sizes=True)):
        np.testing.assert_array_equal(a, b)
    dev = matching.components(ctx.to_device(ind), n_t)
    assert len(dev) == 2
    np.testing.assert_array_equal(dev[0].numpy(), got[0])
    np.testing.assert_array_equal(dev[1].numpy(), got[1])


def test_more_nodes_than_one_grid_and_more_tiles_than_one_scan_round(ctx):
    """1.1 million nodes: the node kernels take their grid-stride loop (a grid is 4096 x 256 threads) and the second level of the
    prefix sum 17 rounds of 256 tiles; 300 000 entries, most nodes singletons."""
    from kiez_amd import matching
    indptr, ind, n_t = CR.random_graph(21, 600_000, 500_000, 300_000)
    want = CR.components(indptr, ind, n_t)
    _assert_same(matching.components_csr(indptr, ind, n_t, return_sizes=True), want, "1.1 M nodes")


def test_more_list_entries_than_one_grid(ctx):
    """[17 000, 64] lists, 1 088 000 entries of which about 25 000 are pairs: the hook kernel takes its grid-stride loop."""
    from kiez_amd import matching
    rng = np.random.default_rng(22)
    n_q, k, n_t = 17_000, 64, 15_000
    ind = np.where(rng.random((n_q, k)) < 1.5 / k, rng.integers(0, n_t, (n_q, k)), -1).astype(np.int64)
    want = CR.components_lists(ind, n_t)
    assert want[2].max() + want[3].max() > 50
    _assert_same(matching.components(ind, n_t, return_sizes=True), want, "1.09 M entries")


def test_same_bits_every_time(ctx, graphs, expected):
    from kiez_amd import matching
    rng = np.random.default_rng(31)
    for name in ("mixed", "hub", "path a"):
        indptr, ind, n_t = graphs[name]
        first = matching.components_csr(indptr, ind, n_t, return_sizes=True)
        again = matching.components_csr(indptr, ind, n_t, return_sizes=True)
        perm = ind.copy()
        for i in np.flatnonzero(np.diff(indptr) > 1):
            perm[indptr[i]:indptr[i + 1]] = rng.permutation(ind[indptr[i]:indptr[i + 1]])
        permuted = matching.components_csr(indptr, perm, n_t, return_sizes=True)
        labels_only = matching.components_csr(indptr, ind, n_t)
        assert len(labels_only) == 2
        for a, b, c in zip(first, again, permuted):
            assert a.tobytes() == b.tobytes() == c.tobytes(), name
        assert labels_only[0].tobytes() == first[0].tobytes() and labels_only[1].tobytes() == first[1].tobytes(), name


def test_size_arrays_are_written_up_to_the_count_only(ctx, graphs, expected):
    from kiez_amd import _native as N
    indptr, ind, n_t = graphs["many chains"]
    n_q, c = len(indptr) - 1, expected["many chains"][4]
    SENT = -12345
    size_q, size_t = ctx.to_device(np.full(n_q + n_t, SENT, dtype=np.int64)), ctx.to_device(np.full(n_q + n_t, SENT, dtype=np.int64))
    label_q, label_t = ctx.empty((n_q,), np.int64), ctx.empty((n_t,), np.int64)
    ptr_dev, ind_dev = ctx.to_device(indptr), ctx.to_device(ind)     # (named: a device array is released with its Python object)
    count = C.c_int64(-1)
    rc = ctx.lib.kz_components_csr(ctx.handle, ptr_dev.ptr, ind_dev.ptr, n_q, ind.shape[0], n_t, label_q.ptr, label_t.ptr,
                                   size_q.ptr, size_t.ptr, C.byref(count))
    assert rc == 0 and count.value == c == 100
    np.testing.assert_array_equal(size_q.numpy(), np.concatenate([np.full(c, 20), np.full(n_q + n_t - c, SENT)]))
    np.testing.assert_array_equal(size_t.numpy(), np.concatenate([np.full(c, 20), np.full(n_q + n_t - c, SENT)]))
    # one size array without the other: refused, nothing written
    rc = ctx.lib.kz_components_csr(ctx.handle, ptr_dev.ptr, ind_dev.ptr, n_q, ind.shape[0], n_t, label_q.ptr, label_t.ptr,
                                   size_q.ptr, None, C.byref(count))
    assert rc == 1


def test_a_bad_indptr_is_a_value_error(ctx):
    from kiez_amd import matching
    ind = ctx.to_device(np.array([0, 1, 1], dtype=np.int64))
    for bad in ([0, 2, 1, 3], [0, 1, 2, 4], [0, 1, 2, 2], [1, 1, 2, 3]):     # decreases; ends beyond nnz; ends before it; starts at 1
        with pytest.raises(ValueError, match="indptr must start at 0, never decrease and end at nnz"):
            matching.components_csr(ctx.to_device(np.array(bad, dtype=np.int64)), ind, 3)
        with pytest.raises(ValueError, match="indptr must start at 0"):      # (a host indptr: before the device is touched)
            matching.components_csr(np.array(bad), np.array([0, 1, 1]), 3)


def test_the_node_limit_is_decided_before_anything_is_read(ctx):
    """n_q + n_index at the limit: KZ_ERR_UNSUPPORTED (3) with 16-byte buffers that no kernel may touch; the outputs keep their bytes."""
    from kiez_amd import _native as N
    SENT = 77
    tiny = [ctx.to_device(np.full(2, SENT, dtype=np.int64)) for _ in range(6)]
    count = C.c_int64(-1)
    for n_q, n_t in ((2 ** 30, 2 ** 30 - 1), (2 ** 31 - 2, 1), (1, 2 ** 31 - 2), (0, 2 ** 31 - 1)):
        rc = ctx.lib.kz_components_csr(ctx.handle, tiny[0].ptr, tiny[1].ptr, n_q, 2, n_t, tiny[2].ptr, tiny[3].ptr, tiny[4].ptr, tiny[5].ptr,
                                       C.byref(count))
        assert rc == (3 if n_t < 2 ** 31 - 1 else 1), (n_q, n_t)             # (n_index alone beyond its range: kz_csr_require's INVALID)
        rc = ctx.lib.kz_components_lists(ctx.handle, tiny[1].ptr, n_q, 1, n_t, tiny[2].ptr, tiny[3].ptr, tiny[4].ptr, tiny[5].ptr, C.byref(count))
        assert rc == (3 if n_t < 2 ** 31 - 1 else 1), (n_q, n_t)
    # lists: n_q k beyond 2^31 - 2
    rc = ctx.lib.kz_components_lists(ctx.handle, tiny[1].ptr, 2 ** 20, 2 ** 11, 5, tiny[2].ptr, tiny[3].ptr, None, None, C.byref(count))
    assert rc == 3
    assert "2^31 - 2" in ctx.lib.kz_last_error().decode()
    rc = ctx.lib.kz_components_lists(ctx.handle, tiny[1].ptr, 4, 0, 5, tiny[2].ptr, tiny[3].ptr, None, None, C.byref(count))
    assert rc == 1
    assert count.value == -1
    for a in tiny:
        np.testing.assert_array_equal(a.numpy(), [SENT, SENT])
    with pytest.raises(NotImplementedError, match="node ids are int32"):
        N._check(ctx.lib.kz_components_csr(ctx.handle, tiny[0].ptr, tiny[1].ptr, 2 ** 30, 2, 2 ** 30, tiny[2].ptr, tiny[3].ptr, None, None,
                                           C.byref(count)))


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_300_280():
    rng = np.random.default_rng(41)
    return rng.standard_normal((300, 16)), rng.standard_normal((280, 16))


def _kiez(hubness):
    from kiez_amd import Kiez
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hubness)


@pytest.mark.parametrize("hubness", [None, "CSLS"])
def test_facade_equals_components_of_the_producing_call(rows_300_280, hubness):
    from kiez_amd import matching
    from kiez_amd.evaluate import cluster_metrics
    source, target = rows_300_280
    kz = _kiez(hubness).fit(source, target)
    for reduced in (False, True):
        plain = kz.radius_neighbors(np.inf, reduced=reduced)[2]
        r = float(np.partition(plain, 900)[900])                             # about three pairs per row
        indptr, ind, _ = kz.radius_neighbors(r, reduced=reduced)
        assert 600 < ind.shape[0] < 1400
        got = kz.components_radius(r, reduced=reduced, return_sizes=True)
        _assert_same(got, CR.components(indptr, ind, 280), f"radius {hubness} {reduced}")
        for a, b in zip(got, matching.components_csr(indptr, ind, 280, return_sizes=True)):
            np.testing.assert_array_equal(a, b)
        assert len(kz.components_radius(r, reduced=reduced)) == 2
        for k, mode in ((3, "union"), (5, "mutual"), (2, "forward"), (2, "reverse")):
            indptr, ind = kz.neighbor_pairs(k, mode=mode, reduced=reduced, return_distance=False)
            got = kz.components_pairs(k, mode=mode, reduced=reduced, return_sizes=True)
            _assert_same(got, CR.components(indptr, ind, 280), f"pairs {hubness} {reduced} {mode}")
        dev = kz.components_pairs_device(3, reduced=reduced)
        assert len(dev) == 2 and not isinstance(dev[0], np.ndarray)
        np.testing.assert_array_equal(dev[0].numpy(), kz.components_pairs(3, reduced=reduced)[0])


def test_mutual_nearest_neighbours_are_the_one_to_one_clusters(rows_300_280):
    source, target = rows_300_280
    kz = _kiez("CSLS").fit(source, target)
    src, tgt, ns, nt = kz.components_pairs(1, mode="mutual", return_sizes=True)
    assert ns.max() <= 1 and nt.max() <= 1 and (ns + nt).min() >= 1
    match = kz.match_pairs(1, mode="mutual", return_distance=False)
    paired = np.flatnonzero((ns == 1) & (nt == 1))
    assert 10 < paired.shape[0] == np.count_nonzero(match >= 0)
    rows = np.flatnonzero(match >= 0)
    np.testing.assert_array_equal(src[rows], tgt[match[rows]])               # a matched pair shares its cluster ...
    np.testing.assert_array_equal(np.sort(src[rows]), paired)                # ... and those are all the (1, 1) clusters


def test_radius_inf_is_one_cluster_with_every_pair(rows_300_280):
    from kiez_amd.evaluate import cluster_metrics
    source, target = rows_300_280
    kz = _kiez(None).fit(source, target)
    src, tgt, ns, nt = kz.components_radius(np.inf, return_sizes=True)
    assert ns.tolist() == [300] and nt.tolist() == [280] and not src.any() and not tgt.any()
    gold = {i: (7 * i) % 280 for i in range(0, 300, 3)}
    m = cluster_metrics(src, tgt, gold)
    assert m["recall"] == 1.0 and m["n_pairs"] == 300 * 280 and m["n_true"] == m["n_gold"] == 100 and m["n_components"] == 1
    dev = kz.components_radius_device(np.inf)
    assert cluster_metrics(dev[0], dev[1], gold) == m                        # device arrays are brought to the host


def test_what_the_facade_refuses(rows_300_280):
    source, target = rows_300_280
    for reduced in (False, True):
        single = _kiez("CSLS").fit(np.array(source))
        for call in (lambda: single.components_radius(1.0, reduced=reduced), lambda: single.components_pairs(3, reduced=reduced)):
            with pytest.raises(NotImplementedError):
                call()
    from kiez_amd import Kiez
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="MutualProximity",
              hubness_kwargs={"method": "empiric"}).fit(source, target)
    with pytest.raises(NotImplementedError):
        kz.components_radius(0.5, reduced=True)
    with pytest.raises(NotImplementedError):
        kz.components_pairs(3, reduced=True)
    with pytest.raises(ValueError, match="mode must be one of"):
        kz.components_pairs(3, mode="all")
    assert len(kz.components_radius(3.0)) == 2                               # (the plain call is served)
