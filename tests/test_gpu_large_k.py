"""kz_knn from 541 to 4096 neighbours per query: the range where no fused kernel runs and every row is answered by the exact float64
kernels (kz_exact.h: kz_exact_dist_* and the family / boolean distance kernels, kz_exact_chunk_kernel / kz_exact_chunk_radix_kernel,
kz_exact_select_kernel, kz_emit_sorted).  The reference's SklearnNN takes any k <= n (sklearn_nearest_neighbors.py:51-65, 96-101);
include/kiez_amd.h promises up to 4096.  Against the oracle (scikit-learn's brute force restated: float64 values, (value, smaller
index) order, also at k = n):

  * the LDS edge of the selection kernel: its static LDS plus 12 bytes per neighbour pass 64 KiB between 3748 and 3749 neighbours
    (kz_exact_select_lds opts in from there on) -- both sides of the edge, with and without the query's own row removed;
  * k = n (a full permutation of the index), also with NaN ranks (correlation: constant rows last, by row);
  * the two-level selection (more than four chunks of 4096 index rows) through both first-level kernels, a last chunk of ONE row,
    and thousands of rows tied at the k-th place;
  * wide rows on both sides of the row-count gates of the distance kernels, a boolean metric, the refusals beyond 4096;
  * the callers: kz_knn_dual (searches twice beyond 110), Kiez with and without hubness reduction.

ROUTE.  kz_knn_stats has no field that names the exact-only route.  What the code (kz_knn_impl: exact_only) leaves behind and no
fused pass does: every row counted as uncertified by the first pass AND as answered by the exact kernels, nothing escalated to
another tier, no speculative or range re-search, no wide lists, first_pass 0 (no fp16 / split-bf16 pass) and max_err_ratio exactly
0.0 -- the finalize kernel, which measures that ratio on every candidate it re-ranks, never ran.  _assert_exact_only asserts all
of them.  One case cannot: 541 neighbours on an index of 161 tiles is still the long-k route's (it takes k + self <= 551 where the
index has >= 4 tiles per range; the 4200-row index of the other cases has 33 tiles and none); there eps_scale = 1e30 lets the fused
pass certify nothing, the exact kernels answer every row (n_fallback_rows), and the route assertion is left out.

`pytest -m gpu`; -s shows the wall time of every case."""
import functools
import time
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = {"cosine": 1e-6}      # (the bounds of test_gpu_longk.py: euclidean family 1e-12 / 1e-12, cosine 1e-6 / 1e-7)
ATOL = {"cosine": 1e-7}


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    c.set_option("exact_rows", 3)
    c.set_option("eps_scale", 1.0)
    c.set_option("precision", 0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _assert_exact_only(st, n_q):
    """The call ran on the exact float64 kernels alone (module docstring: ROUTE)."""
    assert st["n_fallback_rows"] == n_q and st["n_first_pass_fail"] == n_q, st
    assert st["n_escalated_rows"] == 0 and st["n_spec_rows"] == 0 and st["n_range_rows"] == 0 and st["wide_lists"] == 0, st
    assert st["first_pass"] == 0 and st["max_err_ratio"] == 0.0 and st["dual"] == 0, st


def _knn(ctx, case, qm, im, k, **kw):
    """kz_knn -> (dist, ind, stats) on the host; prints the case's wall time."""
    from kiez_amd import _native as N
    t0 = time.perf_counter()
    dd, ii, st = N.knn(ctx, qm, im, k, **kw)
    dd, ii = dd.numpy(), ii.numpy()
    print(f"large-k {case}: {time.perf_counter() - t0:.3f} s")
    return dd, ii, st


def _assert_close(dd, od, metric):
    np.testing.assert_allclose(dd, od, rtol=RTOL.get(metric, 1e-12), atol=ATOL.get(metric, 1e-12))


def _oracle(q, y, k, metric):
    from oracle import kiez_oracle as O
    if metric == "cosine":      # (float64 rows, as every cosine comparison of this suite)
        q, y = q.astype(np.float64), y.astype(np.float64)
    return O.knn_exact(q, y, k, metric)


# ---- A, B: the LDS edge of kz_exact_select_kernel (single-level selection: two chunks) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_data():
    rng = np.random.default_rng(4200)
    y32 = rng.standard_normal((4200, 12)).astype(np.float32)
    q32 = rng.standard_normal((48, 12)).astype(np.float32)
    y64 = rng.standard_normal((4200, 12))
    return _frozen(q32, y32, y64)


@pytest.mark.parametrize("k", [541, 2048, 3748, 3749, 4096])
def test_a_lds_edge_of_the_selection_kernel(ctx, k):
    """Static + dynamic LDS of the selection kernel: 65 536 bytes at 3748 neighbours, past it at 3749."""
    from kiez_amd import _native as N
    q, y, _ = _edge_data()
    dd, ii, st = _knn(ctx, f"A k={k}", N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean"), k)
    _assert_exact_only(st, 48)
    od, oi = _oracle(q, y, k, "euclidean")
    np.testing.assert_array_equal(ii, oi)
    _assert_close(dd, od, "euclidean")


@pytest.mark.parametrize("k", [3747, 3748, 4095])
def test_b_lds_edge_with_the_own_row_removed(ctx, k):
    """The same edge one neighbour earlier: k + 1 = 3748, 3749, 4096 are selected and the query's own row is taken out."""
    from kiez_amd import _native as N
    _, _, y = _edge_data()
    m = N.DeviceMatrix(ctx, y, "sqeuclidean")
    dd, ii, st = _knn(ctx, f"B k={k}", m, m, k, exclude_self=True, q_begin=4100, q_count=64)
    _assert_exact_only(st, 64)
    own = np.arange(4100, 4164)[:, None]
    assert not (ii == own).any()
    fd, fi = _oracle(y[4100:4164], y, k + 1, "sqeuclidean")      # (k + 1 with the own row, which is among them at distance 0 ...)
    keep = fi != own
    assert (keep.sum(axis=1) == k).all()
    np.testing.assert_array_equal(ii, fi[keep].reshape(64, k))      # (... taken out: scikit-learn's self removal, _base.py:937-965)
    _assert_close(dd, fd[keep].reshape(64, k), "sqeuclidean")


# ---- C, D: k = n -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dtype", [("sqeuclidean", np.float64), ("cosine", np.float32)])
def test_c_every_index_row_is_a_neighbour(ctx, metric, dtype):
    from kiez_amd import _native as N
    rng = np.random.default_rng(3000)
    y = rng.standard_normal((3000, 10)).astype(dtype)
    q = rng.standard_normal((32, 10)).astype(dtype)
    dd, ii, st = _knn(ctx, f"C {metric}", N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric), 3000)
    _assert_exact_only(st, 32)
    np.testing.assert_array_equal(np.sort(ii, axis=1), np.broadcast_to(np.arange(3000), (32, 3000)))      # a full permutation ...
    od, oi = _oracle(q, y, 3000, metric)
    np.testing.assert_array_equal(ii, oi)                                                                  # ... in the oracle's order
    _assert_close(dd, od, metric)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_d_every_index_row_with_nan_ranks(ctx, dtype):
    """correlation against constant index rows is NaN: they come after every finite value, by row (the reference for this metric is
    scikit-learn's own search, as in test_gpu_metrics_extra.py: distances bit for bit, indices equal outside runs of equal values)."""
    from kiez_amd import _native as N
    from tests import metric_restate as MR
    from tests.test_gpu_metrics_extra import _check, _sklearn
    rng = np.random.default_rng(31)
    y = rng.standard_normal((3000, 10)).astype(dtype)
    q = rng.standard_normal((32, 10)).astype(dtype)
    const = np.array([4, 700, 1999, 2000, 2999])
    y[const] = np.array([0.5, -2.0, 0.0, 3.0, 0.125], dtype=dtype)[:, None]
    dd, ii, st = _knn(ctx, f"D {np.dtype(dtype).name}", N.DeviceMatrix(ctx, q, "correlation"), N.DeviceMatrix(ctx, y, "correlation"), 3000)
    _assert_exact_only(st, 32)
    assert np.isnan(dd[:, -5:]).all() and np.isfinite(dd[:, :-5]).all()
    np.testing.assert_array_equal(ii[:, -5:], np.broadcast_to(const, (32, 5)))
    sd, si = _sklearn("correlation", y, q, 3000, None)
    _check("correlation", dd, ii, sd, si, q, y, None)
    rd, ri = MR.knn("correlation", q, y, 3000)      # (the restated (value, row) order, NaN last by row: every place)
    np.testing.assert_array_equal(ii, ri)
    np.testing.assert_array_equal(dd, rd)


# ---- E, F: two-level selection (six chunks, the last one holds ONE row) --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _six_chunk_data():
    rng = np.random.default_rng(20481)
    return _frozen(rng.standard_normal((40, 16)).astype(np.float32), rng.standard_normal((20_481, 16)).astype(np.float32))


@pytest.mark.parametrize("k", [541, 1000, 4096])
def test_e_two_level_selection_through_both_first_level_kernels(ctx, k):
    """exact_rows 0: kz_exact_chunk_kernel (k rounds of arg-min per chunk); 2 and 3: kz_exact_chunk_radix_kernel.  The last chunk
    holds one row: fewer entries than places, padded with (+inf, INT_MAX)."""
    from kiez_amd import _native as N
    q, y = _six_chunk_data()
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    fused = k <= 551      # (module docstring, ROUTE: the long-k route would take it -- its pass certifies nothing here)
    if fused:
        ctx.set_option("eps_scale", 1e30)
    out = {}
    for rows in (0, 2, 3):
        ctx.set_option("exact_rows", rows)
        dd, ii, st = _knn(ctx, f"E k={k} exact_rows={rows}", qm, ym, k)
        if fused:
            assert st["n_fallback_rows"] == 40, st
        else:
            _assert_exact_only(st, 40)
        out[rows] = (dd, ii)
    for rows in (2, 3):
        np.testing.assert_array_equal(out[0][1], out[rows][1], err_msg=f"exact_rows {rows}")
        np.testing.assert_array_equal(out[0][0], out[rows][0], err_msg=f"exact_rows {rows}")
    od, oi = _oracle(q, y, k, "euclidean")
    np.testing.assert_array_equal(out[3][1], oi)
    _assert_close(out[3][0], od, "euclidean")


@functools.lru_cache(maxsize=None)
def _tie_data():
    rng = np.random.default_rng(3)
    return _frozen(rng.integers(0, 3, (40, 8)).astype(np.float32), rng.integers(0, 3, (20_481, 8)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _tie_oracle(metric, k):
    q, y = _tie_data()
    return _frozen(*_oracle(q, y, k, metric))


@pytest.mark.parametrize("rows", [0, 3])
@pytest.mark.parametrize("metric,k", [("sqeuclidean", 1000), ("sqeuclidean", 4096), ("manhattan", 1000), ("chebyshev", 4096)])
def test_f_true_ties_at_the_kth_place(ctx, metric, k, rows):
    """Small-integer rows: every value is exact, hundreds to thousands of index rows at the same distance (chebyshev: three distinct
    values in all) -- of the rows tied at the k-th place those with the smallest index, from every chunk and from their union."""
    from kiez_amd import _native as N
    q, y = _tie_data()
    ctx.set_option("exact_rows", rows)
    dd, ii, st = _knn(ctx, f"F {metric} k={k} exact_rows={rows}", N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric), k)
    _assert_exact_only(st, 40)
    od, oi = _tie_oracle(metric, k)
    np.testing.assert_array_equal(ii, oi)
    np.testing.assert_array_equal(dd, od)


# ---- G, H: wide rows, a boolean metric ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide_data():
    rng = np.random.default_rng(200)
    return _frozen(rng.standard_normal((64, 200)).astype(np.float32), rng.standard_normal((20_481, 200)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _wide_oracle(metric):
    q, y = _wide_data()
    return _frozen(*_oracle(q, y, 1000, metric))


@pytest.mark.parametrize("n_q", [64, 33])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_g_wide_rows_on_both_sides_of_the_batch_gates(ctx, metric, n_q):
    """d = 200.  64 rows: the one-pair-per-lane kernel and (cosine) the normalised float64 image of the index; 33 rows: the lane
    kernel (from 32 rows on) on the raw rows of a cosine index (the image is built from 64 rows on)."""
    from kiez_amd import _native as N
    q, y = _wide_data()
    q = q[:n_q]
    dd, ii, st = _knn(ctx, f"G {metric} rows={n_q}", N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric), 1000)      # (fresh matrices: no image of an earlier case)
    _assert_exact_only(st, n_q)
    od, oi = _wide_oracle(metric)
    np.testing.assert_array_equal(ii, oi[:n_q])
    _assert_close(dd, od[:n_q], metric)


def test_h_boolean_metric(ctx):
    """jaccard on 129 bits (past the image's word and row-padding edges), 2048 neighbours: scikit-learn's search and the restated
    (value, row) order, as test_gpu_boolean_metrics.py."""
    from kiez_amd import _native as N
    from tests import boolean_restate as BR
    from tests.test_gpu_boolean_metrics import _check, _data, _sklearn
    rng = np.random.default_rng(129)
    q, y = _data(rng, 48, 129, np.float32), _data(rng, 4200, 129, np.float32)
    dd, ii, st = _knn(ctx, "H jaccard", N.DeviceMatrix(ctx, q, "jaccard"), N.DeviceMatrix(ctx, y, "jaccard"), 2048)
    _assert_exact_only(st, 48)
    sd, si = _sklearn("jaccard", y, q, 2048)
    _check("jaccard", dd, ii, sd, si, q, y)
    rd, ri = BR.knn("jaccard", q, y, 2048)
    np.testing.assert_array_equal(ii, ri)
    np.testing.assert_array_equal(dd, rd)


# ---- I: refusals -------------------------------------------------------------------------------------------------------------------
def test_i_refusals_beyond_4096(ctx):
    from kiez_amd import Kiez
    from kiez_amd import _native as N
    _, y, _ = _edge_data()
    m = N.DeviceMatrix(ctx, y, "euclidean")
    assert N.MAX_NEIGHBORS == 4096
    for k, own in ((4097, False), (4096, True)):
        with pytest.raises(NotImplementedError, match="maximum of 4096"):      # (KZ_ERR_UNSUPPORTED; kz_last_error names the maximum)
            N.knn(ctx, m, m, k, exclude_self=own, q_begin=0, q_count=8)
        assert "4096" in ctx.lib.kz_last_error().decode()
    with pytest.raises(NotImplementedError):
        Kiez(n_candidates=4096, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=None)
    Kiez(n_candidates=4095, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=None)


# ---- J, K, L: through the callers --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_sources():
    rng = np.random.RandomState(600)
    return _frozen(rng.rand(2500, 12).astype(np.float32), rng.rand(2300, 12).astype(np.float32))


def test_j_dual_search_at_600_neighbours(ctx):
    """kz_knn_dual beyond 110 neighbours searches twice (include/kiez_amd.h): the bits of two kz_knn calls."""
    from kiez_amd import _native as N
    a, b = _two_sources()
    am, bm = N.DeviceMatrix(ctx, a, "euclidean"), N.DeviceMatrix(ctx, b, "euclidean")
    t0 = time.perf_counter()
    (d_ab, i_ab, s_ab), (d_ba, i_ba, s_ba) = N.knn_dual(ctx, am, bm, 600)
    got = [x.numpy() for x in (d_ab, i_ab, d_ba, i_ba)]
    print(f"large-k J dual: {time.perf_counter() - t0:.3f} s")
    assert s_ab["dual"] == 0 and s_ba["dual"] == 0, (s_ab, s_ba)
    _assert_exact_only(s_ab, 2500)
    _assert_exact_only(s_ba, 2300)
    d1, i1, _ = _knn(ctx, "J a->b", am, bm, 600)
    d2, i2, _ = _knn(ctx, "J b->a", bm, am, 600)
    for g, w in zip(got, (d1, i1, d2, i2)):
        np.testing.assert_array_equal(g, w)
    od, oi = _oracle(a, b, 600, "euclidean")
    np.testing.assert_array_equal(i1, oi)
    _assert_close(d1, od, "euclidean")


def test_k_api_single_source_at_4095_candidates(ctx):
    """The largest n_candidates the backend takes, one source: 4095 neighbours with the row itself removed -- 4096 selected."""
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    rng = np.random.RandomState(4095)
    s = rng.rand(4200, 8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kz = Kiez(n_candidates=4095, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=None).fit(s)
        t0 = time.perf_counter()
        d, i = kz.kneighbors(4095)
        print(f"large-k K api: {time.perf_counter() - t0:.3f} s")
    _assert_exact_only(kz.algorithm.last_stats, 4200)
    assert d.shape == (4200, 4095) and not (i == np.arange(4200)[:, None]).any()
    od, oi = O.kiez_pipeline(s, None, 4095, 4095, "euclidean", 2, None, {})
    np.testing.assert_array_equal(i, oi)
    _assert_close(d, od, "euclidean")


def test_l_api_with_hubness_at_600_candidates(ctx):
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    s, t = _two_sources()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kz = Kiez(n_candidates=600, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS").fit(s, t)
        t0 = time.perf_counter()
        d, i = kz.kneighbors(500)
        print(f"large-k L api: {time.perf_counter() - t0:.3f} s")
    od, oi = O.kiez_pipeline(s, t, 600, 500, "euclidean", 2, "CSLS", {})
    np.testing.assert_array_equal(i, oi)
    np.testing.assert_allclose(d, od, rtol=1e-9, atol=1e-12)
