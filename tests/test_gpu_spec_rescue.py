"""SPECULATIVE RESCUE (kz_knn.hip): the exact float64 kernels launched behind every finalize kernel for the handful of rows a pass
leaves uncertified, before the host knows the count.  Whatever the count turns out to be -- none, a handful (answered in place), more
than the speculation covers (the ordinary re-search runs) -- the result is the oracle's, bit for bit, and the same as with the
speculation switched off.  Reference path: kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101 (kneighbors of the brute-force
backend); both directions of a fit: kiez/hubness_reduction/base.py:33-50."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("spec_rows", 64), ("eps_scale", 1.0), ("dual_force", 0)):
        c.set_option(name, value)


def _gmm(rows, d, seed):
    """L2-normalised gaussian mixture (bench.py "ea15k" / "gmm": the kind of data that leaves a few rows uncertified)."""
    centres = np.random.RandomState(6).standard_normal((64, d)).astype(np.float32)
    rng = np.random.RandomState(seed)
    x = centres[rng.randint(0, 64, rows)] + np.float32(0.35) * rng.standard_normal((rows, d)).astype(np.float32)
    return (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(np.float32)


def _few_failures(ctx, qm, ym, k, lo=1, hi=16, exclude_self=False, must=False):
    """An `eps_scale` at which the first pass leaves between lo and hi rows uncertified (speculation off while looking).
    must: finding none fails the test instead of skipping it."""
    from kiez_amd import _native as N
    ctx.set_option("spec_rows", 0)
    scale, lo_s, hi_s = 1.0, None, None
    for _ in range(40):
        ctx.set_option("eps_scale", scale)
        _, _, st = N.knn(ctx, qm, ym, k, exclude_self=exclude_self)
        n = st["n_first_pass_fail"]
        if lo <= n <= hi:
            return scale, n
        if n < lo:
            lo_s = scale
            scale = scale * 2 if hi_s is None else 0.5 * (scale + hi_s)
        else:
            hi_s = scale
            scale = scale / 2 if lo_s is None else 0.5 * (scale + lo_s)
    if must:
        pytest.fail("no eps_scale leaves a handful of rows uncertified on this data")
    pytest.skip("no eps_scale leaves a handful of rows uncertified on this data")


@pytest.mark.parametrize("metric,d,k,dtype", [("euclidean", 300, 10, np.float32), ("cosine", 128, 10, np.float32),
                                              ("sqeuclidean", 64, 5, np.float64), ("euclidean", 200, 50, np.float32)])
def test_a_handful_of_uncertified_rows_is_answered_in_place(ctx, metric, d, k, dtype):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(6000, d, 1).astype(dtype), _gmm(9000, d, 2).astype(dtype)
    qm, ym = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
    scale, n_fail = _few_failures(ctx, qm, ym, k)
    d_off, i_off, st_off = N.knn(ctx, qm, ym, k)
    assert st_off["n_spec_rows"] == 0 and st_off["n_escalated_rows"] + st_off["n_fallback_rows"] >= n_fail
    ctx.set_option("spec_rows", 64)
    d_on, i_on, st_on = N.knn(ctx, qm, ym, k)
    assert st_on["n_first_pass_fail"] == n_fail
    assert st_on["n_spec_rows"] == n_fail and st_on["n_fallback_rows"] == n_fail and st_on["n_escalated_rows"] == 0, st_on
    np.testing.assert_array_equal(i_on.numpy(), i_off.numpy())
    np.testing.assert_array_equal(d_on.numpy(), d_off.numpy())
    q64, y64 = (q.astype(np.float64), y.astype(np.float64)) if metric == "cosine" else (q, y)
    od, oi = O.knn_exact(q64, y64, k, metric)
    np.testing.assert_array_equal(i_on.numpy(), oi)
    if metric == "cosine":
        np.testing.assert_allclose(d_on.numpy(), od, rtol=1e-5, atol=1e-7)
    else:
        np.testing.assert_allclose(d_on.numpy(), od, rtol=1e-12, atol=0)


def test_a_large_index_takes_the_one_pair_per_lane_launch(ctx):
    """70 001 index rows are at least 4 x 64 per CU of a 256-CU device: kz_spec_rescue then tries the one-pair-per-lane kernel
    (kz_exact_lanes.h), here with the row count read on the device -- the other tests of this file, on 7 .. 9 k rows, never reach it."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(3000, 32, 9), _gmm(70001, 32, 10)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    _few_failures(ctx, qm, ym, 10, must=True)
    ctx.set_option("spec_rows", 64)
    dist, ind, st = N.knn(ctx, qm, ym, 10)
    assert st["n_spec_rows"] == st["n_first_pass_fail"] > 0, st
    od, oi = O.knn_exact(q, y, 10, "euclidean")
    np.testing.assert_array_equal(ind.numpy(), oi)
    np.testing.assert_allclose(dist.numpy(), od, rtol=1e-12, atol=0)


def test_more_uncertified_rows_than_the_speculation_covers(ctx):
    """The speculative launches find count > R and do nothing; the ordinary re-search answers the rows."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(5000, 96, 3), _gmm(8000, 96, 4)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    scale, n_fail = _few_failures(ctx, qm, ym, 10, lo=80, hi=2000)
    ctx.set_option("spec_rows", 64)
    dist, ind, st = N.knn(ctx, qm, ym, 10)
    assert st["n_first_pass_fail"] == n_fail and st["n_spec_rows"] == 0 and st["n_escalated_rows"] >= n_fail
    od, oi = O.knn_exact(q, y, 10, "euclidean")
    np.testing.assert_array_equal(ind.numpy(), oi)
    np.testing.assert_array_equal(dist.numpy(), od)
    # ... and a speculation of 4 rows against a count of 5 .. 16
    scale, n_fail = _few_failures(ctx, qm, ym, 10, lo=5, hi=16)
    ctx.set_option("spec_rows", 4)
    dist, ind, st = N.knn(ctx, qm, ym, 10)
    assert st["n_spec_rows"] == 0 and st["n_escalated_rows"] >= n_fail
    np.testing.assert_array_equal(ind.numpy(), oi)


def test_self_query_rows_and_row_ranges(ctx):
    """exclude_self (single-source mode) and a query range that does not start at row 0: the rescued rows land where they belong."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    x = _gmm(7000, 200, 5)
    xm = N.DeviceMatrix(ctx, x, "euclidean")
    _few_failures(ctx, xm, xm, 10, exclude_self=True)
    ctx.set_option("spec_rows", 64)
    dist, ind, st = N.knn(ctx, xm, xm, 10, exclude_self=True)
    assert st["n_spec_rows"] == st["n_first_pass_fail"] > 0
    od, oi = O.knn_exact(x, x, 10, "euclidean", exclude_self=True)
    np.testing.assert_array_equal(ind.numpy(), oi)
    np.testing.assert_array_equal(dist.numpy(), od)
    dist, ind, st = N.knn(ctx, xm, xm, 10, q_begin=1000, q_count=5000)
    np.testing.assert_array_equal(ind.numpy(), O.knn_exact(x[1000:6000], x, 10, "euclidean")[1])


def test_through_the_api_with_and_without_the_shared_sweep(ctx):
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    s, t = _gmm(6000, 300, 7), _gmm(7000, 300, 8)
    od, oi = O.kiez_pipeline(s, t, 10, 10, "euclidean", 2, "CSLS", {})
    for force in (0, 1):
        ctx.set_option("dual_force", force)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
            dist, ind = kz.fit(s, t).kneighbors(10)
        assert kz.algorithm.last_stats["dual"] == force
        np.testing.assert_array_equal(ind, oi)
        np.testing.assert_allclose(dist, od, rtol=1e-5, atol=1e-6)
