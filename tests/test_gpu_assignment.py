"""The minimum-cost assignment on the device (kz_assign_lists, matching.assignment, Kiez.assign): match, col, prices and rounds are
compared for exact equality with the numpy restatement of the auction (tests/assignment_restate.py) -- shapes that run wide rounds
first and the single-workgroup kernel after, tail only, one column, lists longer than 64 columns, one target, more rows than one
grid, no rows; float64 and float32 values; sorted and shuffled rows, heavy ties, negative values, padding in the middle of rows,
repeated targets, a threshold below some values -- the phases against each other, two runs, the optimum of scipy and the price
certificate on the device's own output, the round cap, and the facade under every device-native reduction.  `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

from tests import assignment_restate as AR
from tests.test_assignment import lists_of
from tests.test_gpu_match import _kiez, embeddings, shuffled  # noqa: F401  (embeddings: the module's fixture)
from tests.test_match import random_lists

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def run(ctx, dist, ind, n_index, u, eps, tail_rows=0, max_rounds=1_000_000):
    """kz_assign_lists on host lists -> (match, col, prices, rounds, converged), the arrays on the host."""
    from kiez_amd import _native as N
    match, col, prices, rounds, converged = N.assign_lists(ctx, ctx.to_device(dist), ctx.to_device(ind), n_index, u, eps, max_rounds,
                                                           tail_rows=tail_rows, want_prices=True)
    return match.numpy(), col.numpy(), prices.numpy(), rounds, converged


def assert_same(got, want, what=""):
    for name, a, b in zip(("match", "col"), got[:2], want[:2]):
        assert a.dtype == np.int64
        np.testing.assert_array_equal(a, b, err_msg=f"{name} {what}")
    assert got[2].dtype == np.float64
    np.testing.assert_array_equal(got[2].view(np.uint64), want[2].view(np.uint64), err_msg=f"prices, bit for bit {what}")
    assert got[3] == want[3], f"rounds {what}"
    assert bool(got[4]) == bool(want[4]), f"converged {what}"


def check(ctx, dist, ind, n_index, u=None, eps=None, what="", **kw):
    """Device == restatement, bit for bit -> the device's result, u, eps."""
    u, eps = AR.defaults(dist, ind, n_index, u, eps)
    got = run(ctx, dist, ind, n_index, u, eps, **kw)
    assert_same(got, AR.auction(dist, ind, n_index, u, eps), what)
    return got, u, eps


def at(dist, ind, n_index, frac):
    """The value `frac` of the way through the range of the listed values."""
    lo, hi = AR.value_range(dist, ind, n_index)
    return lo + frac * (hi - lo)


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_shapes(ctx, dtype, shuffle):
    rng = np.random.default_rng(17)
    prep = (lambda d, i: shuffled(rng, d, i)) if shuffle else (lambda d, i: (d, i))

    # the first rounds have more than 1 024 bidders, the rest run in the tail (u at 0.7 of the range: ~8 000 rounds, not 140 000)
    dist, ind = prep(*random_lists(rng, 3000, 3000, 10, dtype=dtype))
    got, _, _ = check(ctx, dist, ind, 3000, u=at(dist, ind, 3000, 0.7), what="3000 x 3000 x 10")
    assert got[3] > 1000 and np.count_nonzero(got[0] >= 0) > 2900

    for n_q, n_index, k in ((300, 300, 5), (500, 400, 10), (400, 600, 3), (200, 150, 1), (300, 200, 130)):
        dist, ind = prep(*random_lists(rng, n_q, n_index, k, dtype=dtype))
        got, _, _ = check(ctx, dist, ind, n_index, what=f"{n_q} x {n_index} x {k}")
        assert got[4] and got[3] > 1

    # one target: every row bids for it, the smallest value takes it (listed three times per row: the best entry of a row counts)
    dist, ind = random_lists(rng, 300, 1, 3, dtype=dtype)
    dist, ind = prep(dist, np.zeros_like(ind))
    got, _, _ = check(ctx, dist, ind, 1, what="n_target = 1")
    assert np.count_nonzero(got[0] == 0) == 1 and got[0][np.argmin(dist.min(axis=1))] == 0

    # more rows than one grid covers: the grid-stride loop of every wide kernel, then 50 targets' worth of tail
    ind = rng.integers(0, 50, (70_000, 2), dtype=np.int64)
    dist = np.sort(rng.standard_normal((70_000, 2)), axis=1).astype(dtype)
    got, _, _ = check(ctx, *prep(dist, ind), 50, what="70 000 x 50 x 2")
    assert np.count_nonzero(got[0] >= 0) == 50

    got = run(ctx, np.zeros((0, 4), dtype=dtype), np.zeros((0, 4), dtype=np.int64), 5, 1.0, 0.1)
    assert got[0].shape == got[1].shape == (0,) and got[3] == 0 and got[4] and (got[2] == 0.0).all() and got[2].shape == (5,)


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_contents(ctx, dtype, shuffle):
    rng = np.random.default_rng(23)
    prep = (lambda d, i: shuffled(rng, d, i)) if shuffle else (lambda d, i: (d, i))
    n_q, n_index, k = 257, 130, 8
    inf, nan = np.inf, np.nan

    # integer values with heavy ties (equal bids: the smallest row), at the eps that makes the optimum exact
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype)
    dist = np.sort(rng.integers(0, 4, dist.shape), axis=1).astype(dtype)
    got, u, eps = check(ctx, *prep(dist, ind), n_index, eps=1.0 / (n_q + 1) * (1 - 2.0 ** -20), what="integer ties")
    assert AR.cost(dist, ind, n_index, u, *AR.auction(dist, ind, n_index, u, eps)[:2]) == AR.optimum(dist, ind, n_index, u)
    check(ctx, *prep(np.ones_like(dist), ind), n_index, what="all equal")

    # all-negative values (CSLS)
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype)
    check(ctx, *prep(np.sort(-np.abs(dist) - 0.5, axis=1), ind), n_index, what="negative")

    # padding (-1, INT_MAX, n_index, NaN, +-inf) at the row ends, in the middle, and rows of padding only
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype, pad=0.25)
    ind[:, -1] = 0x7fffffff
    ind[::2, 3] = -1
    dist[1::3, 2] = nan
    dist[2::5, 4] = inf
    dist[3::7, 0] = -inf
    ind[5] = -1
    ind[6] = n_index
    ind[7] = [n_index, -1, 0x7fffffff, -5, n_index + 1, 1 << 40, -(1 << 40), np.iinfo(np.int64).min]
    dist[8] = [nan, inf, -inf, nan, inf, -inf, nan, nan]
    got, _, _ = check(ctx, *prep(dist, ind), n_index, what="padding")
    assert (got[0][5:9] == -1).all() and (got[1][5:9] == -1).all()

    # a target listed twice in one row (k > n_index repeats ids; and one repeated on purpose in every row)
    dist, ind = random_lists(rng, n_q, 5, k, dtype=dtype)
    ind[:, 5] = ind[:, 1]
    check(ctx, *prep(dist, ind), 5, what="repeated targets")

    # u below some values (a threshold), below all of them, and far above
    dist, ind = prep(*random_lists(rng, n_q, n_index, k, dtype=dtype))
    got, u, _ = check(ctx, dist, ind, n_index, u=at(dist, ind, n_index, 0.4), what="u inside the range")
    assert (dist[got[0] >= 0, got[1][got[0] >= 0]] <= u).all() and (got[0] < 0).any()
    got, _, _ = check(ctx, dist, ind, n_index, u=at(dist, ind, n_index, -0.1), what="u below every value")
    assert (got[0] == -1).all() and got[3] == 1
    check(ctx, dist, ind, n_index, u=at(dist, ind, n_index, 1.5), what="u above every value")


@pytest.fixture(scope="module")
def phase_lists():
    """1 500 x 1 200 x 10 (more than 1 024 bidders in the first rounds) and 300 x 300 x 5 (about 1 900 rounds), with the restatement."""
    rng = np.random.default_rng(31)
    out = []
    for n_q, n_index, k in ((1500, 1200, 10), (300, 300, 5)):
        dist, ind = random_lists(rng, n_q, n_index, k)
        u, eps = AR.defaults(dist, ind, n_index)
        out.append((dist, ind, n_index, u, eps, AR.auction(dist, ind, n_index, u, eps)))
    return out


@pytest.mark.parametrize("tail_rows", [0, -1, 1, 64, 1024])
def test_phases_agree(ctx, phase_lists, tail_rows):
    for dist, ind, n_index, u, eps, want in phase_lists:
        assert_same(run(ctx, dist, ind, n_index, u, eps, tail_rows=tail_rows), want, f"tail_rows = {tail_rows}, {dist.shape}")


def test_two_runs_agree(ctx, phase_lists):
    dist, ind, n_index, u, eps, _ = phase_lists[0]
    assert_same(run(ctx, dist, ind, n_index, u, eps), run(ctx, dist, ind, n_index, u, eps), "second run")


@pytest.mark.parametrize("half", [False, True], ids=["u_default", "u_half_range"])
@pytest.mark.parametrize("kind", ["uniform", "hubs", "integer", "negative"])
def test_device_output_is_optimal(ctx, kind, half):
    """cost <= optimum + n_q * eps (scipy on the dense matrix) on what the device returned, at the <= 600-row shapes."""
    for n_q, n_index, k in ((300, 300, 5), (500, 400, 10), (400, 600, 3), (64, 64, 64)):
        dist, ind, eps = lists_of(kind, n_q, n_index, k)
        u, eps = AR.defaults(dist, ind, n_index, u=at(dist, ind, n_index, 0.5) if half else None, eps=eps)
        match, col, prices, rounds, converged = run(ctx, dist, ind, n_index, u, eps)
        assert converged
        got, want = AR.cost(dist, ind, n_index, u, match, col), AR.optimum(dist, ind, n_index, u)
        print(f"{kind} {n_q} x {n_index} x {k}: rounds {rounds}, cost - optimum = {got - want:.3g} (bound {n_q * eps:.3g})")
        if kind == "integer":
            assert got == want
        assert got - want <= n_q * eps
        assert AR.slack_violation(dist, ind, n_index, u, eps, match, col, prices) == 0


def test_price_certificate_at_3000(ctx):
    """Where scipy's dense solver is too slow: eps-complementary slackness of the returned matching and prices, u the default."""
    rng = np.random.default_rng(41)
    dist, ind = random_lists(rng, 3000, 3000, 10)
    u, eps = AR.defaults(dist, ind, 3000)
    match, col, prices, rounds, converged = run(ctx, dist, ind, 3000, u, eps)
    print(f"3000 x 3000 x 10, u the default: {rounds} rounds, {np.count_nonzero(match >= 0)} matched")
    assert converged
    AR.cost(dist, ind, 3000, u, match, col)          # (a matching over pairs)
    assert AR.slack_violation(dist, ind, 3000, u, eps, match, col, prices) == 0
    broken = prices.copy()
    broken[match[0]] += 4.0 * (u - dist.min())       # (the certificate does notice a wrong price)
    assert AR.slack_violation(dist, ind, 3000, u, eps, match, col, broken) > 0


def test_round_cap_and_limits(ctx):
    from kiez_amd import _native as N
    from kiez_amd import matching
    rng = np.random.default_rng(43)
    dist, ind = random_lists(rng, 300, 300, 5)
    u, eps = AR.defaults(dist, ind, 300)
    for tail_rows in (0, -1):
        for cap in (1, 2, 9, 50):
            got = run(ctx, dist, ind, 300, u, eps, tail_rows=tail_rows, max_rounds=cap)
            assert got[3] == cap and not got[4]
            assert_same(got, AR.auction(dist, ind, 300, u, eps, max_rounds=cap), f"cap {cap}, tail_rows {tail_rows}")
            AR.cost(dist, ind, 300, u, got[0], got[1])       # a valid matching: rows still FREE come out as -1
    with pytest.raises(RuntimeError, match=r"1 rounds.*eps.*unmatched_cost.*larger eps or a smaller unmatched_cost"):
        matching.assignment(dist, ind, 300, max_rounds=1)
    # limits as kz_match_lists; the options
    d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
    with pytest.raises(ValueError, match="4096"):
        run(ctx, np.zeros((3, 4097)), np.zeros((3, 4097), dtype=np.int64), 5, 1.0, 0.1)
    for n_index in (0, 1 << 31):
        with pytest.raises(ValueError, match="n_index"):
            N.assign_lists(ctx, d_dev, i_dev, n_index, u, eps, 10)
    for bad_u in (np.inf, np.nan):
        with pytest.raises(ValueError, match="unmatched_cost"):
            N.assign_lists(ctx, d_dev, i_dev, 300, bad_u, eps, 10)
    for bad_eps in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="eps"):
            N.assign_lists(ctx, d_dev, i_dev, 300, u, bad_eps, 10)
    with pytest.raises(ValueError, match="tail_rows"):
        N.assign_lists(ctx, d_dev, i_dev, 300, u, eps, 10, tail_rows=1025)
    with pytest.raises(ValueError, match="max_rounds"):
        N.assign_lists(ctx, d_dev, i_dev, 300, u, eps, -1)
    # prices, rounds and converged may be null
    match, col = ctx.empty((300,), np.int64), ctx.empty((300,), np.int64)
    N._check(ctx.lib.kz_assign_lists(ctx.handle, d_dev.ptr, N.KZ_F64, i_dev.ptr, 300, 5, 300, u, eps, 1_000_000, 0, match.ptr, col.ptr, None,
                                     ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_int)()), "kz_assign_lists")
    want = AR.auction(dist, ind, 300, u, eps)
    np.testing.assert_array_equal(match.numpy(), want[0])
    np.testing.assert_array_equal(col.numpy(), want[1])


def test_assignment(ctx):
    """matching.assignment: the defaults computed on the host (numpy lists) and on the device (DeviceArrays) are the same numbers."""
    from kiez_amd import _native as N
    from kiez_amd import matching
    rng = np.random.default_rng(47)
    for dtype in DTYPES:
        dist, ind = random_lists(rng, 300, 120, 9, dtype=dtype, pad=0.1)
        dist[4, 2] = np.nan
        dist[9, 0] = np.inf           # (not a listed value: the default u is the largest FINITE one)
        u, eps = AR.defaults(dist, ind, 120)
        assert N.assign_range(ctx, ctx.to_device(dist), ctx.to_device(ind), 120) == AR.value_range(dist, ind, 120)
        want = AR.auction(dist, ind, 120, u, eps)
        want_dist = np.where(want[1] >= 0, dist[np.arange(300), np.maximum(want[1], 0)], np.nan).astype(dtype)
        md, mi, prices = matching.assignment(dist, ind, 120, return_prices=True)
        assert md.dtype == dtype and mi.dtype == np.int64 and prices.dtype == np.float64
        np.testing.assert_array_equal(mi, want[0])
        np.testing.assert_array_equal(md.view(np.uint8), want_dist.view(np.uint8))      # bit for bit, NaN where unmatched
        np.testing.assert_array_equal(prices, want[2])
        assert (want[0] < 0).any() and np.isnan(md[want[0] < 0]).all()
        np.testing.assert_array_equal(matching.assignment(dist, ind.astype(np.int32), 120, return_distance=False), want[0])
        md_dev, mi_dev = matching.assignment(ctx.to_device(dist), ctx.to_device(ind), 120)
        assert isinstance(md_dev, N.DeviceArray) and isinstance(mi_dev, N.DeviceArray)
        np.testing.assert_array_equal(mi_dev.numpy(), want[0])
        np.testing.assert_array_equal(md_dev.numpy().view(np.uint8), want_dist.view(np.uint8))
        # explicit options
        u2, eps2 = AR.defaults(dist, ind, 120, u=at(dist, ind, 120, 0.5), eps=1e-3)
        np.testing.assert_array_equal(matching.assignment(dist, ind, 120, unmatched_cost=u2, eps=eps2, return_distance=False),
                                      AR.auction(dist, ind, 120, u2, eps2)[0])
        with pytest.raises(ValueError, match="2\\*\\*-40"):
            matching.assignment(ctx.to_device(dist), ctx.to_device(ind), 120, eps=1e-14)
    # lists without a pair: every row unmatched
    mi = matching.assignment(np.full((4, 2), np.nan), np.zeros((4, 2), dtype=np.int64), 3, return_distance=False)
    assert mi.tolist() == [-1] * 4
    assert N.assign_range(ctx, ctx.to_device(np.full((4, 2), np.nan)), ctx.to_device(np.zeros((4, 2), dtype=np.int64)), 3) is None


def stable_cost(dist, ind, n_target, u, k_inst, **kw):
    md, mi = k_inst.match(10, **kw)
    col = np.full(len(mi), -1, dtype=np.int64)
    for i in np.nonzero(mi >= 0)[0]:
        col[i] = np.nonzero((ind[i] == mi[i]) & (dist[i] == md[i]))[0][0]
    return AR.cost(dist, ind, n_target, u, mi, col)


@pytest.mark.parametrize("hubness,whole,metric,dtype", [("none", False, "euclidean", np.float64), ("csls", False, "euclidean", np.float64),
                                                        ("csls", True, "cosine", np.float32), ("nicdm", False, "cosine", np.float32),
                                                        ("mp_normal", False, "euclidean", np.float64)])
def test_facade(embeddings, hubness, whole, metric, dtype):  # noqa: F811
    from kiez_amd import _native as N
    from kiez_amd import matching
    source, target = (x.astype(dtype) for x in embeddings)
    k_inst = _kiez(hubness, metric).fit(source, target)
    stable_before = k_inst.match(10, whole_index=whole)
    dist, ind = k_inst.kneighbors_whole_index(10) if whole else k_inst.kneighbors(10)
    u, eps = AR.defaults(dist, ind, 400)
    want = AR.auction(dist, ind, 400, u, eps)
    md, mi = k_inst.assign(10, whole_index=whole)
    where = f"{hubness} {metric} whole_index={whole}"
    np.testing.assert_array_equal(mi, want[0], err_msg=where)
    assert md.dtype == dist.dtype and mi.dtype == np.int64
    want_dist = np.where(want[1] >= 0, dist[np.arange(500), np.maximum(want[1], 0)], np.nan).astype(dist.dtype)
    np.testing.assert_array_equal(md.view(np.uint8), want_dist.view(np.uint8), err_msg=where)
    taken = mi[mi >= 0]
    assert len(np.unique(taken)) == len(taken) and (mi < 0).any()                      # no target twice; 500 sources, 400 targets
    np.testing.assert_array_equal(k_inst.assign(10, whole_index=whole, return_distance=False), mi)
    md_dev, mi_dev = k_inst.assign_device(10, whole_index=whole)
    assert isinstance(md_dev, N.DeviceArray) and isinstance(mi_dev, N.DeviceArray)
    np.testing.assert_array_equal(mi_dev.numpy(), mi)
    # equals matching.assignment on the host copies of the same lists
    np.testing.assert_array_equal(matching.assignment(dist, ind, 400, return_distance=False), mi)
    # never dearer than the stable matching under the same u (every stable pair is a pair: u is the largest listed value)
    c_opt, c_stable = AR.cost(dist, ind, 400, u, want[0], want[1]), stable_cost(dist, ind, 400, u, k_inst, whole_index=whole)
    print(f"{where}: optimal {c_opt:.6f}, stable {c_stable:.6f}, rounds {want[3]}")
    assert c_opt <= c_stable + 500 * eps
    # a threshold through the facade
    u_half = at(dist, ind, 400, 0.5)
    np.testing.assert_array_equal(k_inst.assign(10, whole_index=whole, return_distance=False, unmatched_cost=u_half, eps=eps),
                                  AR.auction(dist, ind, 400, u_half, eps)[0])
    # the stable matching is what it was
    stable_after = k_inst.match(10, whole_index=whole)
    np.testing.assert_array_equal(stable_after[1], stable_before[1])
    np.testing.assert_array_equal(stable_after[0].view(np.uint8), stable_before[0].view(np.uint8))


def test_facade_on_a_precomputed_fit(embeddings):  # noqa: F811
    from kiez_amd import Kiez
    source, target = embeddings
    D = np.sqrt(((source[:, None, :] - target[None, :, :]) ** 2).sum(axis=2))
    k_inst = Kiez(n_candidates=10, algorithm_kwargs={"metric": "precomputed"}, hubness="CSLS").fit(D)
    dist, ind = k_inst.kneighbors(10)
    u, eps = AR.defaults(dist, ind, 400)
    md, mi = k_inst.assign(10)
    want = AR.auction(dist, ind, 400, u, eps)
    np.testing.assert_array_equal(mi, want[0])
    assert AR.cost(dist, ind, 400, u, want[0], want[1]) <= stable_cost(dist, ind, 400, u, k_inst) + 500 * eps
