"""gold_ranks(route="sweep") -- kz_gold_ranks_sweep: the fp16 count sweep plus the exact values of its band -- against two references
per case: a plain numpy float64 count and route="exact" on every row (the same bits: the project's anchor).

The numpy count is only a reference where the data lets it be one: no index row that is not an exact duplicate of the gold row may lie
within 1e-9 (relative) of the gold value.  That is a condition on the data, checked here on the CPU for every case; the seeds are
fixed so that it holds.  Exact duplicates are allowed and wanted: they tie in any arithmetic and go by row."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_case(n_q, n_i, d, seed, dups=0, scale=1.0, offset=0.0):
    """Queries, index and gold ids of one call: the first third of the queries has a correlated gold row (target = source + noise: rank
    near 0, the tile-reject path), the next third a random one (rank near n / 2: the count path), then one row without gold, and the last
    query shares the gold row of query 0.  `dups`: that many exact copies of gold row 0 spread over the index, before and behind it."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n_q, d))
    y = rng.standard_normal((n_i, d))
    third = n_q // 3
    gold = rng.integers(0, n_i, n_q)
    gold[:third] = rng.choice(np.arange(n_i // 4, n_i), third, replace=False)
    y[gold[:third]] = q[:third] + 0.05 * rng.standard_normal((third, d))
    gold[2 * third] = -1
    gold[-1] = gold[0]
    if dups:
        free = np.setdiff1d(np.arange(n_i), gold[:third])
        y[np.sort(rng.choice(free, dups, replace=False))] = y[gold[0]]
    q, y = ((a * 1e-3 + 1.0 if offset else a) * scale for a in (q, y))   # (offset: 10^3 spreads)
    return q, y, gold.astype(np.int64)


def numpy_ranks(q, y, gold, metric):
    q, y = q.astype(np.float64), y.astype(np.float64)
    if metric == "cosine":
        q, y = q / np.linalg.norm(q, axis=1, keepdims=True), y / np.linalg.norm(y, axis=1, keepdims=True)
        v = 1.0 - q @ y.T
    else:
        v = (q * q).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (q @ y.T)
    rank = np.full(len(gold), -1, np.int64)
    cols = np.arange(y.shape[0])
    for r in np.flatnonzero(gold >= 0):
        g = gold[r]
        dup = (y == y[g]).all(1)
        near = ~dup & (np.abs(v[r] - v[r, g]) <= 1e-9 * abs(v[r, g]))
        assert not near.any(), f"precondition: query {r} has an index row within 1e-9 of its gold value"
        rank[r] = np.count_nonzero(np.where(dup, cols < g, v[r] < v[r, g]))
    return rank


def both_routes(q, y, gold, metric, dtype):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    qm, im = N.DeviceMatrix(ctx, q.astype(dtype), metric), N.DeviceMatrix(ctx, y.astype(dtype), metric)
    gold_dev = ctx.to_device(np.where(gold < 0, np.iinfo(np.int64).min, gold))
    stats = {}
    sweep = N.gold_ranks(ctx, qm, im, gold_dev, route="sweep", stats=stats).numpy()
    return sweep, N.gold_ranks(ctx, qm, im, gold_dev).numpy(), stats


def check(n_q, n_i, d, metric, dtype=np.float32, seed=0, benign=True, **kw):
    q, y, gold = make_case(n_q, n_i, d, seed, **kw)
    q, y = q.astype(dtype), y.astype(dtype)
    sweep, exact, stats = both_routes(q, y, gold, metric, dtype)
    print(f"{n_q} x {n_i} x {d} {metric} {np.dtype(dtype).name} {kw}: {stats}")
    np.testing.assert_array_equal(sweep, exact)
    np.testing.assert_array_equal(sweep, numpy_ranks(q, y, gold, metric))
    takes_sweep = n_i >= 128 and dtype == np.float32 and d > 16   # (d <= 16 is ONE slice of 16 features: outside the builds of 2 .. 24)
    assert stats["route_taken"] == int(takes_sweep) and stats["n_rows"] == np.count_nonzero(gold >= 0)
    if takes_sweep and benign:   # (without this the fallback could hide a broken sweep)
        assert stats["n_fallback_rows"] == 0 and stats["n_sweep_rows"] == stats["n_rows"] and stats["max_err_ratio"] <= 1.0
    return stats


@pytest.mark.parametrize("n_i", [127, 128, 129, 4097])
def test_index_sizes_around_one_tile(n_i):
    check(256, n_i, 100, "euclidean")


def test_several_index_ranges_per_query_tile():
    from kiez_amd import _native as N
    n, qt, pc, ln = C.c_int(0), (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    for slots in (512, 768):   # (two or three workgroups on each of 256 CUs: the plan the sweep's launcher makes)
        assert N.load().kz_knn_plan(300, 20001, 1, slots, 0, 1, C.byref(n), qt, pc, ln) == 0 and min(pc[:n.value]) >= 2
    check(300, 20001, 32, "sqeuclidean")


@pytest.mark.parametrize("q_begin,q_count", [(37, 150), (299, 1)])
def test_row_ranges(q_begin, q_count):
    """A row range (two query tiles, the second partial; the last row alone): the bytes of route="exact" on the same range, the slice
    of the whole-range result, and the sweep's own route on every row of the range -- a fallback cannot hide a broken range."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y, gold = make_case(300, 4097, 32, 0)
    qm, im = N.DeviceMatrix(ctx, q.astype(np.float32), "euclidean"), N.DeviceMatrix(ctx, y.astype(np.float32), "euclidean")
    dev = lambda g: ctx.to_device(np.where(g < 0, np.iinfo(np.int64).min, g))   # noqa: E731
    rows = slice(q_begin, q_begin + q_count)
    assert (gold[rows] >= 0).all()
    whole = N.gold_ranks(ctx, qm, im, dev(gold), route="sweep").numpy()
    stats = {}
    got = N.gold_ranks(ctx, qm, im, dev(gold[rows]), q_begin, q_count, route="sweep", stats=stats).numpy()
    print(f"rows [{q_begin}, {q_begin + q_count}): {stats}")
    assert got.tobytes() == N.gold_ranks(ctx, qm, im, dev(gold[rows]), q_begin, q_count).numpy().tobytes()
    np.testing.assert_array_equal(got, whole[rows])
    assert stats["route_taken"] == 1 and stats["n_rows"] == q_count


@pytest.mark.parametrize("d,metric", [(8, "cosine"), (32, "euclidean"), (100, "sqeuclidean"), (208, "cosine"), (384, "euclidean")])
def test_widths_and_metrics(d, metric):
    check(256, 4097, d, metric, seed=d)


@pytest.mark.parametrize("dtype", [np.float64, np.float16])
def test_other_element_types_take_the_exact_route(dtype):
    check(256, 4097, 100, "euclidean", dtype=dtype)


def test_ties_by_row_and_the_per_row_cap():
    check(256, 4097, 100, "euclidean", dups=5, benign=False)
    stats = check(256, 8193, 100, "euclidean", dups=3000, benign=False)
    assert stats["n_fallback_rows"] >= 1   # (3 000 band entries of one row: beyond the per-row cap)


@pytest.mark.parametrize("kw", [{"scale": 2.0 ** -20}, {"offset": 1.0}])
def test_magnitudes(kw):
    # (the bound is made of magnitudes: far from unit scale rows may fall back, the ranks may not change)
    check(256, 4097, 100, "euclidean", benign=False, **kw)


def test_interface():
    from kiez_amd import Kiez
    q, y, gold = make_case(256, 4097, 100, 0)
    k = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"})
    k.fit(q.astype(np.float32), y.astype(np.float32))
    want = numpy_ranks(q.astype(np.float32), y.astype(np.float32), gold, "euclidean")
    np.testing.assert_array_equal(k.gold_ranks(gold), want)               # the default: unchanged
    assert k.algorithm.rank_stats_ is None
    np.testing.assert_array_equal(k.gold_ranks(gold, route="sweep"), want)
    assert k.algorithm.rank_stats_["route_taken"] == 1
    with pytest.raises(NotImplementedError, match="reduced"):
        k.gold_ranks(gold, reduced=True, route="sweep")
    with pytest.raises(ValueError, match="route"):
        k.gold_ranks(gold, route="fast")
