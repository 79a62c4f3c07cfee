"""gold_ranks_reduced_sweep -- kz_gold_ranks_reduced_sweep: the rank-one count sweep of the fp16 images plus the exact w of its band --
against two references per case: (a) gold_ranks_reduced (the exact route) on the same handles, on every row, and (b) a plain numpy
float64 count #{w_j < w_g} from the same state vectors, exact duplicate rows with equal state tying by row.

numpy is a reference for a row only if no non-duplicate index row lies within tol |w_g| of its gold value: tol = 1e-9 under cosine and
sqeuclidean (no row may be left out), 1e-6 under euclidean (the float32 rounding of the distance; at most 3 % of the gold rows).
State vectors as in the reduced-list test: q_a = U(0.8, 1.2) x the mean distance, t_a = U(0.5, 2) x the mean."""
import numpy as np
import pytest

from tests.test_gpu_gold_ranks_sweep import make_case
from tests.test_gpu_knn_reduced_sweep import KINDS, numpy_distances, numpy_w

pytestmark = pytest.mark.gpu


def check(kind, metric, d, n_q=256, n_i=4097, dtype=np.float32, seed=0, benign=True, exact_route=False, spoil=None, flat_t=False, **kw):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y, gold = make_case(n_q, n_i, d, seed, **kw)
    q, y = q.astype(dtype), y.astype(dtype)
    dist = numpy_distances(q, y, metric)
    rng = np.random.default_rng(seed + 1)
    mean = dist.mean()
    q_a, t_a = rng.uniform(0.8, 1.2, n_q) * mean, (np.ones(n_i) if flat_t else rng.uniform(0.5, 2.0, n_i)) * mean
    if spoil:
        spoil(q_a, t_a)
    q_state, t_state = [q_a], [t_a]
    if kind == "mp_normal":
        q_state, t_state = q_state + [np.full(n_q, 0.3 * mean)], t_state + [np.full(n_i, 0.3 * mean)]
    qm, im = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
    gold_dev = ctx.to_device(np.where(gold < 0, np.iinfo(np.int64).min, gold))
    dev = lambda vs: tuple(ctx.to_device(np.ascontiguousarray(v)) for v in vs)   # noqa: E731
    args = (ctx, qm, im, gold_dev, KINDS[kind], dev(q_state), dev(t_state))
    stats = {}
    sweep = N.gold_ranks_reduced_sweep(*args, stats=stats).numpy()
    exact = N.gold_ranks_reduced(*args).numpy()
    print(f"{kind} {metric} {n_q} x {n_i} x {d} {np.dtype(dtype).name} {kw}: {stats}")
    np.testing.assert_array_equal(sweep, exact)                                         # (a)
    assert stats["n_rows"] == np.count_nonzero(gold >= 0)
    if exact_route:
        assert stats["route_taken"] == 0
        return stats
    if kind != "mp_normal":                                                             # (b)
        w = numpy_w(kind, dist, q_a, t_a)
        tol, cols, left_out = (1e-6 if metric == "euclidean" else 1e-9), np.arange(n_i), 0
        for r in np.flatnonzero(gold >= 0):
            g = gold[r]
            dup = (y == y[g]).all(1) & (t_a == t_a[g])
            if (~dup & (np.abs(w[r] - w[r, g]) <= tol * abs(w[r, g]))).any():
                left_out += 1
                continue
            assert sweep[r] == np.count_nonzero(np.where(dup, cols < g, w[r] < w[r, g])), f"row {r}"
        assert left_out <= (0.03 * np.count_nonzero(gold >= 0) if metric == "euclidean" else 0), f"{left_out} rows left out"
    assert stats["route_taken"] == 1
    if benign:                                                                          # (c): the fallback cannot hide a broken sweep
        assert stats["n_fallback_rows"] == 0 and stats["n_sweep_rows"] == stats["n_rows"] and stats["max_err_ratio"] <= 1.0
    return stats


@pytest.mark.parametrize("d", [17, 100, 144, 224, 384])
def test_slice_classes(d):
    check("csls", "euclidean", d, seed=d)


@pytest.mark.parametrize("n_i", [127, 128, 129])
def test_index_sizes_around_one_tile(n_i):
    check("csls", "euclidean", 100, n_i=n_i, exact_route=n_i < 128)


def test_several_index_ranges_per_query_tile():
    check("csls", "sqeuclidean", 32, n_q=300, n_i=20001)


@pytest.mark.parametrize("q_begin,q_count", [(37, 150), (299, 1)])
def test_row_ranges(q_begin, q_count):
    """A row range (two query tiles, the second partial; the last row alone): the bytes of the exact route on the same range, the
    slice of the whole-range result, and the sweep's own route on every row of the range -- a fallback cannot hide a broken range."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y, gold = make_case(300, 4097, 32, 0)
    q, y = q.astype(np.float32), y.astype(np.float32)
    rng = np.random.default_rng(1)
    mean = numpy_distances(q, y, "euclidean").mean()
    q_a, t_a = rng.uniform(0.8, 1.2, 300) * mean, rng.uniform(0.5, 2.0, 4097) * mean
    qm, im = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    dev_gold = lambda g: ctx.to_device(np.where(g < 0, np.iinfo(np.int64).min, g))   # noqa: E731
    t_state = (ctx.to_device(t_a),)
    rows = slice(q_begin, q_begin + q_count)
    assert (gold[rows] >= 0).all()
    whole = N.gold_ranks_reduced_sweep(ctx, qm, im, dev_gold(gold), KINDS["csls"], (ctx.to_device(q_a),), t_state).numpy()
    args = (ctx, qm, im, dev_gold(gold[rows]), KINDS["csls"], (ctx.to_device(np.ascontiguousarray(q_a[rows])),), t_state, q_begin, q_count)
    stats = {}
    got = N.gold_ranks_reduced_sweep(*args, stats=stats).numpy()
    print(f"rows [{q_begin}, {q_begin + q_count}): {stats}")
    assert got.tobytes() == N.gold_ranks_reduced(*args).numpy().tobytes()
    np.testing.assert_array_equal(got, whole[rows])
    assert stats["route_taken"] == 1 and stats["n_rows"] == q_count


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cosine"])
@pytest.mark.parametrize("kind", ["csls", "ls", "nicdm", "dual"])
def test_kinds_and_metrics(kind, metric):
    check(kind, metric, 100)


def test_ties_by_row_and_the_per_row_cap():
    check("csls", "euclidean", 100, dups=5, benign=False)
    stats = check("csls", "euclidean", 100, n_i=8193, dups=3000, flat_t=True, benign=False)
    assert stats["n_fallback_rows"] >= 1   # (3 000 tied band entries of one row: beyond the per-row cap)


@pytest.mark.parametrize("kw", [{"scale": 2.0 ** -20}, {"offset": 1.0}])
def test_magnitudes(kw):
    check("csls", "euclidean", 100, benign=False, **kw)


def _set(side, at, value):
    def spoil(q_a, t_a):
        (q_a if side == "q" else t_a)[at] = value
    return spoil


@pytest.mark.parametrize("kind,kw", [("csls", dict(dtype=np.float64)), ("mp_normal", {}), ("csls", dict(spoil=_set("t", 4000, np.nan))),
                                     ("nicdm", dict(spoil=_set("t", 77, -1.0)))], ids=["float64", "mp_normal", "nan_state", "negative_state"])
def test_must_take_the_exact_route(kind, kw):
    check(kind, "euclidean", 100, exact_route=True, **kw)


def test_kiez_end_to_end():
    from kiez_amd import Kiez
    rng = np.random.default_rng(5)
    source, target = rng.standard_normal((300, 64)).astype(np.float32), rng.standard_normal((4097, 64)).astype(np.float32)
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(source, target)
    gold = rng.integers(0, 4097, 300)
    got = kz.hubness.gold_ranks(gold, route="sweep")
    assert kz.algorithm.rank_stats_["route_taken"] == 1
    np.testing.assert_array_equal(got, kz.gold_ranks(gold, reduced=True))
    with pytest.raises(ValueError, match="route"):
        kz.hubness.gold_ranks(gold, route="fast")
