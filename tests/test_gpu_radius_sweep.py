"""radius_neighbors / radius_counts (route="sweep") -- kz_radius_neighbors_sweep: the fp16 emit / count sweep plus the exact values of
its candidates -- against two references per case: (a) a plain numpy float64 brute force of "all pairs with distance <= radius" and
(b) route="exact" on the same handles, byte for byte (the project's anchor), for sort_results True and False.

The numpy brute force is only a reference where the data lets it be one: the radius sits in a gap of the float64 distances
(radius_restate.gap_radius) that is at least 1e-9 relative.  That is a condition on the data, asserted here on the CPU for every case;
the seeds are fixed so that it holds."""
import ctypes as C

import numpy as np
import pytest

from tests import radius_restate as RR

pytestmark = pytest.mark.gpu
STAT_KEYS = ("route_taken", "overflowed", "n_rows", "n_candidates", "n_pairs", "max_err_ratio")


def make_case(n_q, n_i, d, seed, dups=0, nan_row=None, scale=1.0, offset=0.0):
    """Gaussian queries and index; `dups`: that many exact copies of one index row next to query 0, spread over the index (ties that
    go by row); `nan_row`: a query row with one NaN feature."""
    rng = np.random.default_rng(seed)
    q, y = rng.standard_normal((n_q, d)), rng.standard_normal((n_i, d))
    if dups:
        y[np.sort(rng.choice(n_i, dups, replace=False))] = q[0] + 0.05 * rng.standard_normal(d)
    q, y = ((a * 1e-3 + 1.0 if offset else a) * scale for a in (q, y))   # (offset: 10^3 spreads)
    q, y = q.astype(np.float32), y.astype(np.float32)
    if nan_row is not None:
        q[nan_row, d // 2] = np.nan
    return q, y


def numpy_distances(q, y, metric):
    q, y = q.astype(np.float64), y.astype(np.float64)
    with np.errstate(invalid="ignore"):   # (a NaN query row)
        if metric == "cosine":
            q, y = q / np.linalg.norm(q, axis=1, keepdims=True), y / np.linalg.norm(y, axis=1, keepdims=True)
            return 1.0 - q @ y.T
        v = np.maximum((q * q).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (q @ y.T), 0.0)
        return np.sqrt(v) if metric == "euclidean" else v


def pick_radius(w, per_row):
    """A radius in a gap of w with about per_row pairs a row (0: three pairs in all) and the assertion that the gap is one."""
    if per_row:
        radius, gap = RR.gap_radius(w, per_row)
    else:
        flat = np.sort(w[~np.isnan(w)], axis=None)
        radius, gap = 0.5 * (flat[2] + flat[3]), flat[3] - flat[2]
    assert gap >= 1e-9 * radius, f"precondition: the gap around the radius is {gap / radius:.3g} relative"
    return radius


def call(qm, im, radius, route, stats=None, **kw):
    from kiez_amd import _native as N
    indptr, ind, dist, total = N.radius_neighbors(N.Context.get(), qm, im, radius, route=route, stats=stats, **kw)
    return indptr.numpy(), ind.numpy(), dist.numpy(), total


def assert_same_bytes(a, b, capacity=None):
    """indptr and total equal; ind / dist byte-equal over the rows that end within the capacity (the rows the contract writes)."""
    np.testing.assert_array_equal(a[0], b[0])
    assert a[3] == b[3]
    n = a[3] if capacity is None else int(a[0][a[0] <= capacity].max())
    np.testing.assert_array_equal(a[1][:n], b[1][:n])
    assert a[2][:n].tobytes() == b[2][:n].tobytes()


def check(n_q, n_i, d, metric, per_row=8, dtype=np.float32, seed=0, benign=True, radius=None, reference=True, **kw):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y = make_case(n_q, n_i, d, seed, **kw)
    q, y = q.astype(dtype), y.astype(dtype)
    w = numpy_distances(q, y, metric)
    if radius is None:
        radius = pick_radius(w, per_row)
    im = N.DeviceMatrix(ctx, y, metric)
    if np.isnan(q).any():   # (host rows with a NaN are refused: the row arrives as device rows, which no radius call inspects)
        q_dev = ctx.to_device(q)
        qm = N.DeviceMatrix(ctx, None, metric, device_ptr=q_dev.ptr.value, shape=q.shape, dtype=q.dtype)
    else:
        qm = N.DeviceMatrix(ctx, q, metric)
    takes_sweep = n_i >= 128 and dtype == np.float32 and 0.0 <= radius < np.inf
    for sort_results in (True, False):
        stats = {}
        sweep = call(qm, im, radius, "sweep", stats, sort_results=sort_results)
        print(f"{n_q} x {n_i} x {d} {metric} {np.dtype(dtype).name} r={radius:.6g} {kw}: {[{k: c[k] for k in STAT_KEYS} for c in stats['calls']]}")
        assert_same_bytes(sweep, call(qm, im, radius, "exact", sort_results=sort_results))
        for c in stats["calls"]:
            assert c["route_taken"] == int(takes_sweep) or not benign
            if takes_sweep and benign:   # (without this the fallback could hide a broken sweep)
                assert c["overflowed"] == 0 and c["max_err_ratio"] <= 1.0 and c["n_rows"] == n_q
    if reference:
        want = RR.csr(w, radius, sort_results=False)
        np.testing.assert_array_equal(sweep[0], want[0])
        np.testing.assert_array_equal(sweep[1], want[1])   # (rows ascending by index row: the sets, as sequences)
    # the capacity contract: the count-only call, a capacity inside a row, the exact total
    total, mid = sweep[3], int(sweep[0][n_q // 2] + sweep[0][n_q // 2 + 1]) // 2
    cstats = {}
    indptr, n = N.radius_counts(ctx, qm, im, radius, route="sweep", stats=cstats)
    np.testing.assert_array_equal(indptr.numpy(), sweep[0])
    assert n == total and (cstats["route_taken"] == int(takes_sweep) or not benign)
    for capacity in {mid, total} - {0}:
        assert_same_bytes(call(qm, im, radius, "sweep", capacity=capacity), call(qm, im, radius, "exact", capacity=capacity), capacity)
    return qm, im, sweep, stats


@pytest.mark.parametrize("d,metric", [(17, "cosine"), (144, "euclidean"), (208, "sqeuclidean"), (224, "cosine"), (384, "euclidean")])
def test_widths_and_metrics(d, metric):
    check(300, 4097, d, metric, seed=d)


@pytest.mark.parametrize("n_i", [127, 128, 129, 4097])
def test_index_sizes_around_one_tile(n_i):
    check(129, n_i, 100, "euclidean")


@pytest.mark.parametrize("n_q", [1, 127, 129, 300])
def test_query_sizes(n_q):
    check(n_q, 4097, 32, "sqeuclidean", seed=n_q)


@pytest.mark.parametrize("q_begin,q_count", [(37, 150), (299, 1)])
def test_row_ranges(q_begin, q_count):
    """A row range (two query tiles, the second partial; the last row alone), neighbours for both sort_results and the count-only
    call: the bytes of route="exact" on the same range, the slice of the whole-range result, and the sweep's own route on every row
    of the range -- a fallback cannot hide a broken range."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y = make_case(300, 4097, 32, 0)
    radius = pick_radius(numpy_distances(q, y, "euclidean"), 8)
    qm, im = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    for sort_results in (True, False):
        whole = call(qm, im, radius, "sweep", sort_results=sort_results)
        lo, hi = whole[0][q_begin], whole[0][q_begin + q_count]
        stats = {}
        got = call(qm, im, radius, "sweep", stats, sort_results=sort_results, q_begin=q_begin, q_count=q_count)
        print(f"rows [{q_begin}, {q_begin + q_count}) sorted={sort_results}: {[{k: c[k] for k in STAT_KEYS} for c in stats['calls']]}")
        assert_same_bytes(got, call(qm, im, radius, "exact", sort_results=sort_results, q_begin=q_begin, q_count=q_count))
        np.testing.assert_array_equal(got[0], whole[0][q_begin:q_begin + q_count + 1] - lo)
        np.testing.assert_array_equal(got[1], whole[1][lo:hi])
        assert got[2].tobytes() == whole[2][lo:hi].tobytes() and got[3] == hi - lo
        assert all(c["route_taken"] == 1 and c["n_rows"] == q_count for c in stats["calls"])
    cstats = {}
    indptr, n = N.radius_counts(ctx, qm, im, radius, q_begin=q_begin, q_count=q_count, route="sweep", stats=cstats)
    exact_indptr, exact_n = N.radius_counts(ctx, qm, im, radius, q_begin=q_begin, q_count=q_count)
    assert indptr.numpy().tobytes() == exact_indptr.numpy().tobytes() and n == exact_n
    np.testing.assert_array_equal(indptr.numpy(), got[0])
    assert cstats["route_taken"] == 1 and cstats["n_rows"] == q_count


def test_several_index_ranges_per_query_tile():
    from kiez_amd import _native as N
    n, qt, pc, ln = C.c_int(0), (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    for slots in (512, 768):   # (two or three workgroups on each of 256 CUs: the plan the sweep's launcher makes)
        assert N.load().kz_knn_plan(300, 20001, 1, slots, 0, 1, C.byref(n), qt, pc, ln) == 0 and min(pc[:n.value]) >= 2
    check(300, 20001, 32, "sqeuclidean")


@pytest.mark.parametrize("per_row", [0, 8, 200])
def test_radii(per_row):
    check(300, 4097, 100, "euclidean", per_row=per_row)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_radius_on_a_stored_value(metric):
    # (a tie at the threshold that the band must resolve as <=; numpy's float64 has no say at a tie: reference (b) alone)
    qm, im, sweep, _ = check(300, 4097, 100, metric)
    stored = float(sweep[2][sweep[3] // 2])
    _, _, again, _ = check(300, 4097, 100, metric, radius=stored, reference=False)
    assert (again[2] == stored).any() and again[2].max() == stored


def test_duplicate_index_rows():
    _, _, sweep, _ = check(300, 4097, 100, "euclidean", dups=5)
    assert sweep[0][1] >= 5   # (query 0 holds the copies, in index order)


def test_a_nan_query_row():
    # (device rows only: host rows with a NaN are refused.  The exact route's fmax(NaN, 0) gives the row the value 0 against every
    #  index row -- a full row where numpy has an empty one --, so the call takes the exact route: same bytes, reference (b) alone)
    _, _, sweep, stats = check(300, 4097, 100, "euclidean", nan_row=7, benign=False, reference=False)
    assert sweep[0][8] - sweep[0][7] == 4097 and all(c["route_taken"] == 0 for c in stats["calls"])


@pytest.mark.parametrize("radius", [np.inf, -1.0])
def test_radii_outside_the_sweep(radius):
    check(129, 300, 32, "euclidean", radius=radius)   # (exact route, same bytes)


def test_nan_radius():
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y = make_case(129, 300, 32, 0)
    with pytest.raises(ValueError, match="NaN"):
        N.radius_neighbors(ctx, N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean"), float("nan"), route="sweep")


def test_log_overflow_takes_the_exact_route():
    # (1.21 M candidates against a log of 2^20)
    _, _, sweep, stats = check(1100, 1100, 32, "euclidean", radius=1e3, benign=False)
    assert sweep[3] == 1100 * 1100 and all(c["overflowed"] == 1 and c["route_taken"] == 0 for c in stats["calls"])


@pytest.mark.parametrize("dtype", [np.float64, np.float16])
def test_other_element_types_take_the_exact_route(dtype):
    check(300, 4097, 100, "euclidean", dtype=dtype)


@pytest.mark.parametrize("kw", [{"scale": 2.0 ** -20}, {"offset": 1.0}])
def test_magnitudes(kw):
    # (the bound is made of magnitudes: far from unit scale the call may fall back, the bytes may not change)
    check(300, 4097, 100, "euclidean", benign=False, **kw)


def test_interface():
    from kiez_amd import Kiez
    q, y = make_case(300, 4097, 100, 0)
    radius = pick_radius(numpy_distances(q, y, "euclidean"), 8)
    k = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"})
    k.fit(q, y)
    want = k.radius_neighbors(radius)               # the default: unchanged
    assert k.algorithm.radius_stats_ is None
    got = k.radius_neighbors(radius, route="sweep")
    assert k.algorithm.radius_stats_["route_taken"] == 1
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    counts = k.radius_counts(radius, route="sweep")
    assert k.algorithm.radius_stats_["route_taken"] == 1
    np.testing.assert_array_equal(counts, k.radius_counts(radius))
    with pytest.raises(NotImplementedError, match="reduced"):
        k.radius_neighbors(radius, reduced=True, route="sweep")
    with pytest.raises(ValueError, match="route"):
        k.radius_counts(radius, route="fast")
