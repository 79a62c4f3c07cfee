"""kz_radius_neighbors / kz_radius_neighbors_reduced where tests/test_gpu_radius.py does not reach (kiez_amd/csrc/kz_radius.h): the
row sort at every size branch -- the bitonic network at one, two, four and eight trips per thread and stage, the 4096 | 4097
hand-over, the radix path with zero, one, two, three, seven and eight passes, last tiles of 1, 255 and 256 entries, orders decided
by thousands of ties alone, radix rows beside LDS rows and a capacity that ends inside or exactly behind one -- the carry of the
chunk scan beyond 256 chunks, and the distance conversions and element types no native radius call has run.

The sort and scan tests drive the kernels through metric='precomputed': the plain call's w is the matrix entry itself, and with
KZ_RANK_DUAL it is (d - f_i) - g_j, exact on a dyadic grid, so a test chooses every row length and every key (the matrices:
tests/radius_restate.py, checked on the host by tests/test_radius.py).  Every bit-for-bit comparison is against numpy --
radius_restate.csr, a stable sort by (w, row), of a w computed in float64 on the host; the comparisons with other device calls
are additional and say so.  `pytest -m gpu`."""
import numpy as np
import pytest

from tests import boolean_restate as BR
from tests import half_inputs as H
from tests import metric_restate as MR
from tests import radius_restate as RA
from tests import reduced_rank_restate as RD
from tests import test_gpu_reduced_ranks as GR

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _radius(ctx, qm, ym, radius, kind=None, q_state=None, t_state=None, **kw):
    """N.radius_neighbors -> numpy (indptr, ind, dist, total)."""
    from kiez_amd import _native as N
    indptr, ind, dist, total = N.radius_neighbors(ctx, qm, ym, radius, kind, q_state, t_state, **kw)
    return indptr.numpy(), ind.numpy(), dist.numpy(), total


def _assert_csr(got, want, where):
    """got (indptr, ind, dist, total) is the restatement's (indptr, ind, values): ids, and the values bit for bit."""
    indptr, ind, dist, total = got
    assert indptr.dtype == np.int64 and ind.dtype == np.int64 and dist.dtype == np.float64, where
    np.testing.assert_array_equal(indptr, want[0], err_msg=where)
    assert total == want[0][-1] == ind.size == dist.size, where
    np.testing.assert_array_equal(ind, want[1], err_msg=where)
    np.testing.assert_array_equal(dist.view(np.int64), want[2].view(np.int64), err_msg=f"{where} (bits)")


def _assert_row_order(got, sort_results, where):
    """Sorted rows: values non-decreasing, ids ascending inside every run of equal keys; unsorted rows: ids ascending."""
    for ids, vals in zip(RA.rows(got[0], got[1]), RA.rows(got[0], got[2])):
        if sort_results:
            key = RA.order_key(vals)
            assert (key[1:] >= key[:-1]).all() and (vals[1:] >= vals[:-1]).all(), where      # (no np.diff: -inf - -inf)
            assert (np.diff(ids)[key[1:] == key[:-1]] > 0).all(), where
        else:
            assert (np.diff(ids) > 0).all(), where


# ---- 1. the row sort at every size branch and every key regime ------------------------------------------------------------------

@pytest.mark.parametrize("sort_results", [True, False], ids=["sorted", "by_row"])
@pytest.mark.parametrize("regime", RA.REGIMES, ids=RA.regime_id)
def test_row_sort_at_every_size_branch(ctx, regime, sort_results):
    """24 x 9000 float64 precomputed, row i with exactly LENGTHS[i] entries <= radius (radius_restate.planted): the whole CSR equals
    numpy's, ids and value bits."""
    from kiez_amd import _native as N
    D, radius = RA.planted(regime)
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D)
    got = _radius(ctx, rows_view, cols_view, radius, sort_results=sort_results)
    where = f"{RA.regime_id(regime)} sorted={sort_results}"
    _assert_csr(got, RA.csr(D, radius, sort_results), where)
    np.testing.assert_array_equal(np.diff(got[0]), RA.LENGTHS, err_msg=where)
    _assert_row_order(got, sort_results, where)


@pytest.mark.parametrize("sort_results", [True, False], ids=["sorted", "by_row"])
def test_row_sort_other_direction_and_float32(ctx, sort_results):
    """Additionally: 'grid8' with the columns view as the query -- 9000 rows of at most 24 entries, w = D.T -- and 'distinct' as a
    float32 matrix (w = the float64 of the float32 entry: keys that differ in bits 29 .. 62 only).  Both against numpy."""
    from kiez_amd import _native as N
    D, radius = RA.planted("grid8")
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D)
    got = _radius(ctx, cols_view, rows_view, radius, sort_results=sort_results)
    want = RA.csr(D.T, radius, sort_results)
    _assert_csr(got, want, f"grid8 transposed sorted={sort_results}")
    np.testing.assert_array_equal(np.diff(got[0]), (D.T <= radius).sum(axis=1))
    assert np.diff(got[0]).max() >= 10 and got[3] == sum(RA.LENGTHS)
    _assert_row_order(got, sort_results, "grid8 transposed")
    D32, radius32 = RA.planted("distinct", np.float32)
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D32)
    got = _radius(ctx, rows_view, cols_view, radius32, sort_results=sort_results)
    _assert_csr(got, RA.csr(D32, radius32, sort_results), f"distinct float32 sorted={sort_results}")
    np.testing.assert_array_equal(np.diff(got[0]), RA.LENGTHS)
    _assert_row_order(got, sort_results, "distinct float32")


# ---- 2. signs, infinities and NaN through both sort paths -----------------------------------------------------------------------

@pytest.mark.parametrize("radius", RA.SIGNED_RADII, ids=lambda r: f"radius_{r}")
def test_signs_infinities_and_nan_through_both_sort_paths(ctx, radius):
    """radius_restate.signed_case under KZ_RANK_DUAL: rows of 8997 (+inf: all eight radix passes, -inf entries first and +inf
    entries last by row, the NaN ids absent), about 4500 (0.0: radix, exact zeros), about 1150 (-3.0: LDS over 2048), about 120
    (-4.5) and 2 (-inf) entries.  The counts asserted are numpy's."""
    from kiez_amd import _native as N
    D, q_a, t_a, w = RA.signed_case()
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D)
    q_dev, t_dev = ctx.to_device(q_a), ctx.to_device(t_a)
    for sort_results in (True, False):
        where = f"dual radius {radius!r} sorted={sort_results}"
        got = _radius(ctx, rows_view, cols_view, radius, N.RANK_DUAL, q_dev, t_dev, sort_results=sort_results)
        want = RA.csr(w, radius, sort_results)
        _assert_csr(got, want, where)
        assert not np.isnan(got[2]).any() and not np.isin(got[1], RA.SIGNED_NAN).any(), where
        _assert_row_order(got, sort_results, where)
        if radius == np.inf and sort_results:
            for ids in RA.rows(got[0], got[1]):
                assert len(ids) == 8997 and tuple(ids[:2]) == RA.SIGNED_TO_MINUS_INF and tuple(ids[-2:]) == RA.SIGNED_TO_PLUS_INF, where
        if radius == -np.inf:
            np.testing.assert_array_equal(got[1], np.tile(RA.SIGNED_TO_MINUS_INF, 6), err_msg=where)


# ---- 3. capacity around radix rows ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sort_results", [True, False], ids=["sorted", "by_row"])
def test_capacity_inside_and_exactly_behind_a_radix_row(ctx, sort_results):
    """The 'distinct' matrix with a capacity exactly behind the 4097-entry first row, one more, and in the middle of the 9000-entry
    row 7: indptr and total are the full call's, the arrays have `capacity` entries, every row that ends at or before the capacity is
    complete and in order.  Nothing is asserted about the places behind the last complete row."""
    from kiez_amd import _native as N
    D, radius = RA.planted("distinct")
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D)
    full = RA.csr(D, radius, sort_results)
    assert full[0][1] == 4097 and full[0][8] - full[0][7] == 9000
    for capacity in (int(full[0][1]), int(full[0][1]) + 1, int(full[0][7]) + 4500):
        where = f"capacity {capacity} sorted={sort_results}"
        indptr, ind, dist, total = _radius(ctx, rows_view, cols_view, radius, sort_results=sort_results, capacity=capacity)
        np.testing.assert_array_equal(indptr, full[0], err_msg=where)
        assert total == full[0][-1] and ind.size == dist.size == capacity, where
        done = int(full[0][full[0] <= capacity].max())
        assert done in (4097, int(full[0][7])), where
        np.testing.assert_array_equal(ind[:done], full[1][:done], err_msg=where)
        np.testing.assert_array_equal(dist[:done].view(np.int64), full[2][:done].view(np.int64), err_msg=where)


# ---- 4. the scan beyond 256 chunks ----------------------------------------------------------------------------------------------

def test_scan_carry_beyond_256_chunks(ctx):
    """2 x 2 097 153 float32 precomputed (radius_restate.carry_case), 257 chunks: the offsets of chunk 256 stand on the carry of
    the 256 chunks before it, in an LDS row (8 entries, two of them around the carry) and in a radix row (5001 entries) beside it.
    `capacity` is given, so each call runs once."""
    from kiez_amd import _native as N
    D, radius = RA.carry_case()
    rows_view, cols_view = N.DeviceMatrix.precomputed(ctx, D)
    for sort_results in (True, False):
        want = RA.csr(D, radius, sort_results)
        got = _radius(ctx, rows_view, cols_view, radius, sort_results=sort_results, capacity=int(want[0][-1]))
        _assert_csr(got, want, f"257 chunks sorted={sort_results}")
    indptr, total = N.radius_counts(ctx, rows_view, cols_view, radius)
    np.testing.assert_array_equal(indptr.numpy(), want[0])
    assert total == 8 + 5001


# ---- 5. the conversions and element types no native radius call has run ---------------------------------------------------------

N_SOURCE, N_TARGETS, DIM = 96, (64, 257), 8


def _kind_id(kind):
    return None if kind == "plain" else RD.kind_id(kind)


def _with_ties(source, target):
    """Two identical index rows (equal distance, equal state, equal w: the tie goes by row) and two pairs of identical query rows."""
    target[len(target) - 2] = target[1]
    source[1], source[3] = source[0], source[2]


def _reduced(kind, dist, q_state, t_state):
    """The host's w of the host's distances: the distances themselves, or radius_restate's reduced form of them."""
    return dist if kind == "plain" else RD.reduce(kind, dist, q_state, t_state)


def _radii(w):
    """The radii of test_gpu_radius.py's conversion test, from the host's w: the midpoint of a gap; exactly one pair's own w (pair
    (0, 1), which ties with (0, n_t - 2)); below the minimum of half the rows (an all-NaN row has none); +inf, which leaves out
    the NaN values only."""
    minima = np.where(np.isnan(w), np.inf, w).min(axis=1)
    radii = {"gap": RA.gap_radius(w, per_row=5, window=200)[0], "below half the row minima": float(np.median(minima[minima < np.inf])),
             "+inf": np.inf}
    if not np.isnan(w[0, 1]):
        radii["one pair's own w"] = float(w[0, 1])
    return radii


def _check_against_host(ctx, qm, ym, kind, w, q_dev, t_dev, what):
    """Every radius of _radii(w), sorted and by row: the device's CSR is numpy's of the host's w, ids and value bits.  Returns the
    sorted results by radius name."""
    n_t = w.shape[1]
    assert w[0, 1].tobytes() == w[0, n_t - 2].tobytes() or (np.isnan(w[0, 1]) and np.isnan(w[0, n_t - 2])), what
    out = {}
    for name, r in _radii(w).items():
        for sort_results in (True, False):
            where = f"{what} {kind} n_target={n_t} radius {name} = {r!r} sorted={sort_results}"
            got = _radius(ctx, qm, ym, r, _kind_id(kind), q_dev, t_dev, sort_results=sort_results)
            _assert_csr(got, RA.csr(w, r, sort_results), where)
            assert not np.isnan(got[2]).any(), where
            counts = np.diff(got[0])
            if name == "one pair's own w":
                row0 = list(got[1][:counts[0]])
                assert 1 in row0 and n_t - 2 in row0, where
                if sort_results:
                    assert row0.index(1) < row0.index(n_t - 2), where
            if name == "below half the row minima":     # (rows whose minimum IS the radius are in: with ties, more than half)
                assert (counts > 0).sum() >= w.shape[0] // 2 - 2 and (counts > 0).sum() < w.shape[0], where
            if name == "+inf":
                np.testing.assert_array_equal(counts, (~np.isnan(w)).sum(axis=1), err_msg=where)
            if sort_results:
                out[name] = got
    return out


def _check_against_the_siblings(ctx, qm, ym, kind, q_dev, t_dev, results, rng, what):
    """ADDITIONALLY, against other device calls (they share kz_rank_dispatch): a sorted radius row of at most k entries is the head
    of kz_knn_reduced's list, ids and bits; kz_gold_ranks_reduced(gold)[i] < count_i exactly when gold[i] is in row i."""
    from kiez_amd import _native as N
    n_s, n_t = qm.shape[0], ym.shape[0]
    k = min(n_t, N.KNN_REDUCED_MAX_K)
    list_w, list_i = N.knn_reduced(ctx, qm, ym, k, _kind_id(kind), q_dev, t_dev)
    list_w, list_i = list_w.numpy(), list_i.numpy()
    gold = rng.integers(0, n_t, n_s).astype(np.int64)
    rank = N.gold_ranks_reduced(ctx, qm, ym, ctx.to_device(gold), _kind_id(kind), q_dev, t_dev).numpy()
    seen_in = seen_out = False
    for name, (indptr, ind, dist, _) in results.items():
        counts = np.diff(indptr)
        assert counts.max() <= k
        for i in range(n_s):
            np.testing.assert_array_equal(ind[indptr[i]:indptr[i + 1]], list_i[i, :counts[i]], err_msg=f"{what} {kind} radius {name} row {i}")
            np.testing.assert_array_equal(dist[indptr[i]:indptr[i + 1]].view(np.int64), list_w[i, :counts[i]].view(np.int64))
        inside = np.array([gold[i] in ind[indptr[i]:indptr[i + 1]] for i in range(n_s)])
        np.testing.assert_array_equal(rank < counts, inside, err_msg=f"{what} {kind} radius {name}")
        seen_in, seen_out = seen_in or inside.any(), seen_out or not inside.all()
    assert seen_in and seen_out


def _host_states(rng, kind, n_s, n_t):
    """Arbitrary positive state vectors (the two identical index rows share theirs), on the host and on the device."""
    if kind == "plain":
        return None, None
    q_state, t_state = (rng.random(n_s) + 0.5,), (rng.random(n_t) + 0.5,)
    t_state[0][n_t - 2] = t_state[0][1]
    return q_state, t_state


def _dev(ctx, state):
    return None if state is None else tuple(ctx.to_device(v) for v in state)


@pytest.mark.parametrize("kind", ["plain", "csls", "nicdm"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_seuclidean(ctx, dtype, kind):
    """KZ_SEUCLIDEAN, both roundings of its sqrt, with variances over six orders of magnitude: the host's w is
    metric_restate's sqrt of its ranking value (bit-exact restatements), reduced by reduced_rank_restate."""
    from kiez_amd import _native as N
    for n_t in N_TARGETS:
        rng = np.random.default_rng(700 + n_t)
        source, target = rng.standard_normal((N_SOURCE, DIM)).astype(dtype), rng.standard_normal((n_t, DIM)).astype(dtype)
        _with_ties(source, target)
        V = 10.0 ** rng.uniform(-3.0, 3.0, DIM)
        qm, ym = N.DeviceMatrix(ctx, source, "seuclidean", V=V), N.DeviceMatrix(ctx, target, "seuclidean", V=V)
        dist = MR.output_distance("seuclidean", MR.ranking_values("seuclidean", source, target, V), dtype)
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        q_dev, t_dev = _dev(ctx, q_state), _dev(ctx, t_state)
        results = _check_against_host(ctx, qm, ym, kind, _reduced(kind, dist, q_state, t_state), q_dev, t_dev, f"seuclidean {np.dtype(dtype).name}")
        if kind != "plain":
            _check_against_the_siblings(ctx, qm, ym, kind, q_dev, t_dev, results, rng, "seuclidean")


@pytest.mark.parametrize("kind", ["plain", "csls", "nicdm"])
def test_correlation_with_constant_rows(ctx, kind):
    """KZ_CORRELATION, float64: the group whose +inf ranking value is a NaN distance.  Two constant index rows and one constant query
    row: those pairs are NaN and absent at every radius, +inf included; every other row is non-empty there."""
    from kiez_amd import _native as N
    for n_t in N_TARGETS:
        rng = np.random.default_rng(800 + n_t)
        source, target = rng.standard_normal((N_SOURCE, DIM)), rng.standard_normal((n_t, DIM))
        _with_ties(source, target)
        target[5], target[n_t - 3], source[7] = 1.5, -2.0, 0.25
        qm, ym = N.DeviceMatrix(ctx, source, "correlation"), N.DeviceMatrix(ctx, target, "correlation")
        dist = MR.ranking_values("correlation", source, target)
        assert np.isnan(dist[7]).all() and np.isnan(dist[:, [5, n_t - 3]]).all() and np.isnan(dist).sum() == n_t + 2 * (N_SOURCE - 1)
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        q_dev, t_dev = _dev(ctx, q_state), _dev(ctx, t_state)
        results = _check_against_host(ctx, qm, ym, kind, _reduced(kind, dist, q_state, t_state), q_dev, t_dev, "correlation")
        indptr, ind, _, _ = results["+inf"]
        counts = np.diff(indptr)
        assert counts[7] == 0 and (np.delete(counts, 7) == n_t - 2).all()
        assert not np.isin(ind, [5, n_t - 3]).any()
        if kind != "plain":
            _check_against_the_siblings(ctx, qm, ym, kind, q_dev, t_dev, results, rng, "correlation")


@pytest.mark.parametrize("kind", ["plain", "csls", "nicdm"])
@pytest.mark.parametrize("metric", ["braycurtis", "hamming"])
def test_braycurtis_and_hamming_float32(ctx, metric, kind):
    """float32 rows of two metrics whose ranking value is the distance (hamming: features in {0, 1, 2}, nine distinct values)."""
    from kiez_amd import _native as N
    for n_t in N_TARGETS:
        rng = np.random.default_rng(900 + n_t)
        draw = (lambda n: rng.integers(0, 3, (n, DIM)).astype(np.float32)) if metric == "hamming" \
            else (lambda n: rng.standard_normal((n, DIM)).astype(np.float32))
        source, target = draw(N_SOURCE), draw(n_t)
        _with_ties(source, target)
        qm, ym = N.DeviceMatrix(ctx, source, metric), N.DeviceMatrix(ctx, target, metric)
        dist = MR.output_distance(metric, MR.ranking_values(metric, source, target), np.float32)
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        _check_against_host(ctx, qm, ym, kind, _reduced(kind, dist, q_state, t_state), _dev(ctx, q_state), _dev(ctx, t_state), metric)


@pytest.mark.parametrize("metric,kind", [("dice", "plain"), ("dice", "csls"), ("jaccard", "plain"), ("jaccard", "csls"), ("jaccard", "nicdm")])
def test_boolean_metrics_order_by_ties(ctx, metric, kind):
    """24 boolean features: few distinct values, so the order inside a row is mostly by ties.  dice with three all-false rows on
    each side: those nine pairs are NaN (0 / 0) and absent at every radius; NICDM runs on jaccard, which has no NaN."""
    from kiez_amd import _native as N
    for n_t in N_TARGETS:
        rng = np.random.default_rng(2000 + n_t)             # (no row is all false by chance)
        source, target = (rng.random((N_SOURCE, 24)) < 0.3).astype(np.float32), (rng.random((n_t, 24)) < 0.3).astype(np.float32)
        _with_ties(source, target)
        if metric == "dice":
            source[[5, 40, 95]] = 0.0
            target[[0, 33, n_t - 1]] = 0.0
        qm, ym = N.DeviceMatrix(ctx, source, metric), N.DeviceMatrix(ctx, target, metric)
        dist = BR.ranking_values(metric, source, target)
        assert int(np.isnan(dist).sum()) == (9 if metric == "dice" else 0) and len(np.unique(dist[~np.isnan(dist)])) < 200
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        results = _check_against_host(ctx, qm, ym, kind, _reduced(kind, dist, q_state, t_state), _dev(ctx, q_state), _dev(ctx, t_state), metric)
        if metric == "dice":
            indptr, ind, _, _ = results["+inf"]
            for i in (5, 40, 95):
                assert indptr[i + 1] - indptr[i] == n_t - 3 and not np.isin(ind[indptr[i]:indptr[i + 1]], [0, 33, n_t - 1]).any()


@pytest.mark.parametrize("kind", ["plain", "csls"])
@pytest.mark.parametrize("metric", ["minkowski[3.0]", "minkowski[1.5]", "manhattan"], ids=["minkowski3", "minkowski1.5", "manhattan"])
def test_float64_minkowski_family_on_the_devices_values(ctx, metric, kind):
    """The float64 form of KZ_MINKOWSKI's pow and manhattan.  THIS ONE CASE RESTS ON THE DEVICE'S VALUES: the suite has no bit-exact
    numpy restatement of these sums, so -- the construction of test_gpu_radius.py::test_chunks_and_parities -- w is the device's own
    value matrix (kz_pair_values) converted and reduced in numpy.  The radius stands in a gap of that w asserted to be > 4e-12, the
    bound that test uses: numpy's pow and the device's differ by an ulp or so (values of order 1: ~2e-16), so the ids are numpy's;
    the values are compared within 1e-12, and for manhattan, which converts nothing, bit for bit."""
    from kiez_amd import _native as N
    p = N.split_metric(metric)[1]
    for n_t in N_TARGETS:
        rng = np.random.default_rng(1100 + n_t)
        source, target = rng.standard_normal((N_SOURCE, DIM)), rng.standard_normal((n_t, DIM))
        _with_ties(source, target)
        qm, ym = N.DeviceMatrix(ctx, source, metric), N.DeviceMatrix(ctx, target, metric)
        vals = GR._all_pair_values(ctx, qm, ym)
        dist = vals if p is None else vals ** (1.0 / p)
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        w = _reduced(kind, dist, q_state, t_state)
        r, gap = RA.gap_radius(w, per_row=5, window=200)
        assert gap > 4e-12
        for radius in (r, np.inf):
            for sort_results in (True, False):
                where = f"{metric} {kind} n_target={n_t} radius {radius!r} sorted={sort_results}"
                got = _radius(ctx, qm, ym, radius, _kind_id(kind), _dev(ctx, q_state), _dev(ctx, t_state), sort_results=sort_results)
                want = RA.csr(w, radius, sort_results)
                assert got[2].dtype == np.float64 and got[3] == want[0][-1], where
                np.testing.assert_array_equal(got[0], want[0], err_msg=where)
                if p is None:
                    _assert_csr(got, want, where)
                else:                                       # (values an ulp apart may swap places in a sorted row: the sets)
                    for a, b in zip(RA.rows(got[0], got[1]), RA.rows(want[0], want[1])):
                        np.testing.assert_array_equal(a if not sort_results else np.sort(a), b if not sort_results else np.sort(b), err_msg=where)
                    assert np.abs(got[2] - w[np.repeat(np.arange(N_SOURCE), np.diff(got[0])), got[1]]).max() <= 1e-12, where
                _assert_row_order(got, sort_results, where)
                if radius == r:
                    assert 2 * N_SOURCE <= got[3] <= 8 * N_SOURCE, where
                elif sort_results:                          # the two identical index rows are neighbours in every row, by row
                    for ids in RA.rows(got[0], got[1]):
                        at = list(ids).index(1)
                        assert ids[at + 1] == n_t - 2, where


@pytest.mark.parametrize("kind", ["plain", "csls"])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("elem", H.HALF_ELEMS)
def test_half_rows_equal_the_float64_matrix_of_the_widened_values(ctx, elem, metric, kind):
    """float16 / bfloat16 rows (T = double: the float64 conventions).  The contract of the 2-byte element types: the result equals
    the call on the KZ_F64 matrix of the widened values -- ids, value bits, float64 -- which is a comparison of two device calls;
    ADDITIONALLY the ids equal numpy's, from float64 distances of the widened rows, at a radius in a gap > 4e-12 of them."""
    from kiez_amd import _native as N
    for n_t in N_TARGETS:
        rng = np.random.default_rng(1200 + n_t)
        s_dev, s64 = H.draw(N_SOURCE, DIM, elem, 12 + n_t)
        t_dev, t64 = H.draw(n_t, DIM, elem, 1012 + n_t)
        for a in (s_dev, s64):
            a[1], a[3] = a[0], a[2]
        for a in (t_dev, t64):
            a[n_t - 2] = a[1]
        half = [N.DeviceMatrix(ctx, x, metric, elem="bfloat16" if elem == "bfloat16" else None) for x in (s_dev, t_dev)]
        wide = [N.DeviceMatrix(ctx, x, metric) for x in (s64, t64)]
        assert half[0].elem == half[1].elem == elem and wide[0].elem == wide[1].elem == "float64"
        if metric == "euclidean":
            dist = np.sqrt(((s64[:, None, :] - t64[None, :, :]) ** 2).sum(axis=2))
        else:
            dist = 1.0 - (s64 @ t64.T) / (np.linalg.norm(s64, axis=1)[:, None] * np.linalg.norm(t64, axis=1)[None, :])
        q_state, t_state = _host_states(rng, kind, N_SOURCE, n_t)
        q_dev, t_dev_state = _dev(ctx, q_state), _dev(ctx, t_state)
        w = _reduced(kind, dist, q_state, t_state)
        r, gap = RA.gap_radius(w, per_row=5, window=200)
        assert gap > 4e-12
        for name, radius in (("gap", r), ("below half the row minima", float(np.median(w.min(axis=1)))), ("+inf", np.inf)):
            for sort_results in (True, False):
                where = f"{elem} {metric} {kind} n_target={n_t} radius {name} sorted={sort_results}"
                got = _radius(ctx, half[0], half[1], radius, _kind_id(kind), q_dev, t_dev_state, sort_results=sort_results)
                ref = _radius(ctx, wide[0], wide[1], radius, _kind_id(kind), q_dev, t_dev_state, sort_results=sort_results)
                _assert_csr(got, ref[:3], where)
                _assert_row_order(got, sort_results, where)
                if name == "gap":                           # numpy decides every pair the same way
                    want = RA.csr(w, radius, sort_results=False)
                    np.testing.assert_array_equal(got[0], want[0], err_msg=where)
                    for a, b in zip(RA.rows(got[0], got[1]), RA.rows(want[0], want[1])):
                        np.testing.assert_array_equal(np.sort(a), b, err_msg=where)
                    assert 2 * N_SOURCE <= got[3] <= 8 * N_SOURCE, where
                if name == "+inf":
                    assert got[3] == N_SOURCE * n_t, where
