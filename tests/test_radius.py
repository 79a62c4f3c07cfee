"""The numpy restatement of the radius calls (tests/radius_restate.py) against scikit-learn's
NearestNeighbors(algorithm="brute").radius_neighbors(sort_results=True), the argument errors the new methods raise on the host
before any device call, and the restated sort key and planted matrices of tests/test_gpu_radius_sort.py: row lengths, radix pass
sets, finite and non-negative entries.  No GPU."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist

from tests import radius_restate as RA


@pytest.fixture(scope="module")
def rows():
    """default_rng(7): source 257 x 24, target 9001 x 24, uniform float32 rows, as their float64 copies."""
    rng = np.random.default_rng(7)
    source = rng.random((257, 24), dtype=np.float32).astype(np.float64)
    target = rng.random((9001, 24), dtype=np.float32).astype(np.float64)
    return source, target


@pytest.mark.parametrize("metric,scipy_metric", [("euclidean", "euclidean"), ("manhattan", "cityblock"), ("cosine", "cosine")])
def test_restatement_is_scikit_learns_radius_neighbors(rows, metric, scipy_metric):
    """The radius sits in the middle of the widest gap among the 2 000 sorted pair distances around the (20 x 257)-th: the gap is
    asserted to be > 1e-9 radius (measured: relative gaps of 8e-5 to 2e-4), far beyond what two float64 evaluations of a distance
    differ by, so scikit-learn alone decides every pair; about 20 pairs a row, rows from empty to over 100."""
    from sklearn.neighbors import NearestNeighbors
    source, target = rows
    d = cdist(source, target, scipy_metric)
    radius, gap = RA.gap_radius(d)
    indptr, ind, val = RA.csr(d, radius)
    counts = np.diff(indptr)
    print(metric, "radius", radius, "relative gap", gap / radius, "pairs per row", counts.mean(), "row counts", counts.min(), "to", counts.max())
    assert gap > 1e-9 * radius
    assert indptr[0] == 0 and indptr[-1] == ind.size == val.size and 10 * 257 < ind.size < 30 * 257
    want_d, want_i = NearestNeighbors(algorithm="brute", metric=metric).fit(target).radius_neighbors(source, radius=radius, sort_results=True)
    got_i, got_d = RA.rows(indptr, ind), RA.rows(indptr, val)
    for i in range(source.shape[0]):
        np.testing.assert_array_equal(got_i[i], want_i[i], err_msg=f"{metric} row {i}")
        np.testing.assert_allclose(got_d[i], want_d[i], rtol=1e-9, atol=0, err_msg=f"{metric} row {i}")
        assert (np.diff(got_d[i]) >= 0).all()
    if metric in ("euclidean", "cosine"):
        assert (counts == 0).any()                 # (an empty row: the abstain case is in the data)
    # by row alone: the same sets, ascending
    indptr_u, ind_u, val_u = RA.csr(d, radius, sort_results=False)
    np.testing.assert_array_equal(indptr_u, indptr)
    for a, b in zip(RA.rows(indptr_u, ind_u), got_i):
        np.testing.assert_array_equal(a, np.sort(b))
    np.testing.assert_array_equal(val_u, d[np.repeat(np.arange(257), counts), ind_u])


def test_restatement_nan_infinities_ties_and_signed_zero():
    w = np.array([[np.nan, 1.0, -np.inf, 1.0, np.inf, -0.0, 0.0],
                  [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]])
    indptr, ind, val = RA.csr(w, np.inf)
    np.testing.assert_array_equal(indptr, [0, 6, 6])          # a NaN is never inside, not even for +inf
    np.testing.assert_array_equal(ind, [2, 5, 6, 1, 3, 4])    # -inf first; -0.0 == +0.0 and 1.0 == 1.0 go by row; +inf <= +inf
    assert np.signbit(val[1]) and not np.signbit(val[2])      # the value is the entry's own
    indptr, ind, _ = RA.csr(w, 1.0)                           # the rule is <=: both ties are in
    np.testing.assert_array_equal(ind, [2, 5, 6, 1, 3])
    indptr, ind, _ = RA.csr(w, -np.inf)
    np.testing.assert_array_equal(ind, [2])
    indptr, ind, _ = RA.csr(w, -1.0, sort_results=False)
    np.testing.assert_array_equal(indptr, [0, 1, 1])


def test_radius_is_checked_on_the_host():
    """A bool or a non-number: TypeError; NaN: ValueError -- before the fit state is looked at, so also on an unfitted instance."""
    from kiez_amd import Kiez
    from kiez_amd import _native as N
    from kiez_amd.neighbors import NotFittedError
    assert N.radius_value(3) == 3.0 and N.radius_value(np.float32(-0.5)) == -0.5
    assert N.radius_value(float("inf")) == np.inf and N.radius_value(-np.inf) == -np.inf
    kz = Kiez(n_candidates=5, hubness="CSLS")
    calls = [kz.radius_neighbors, kz.radius_counts, kz.algorithm.radius_neighbors, kz.algorithm.radius_neighbors_device,
             kz.algorithm.radius_counts, kz.hubness.radius_neighbors, kz.hubness.radius_neighbors_device, kz.hubness.radius_counts,
             N.radius_value]
    for call in calls:
        for bad in (True, np.bool_(False), "1.0", None, 1 + 0j, [1.0]):
            with pytest.raises(TypeError, match="real number"):
                call(bad)
        for bad in (float("nan"), np.float64("nan"), np.float32("nan")):
            with pytest.raises(ValueError, match="NaN"):
                call(bad)
    for call in calls[:-1]:                        # a good radius gets as far as the fit state
        with pytest.raises(NotFittedError):
            call(0.5)
    for reduced in (False, True):
        with pytest.raises(NotFittedError):
            kz.radius_neighbors(-1.0, reduced=reduced, ragged=True)
    # the reduction is fitted source -> target only
    for call in (kz.hubness.radius_neighbors, kz.hubness.radius_neighbors_device, kz.hubness.radius_counts):
        with pytest.raises(ValueError, match="s_to_t=True"):
            call(0.5, s_to_t=False)


# ---- the helpers and the planted inputs of tests/test_gpu_radius_sort.py ----

def test_order_key_orders_like_the_doubles():
    """kz_knnr_key restated: keys ascend exactly as np.sort orders the values (NaN last, beside +inf), -0.0 and +0.0 share a key,
    NaN shares +inf's."""
    tiny = np.float64(5e-324)
    v = np.array([np.inf, np.nan, -np.inf, 0.0, -0.0, tiny, -tiny, 2.5e-310, -2.5e-310, 1.0, -1.0, 1e300, -1e300, 0.625, -3.0,
                  np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 2.2250738585072014e-308])
    key = RA.order_key(v)
    assert key.dtype == np.uint64 and key.shape == v.shape
    by_key = v[np.argsort(key, kind="stable")]                 # (NaN stands behind +inf in v: they share a key and go by place)
    np.testing.assert_array_equal(by_key, np.sort(v))          # (array_equal: NaN == NaN in place, -0.0 == +0.0)
    finite = v[~np.isnan(v)]
    fk = RA.order_key(finite)
    assert ((fk[:, None] < fk[None, :]) == (finite[:, None] < finite[None, :])).all()
    assert ((fk[:, None] == fk[None, :]) == (finite[:, None] == finite[None, :])).all()
    assert RA.order_key([np.nan])[0] == RA.order_key([np.inf])[0] == 0xFFF0000000000000
    assert RA.order_key([-0.0])[0] == RA.order_key([0.0])[0] == 0x8000000000000000
    assert RA.order_key([-np.inf])[0] == 0x000FFFFFFFFFFFFF and RA.order_key([1.0])[0] == 0xBFF0000000000000


def test_byte_values_and_radix_passes():
    rng = np.random.default_rng(0)
    assert RA.radix_passes([0.625] * 50) == [] and RA.radix_passes([-0.0, 0.0]) == []
    assert RA.radix_passes([1.0, -1.0]) == list(range(0, 64, 8))
    for shifts in RA.BYTE_REGIMES:
        v = RA.byte_values(rng, 9000, shifts)
        assert v.dtype == np.float64 and np.isfinite(v).all() and (v >= 0).all() and not np.signbit(v).any()
        assert RA.radix_passes(v) == list(shifts)
        for s in shifts:                                    # every digit value of the byte occurs
            assert len(np.unique((RA.order_key(v) >> np.uint64(s)) & np.uint64(0xFF))) == (0x40 if s == 56 else 256)


@pytest.mark.parametrize("regime", RA.REGIMES, ids=RA.regime_id)
def test_planted_matrix_has_the_lengths_and_the_passes_of_its_regime(regime):
    assert sorted(RA.LENGTHS)[0] == 0 and max(RA.LENGTHS) == RA.PLANT_N_INDEX and len(RA.LENGTHS) == 24
    for edge in (2, 256, 512, 1024, 2048, 4096):             # both sides of every size the sort branches at
        assert {edge - 1, edge, edge + 1} <= set(RA.LENGTHS) | {1, 3}
    assert {n % 256 for n in RA.LENGTHS if n > RA.SORT_LDS} >= {0, 1, 255}          # the radix path's last tile
    for dtype in (np.float64, np.float32):
        D, radius = RA.planted(regime, dtype)
        assert D.dtype == dtype and D.shape == (24, 9000) and np.isfinite(D).all() and (D >= 0).all()
        np.testing.assert_array_equal((D <= radius).sum(axis=1), RA.LENGTHS)
        assert (D[D > radius] >= 1e30).all() and radius <= 2.0
        indptr, ind, val = RA.csr(D, radius)
        np.testing.assert_array_equal(np.diff(indptr), RA.LENGTHS)
        assert (np.diff(RA.csr(D.T, radius)[0]) <= 24).all()
    D, radius = RA.planted(regime)
    for n, row in zip(RA.LENGTHS, D):
        if n > RA.SORT_LDS:
            passes = RA.radix_passes(row[row <= radius])
            if n == 9000 or regime != "distinct":
                assert passes == RA.REGIME_PASSES[regime], (n, passes)
            else:                                               # (a shorter row need not reach below 2^-15, the top byte's edge)
                assert passes[:7] == RA.REGIME_PASSES[regime], (n, passes)
    assert len(RA.REGIME_PASSES["distinct"]) % 2 == 1           # an odd number of passes: the copy back
    if regime == "grid8":
        zeros = D[D == 0.0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
        assert len(np.unique(D[D <= radius])) == 9 and radius == 1.0
    if regime == "distinct":
        assert len(np.unique(D[D <= radius])) == sum(RA.LENGTHS)


def test_signed_case_is_exact_and_has_the_row_lengths_of_both_sort_paths():
    D, q_a, t_a, w = RA.signed_case()
    assert np.isfinite(D).all() and (D >= 0).all() and D.shape == (6, 9000)
    # exact: every term is a multiple of 1 / 128 below 2^4, so the differences round nowhere and any order gives the same bits
    ok = np.isfinite(w)
    assert (w[ok] * 128 == np.round(w[ok] * 128)).all() and np.abs(w[ok]).max() < 16
    assert np.isnan(w[:, list(RA.SIGNED_NAN)]).all() and np.isnan(w).sum() == 6 * 3
    assert (w[:, list(RA.SIGNED_TO_MINUS_INF)] == -np.inf).all() and (w[:, list(RA.SIGNED_TO_PLUS_INF)] == np.inf).all()
    assert (w[ok] == 0).any() and (w[ok] < 0).any() and (w[ok] > 0).any()
    bounds = {np.inf: (8997, 8997), 0.0: (RA.SORT_LDS + 1, 9000), -3.0: (1025, 2048), -4.5: (65, 512), -np.inf: (2, 2)}
    for radius in RA.SIGNED_RADII:
        counts = np.diff(RA.csr(w, radius)[0])
        print("radius", radius, "rows of", counts.min(), "to", counts.max())
        lo, hi = bounds[radius]
        assert lo <= counts.min() and counts.max() <= hi
    assert RA.radix_passes(w[0][w[0] <= np.inf]) == list(range(0, 64, 8))       # -inf .. +inf: all eight passes


def test_carry_case():
    D, radius = RA.carry_case()
    assert D.dtype == np.float32 and D.shape == (2, 256 * 8192 + 1) and np.isfinite(D).all() and (D >= 0).all()
    indptr, ind, val = RA.csr(D, radius, sort_results=False)
    np.testing.assert_array_equal(indptr, [0, 8, 8 + 5001])
    np.testing.assert_array_equal(ind[:8], RA.CARRY_ROW0)
    assert ind[-1] == 256 * 8192 and val[-1] == 0.0 and ind[7] // 8192 == 256 and ind[5] // 8192 == ind[6] // 8192 == 255
    assert RA.csr(D, radius)[1][8] == 256 * 8192                # sorted: the entry of the last chunk comes first in row 1
    np.testing.assert_array_equal(RA.csr(D, radius)[1][:8], RA.CARRY_ROW0[::-1])
