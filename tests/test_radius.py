"""The numpy restatement of the radius calls (tests/radius_restate.py) against scikit-learn's
NearestNeighbors(algorithm="brute").radius_neighbors(sort_results=True), and the argument errors the new methods raise on the host
before any device call.  No GPU."""
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
