"""tests/hubness_restate.py against numpy and the oracle on the host (no GPU): the summation tree, the NaN forms of mean and
standard deviation, the per-row MutualProximity empiric restatement and the exact DisSimLocal references the GPU tests
(tests/test_gpu_hubness_kernels.py) compare the device with."""
from fractions import Fraction

import numpy as np
import pytest

from tests import hubness_restate as R

# every branch of the tree: sequential (< 8), eight accumulators with and without a tail, the first split (129), halves that are
# (not) multiples of 8 (136 / 137, 272 / 273), two levels of splits (257 ... 4096)
K_LIST = [1, 2, 7, 8, 9, 16, 17, 127, 128, 129, 136, 137, 255, 256, 257, 272, 273, 1000, 1024, 1025, 4095, 4096]


def _bits(a):
    """The bit patterns, every NaN as one value (sign and payload of a NaN are not part of any contract)."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


@pytest.mark.parametrize("K", K_LIST)
def test_the_tree_is_numpys(K):
    """C-contiguous float64 rows: ndarray.mean / std and the nan forms reduce every row with DOUBLE_pairwise_sum."""
    rng = np.random.default_rng(K)
    for scale in (1e-3, 1.0, 1e3):
        a = np.ascontiguousarray(rng.random((4, K)) * scale)
        assert np.array_equal(_bits(R.rows(R.pairwise_sum, a)), _bits(a.sum(axis=1)))
        assert np.array_equal(_bits(R.rows(R.mean, a)), _bits(a.mean(axis=1)))
        assert np.array_equal(_bits(R.rows(R.std, a)), _bits(a.std(axis=1)))
        assert np.array_equal(_bits(R.rows(R.nanmean, a)), _bits(np.nanmean(a, axis=1)))
        assert np.array_equal(_bits(R.rows(R.nanstd, a)), _bits(np.nanstd(a, axis=1)))


@pytest.mark.parametrize("K", K_LIST)
def test_the_nan_forms_are_numpys(K):
    """NaN at the tail (what a candidate list looks like), NaN scattered, a row of NaN only, a row without."""
    rng = np.random.default_rng(1000 + K)
    for scale in (1e-3, 1.0, 1e3):
        a = np.ascontiguousarray(rng.random((5, K)) * scale)
        a[0, K - min(K, 3):] = np.nan                      # (K <= 3: the whole row)
        a[1, rng.random(K) < 0.3] = np.nan
        a[2, :] = np.nan
        a[3, K - 1] = np.nan
        with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
            want_m, want_s = np.nanmean(a, axis=1), np.nanstd(a, axis=1)
        got_m, got_s = R.rows(R.nanmean, a), R.rows(R.nanstd, a)
        assert np.array_equal(_bits(got_m), _bits(want_m)), (got_m, want_m)
        assert np.array_equal(_bits(got_s), _bits(want_s)), (got_s, want_s)
        assert np.isnan(got_m[2]) and np.isnan(got_s[2]) and np.isfinite(got_m[4]) and np.isfinite(got_s[4])
        # the plain mean propagates the NaN the nan form skips
        assert np.isnan(R.mean(a[3])) and (K == 1 or np.isfinite(R.nanmean(a[3])))


def _mp_case(rng, n, K, n_t, Kt, grid):
    ind = np.stack([rng.choice(n_t, K, replace=False) for _ in range(n)]).astype(np.int64)
    dist = np.sort(np.round(rng.random((n, K)) * grid) / grid, axis=1)
    ind_t2s = np.stack([rng.choice(2 * n_t, Kt, replace=False) for _ in range(n_t)]).astype(np.int64)
    dist_t2s = np.sort(np.round(rng.random((n_t, Kt)) * grid) / grid, axis=1)
    return dist, ind, dist_t2s, ind_t2s


@pytest.mark.parametrize("n,K,n_t,Kt,grid", [(7, 1, 5, 1, 4), (6, 5, 9, 3, 4), (5, 17, 30, 17, 8), (4, 60, 70, 60, 16), (4, 33, 64, 60, 2),
                                             (3, 60, 61, 7, 1000)])
def test_mp_empiric_rows_is_the_oracles(n, K, n_t, Kt, grid):
    """Distances on a coarse grid (the strict `>` meets equality in most rows); half of the reverse-list ids are no candidate id of
    anybody, some are negative or beyond 2^32."""
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(n * 100 + K)
    dist, ind, dist_t2s, ind_t2s = _mp_case(rng, n, K, n_t, Kt, grid)
    ind_t2s[0, 0] = -1 - int(ind[0, 0])
    ind_t2s[n_t - 1, Kt - 1] = (1 << 32) + int(ind[0, 0])
    got = R.mp_empiric_rows(dist, ind, dist_t2s, ind_t2s)
    assert np.array_equal(got, O.mp_empiric_transform(dist, ind, dist_t2s, ind_t2s))
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_mp_empiric_rows_without_any_match():
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(3)
    dist, ind, dist_t2s, ind_t2s = _mp_case(rng, 5, 20, 40, 12, 8)
    ind_t2s += 1000                                            # no reverse-list id is a candidate id: every T is the fill value
    got = R.mp_empiric_rows(dist, ind, dist_t2s, ind_t2s)
    assert np.array_equal(got, O.mp_empiric_transform(dist, ind, dist_t2s, ind_t2s))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("centre,spread", [(0.0, 1.0), (100.0, 0.01)])
def test_exact_dissimlocal_brackets_the_float64_oracle(dtype, centre, spread):
    """The Fraction references against the oracle's float64 evaluation: inside the derived bound, and the bound is small against
    the values' own scale (it is a rounding bound, not a tolerance)."""
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(11)
    n_s, n_t, d, Kt, K = 30, 25, 65, 5, 4
    src = (centre + spread * rng.standard_normal((n_s, d))).astype(dtype)
    tgt = (centre + spread * rng.standard_normal((n_t, d))).astype(dtype)
    ind_t2s = np.stack([rng.choice(n_s, Kt, replace=False) for _ in range(n_t)]).astype(np.int64)
    exact = R.dsl_fit_exact(ind_t2s, src, tgt)
    bound = R.dsl_fit_bound(ind_t2s, src, tgt)
    got = O.dsl_fit(ind_t2s, src.astype(np.float64), tgt.astype(np.float64))
    for j in range(n_t):
        assert abs(Fraction(float(got[j])) - exact[j]) <= bound[j], (j, float(got[j]), float(exact[j]), float(bound[j]))
        assert bound[j] <= Fraction(1, 10 ** 12) * max(exact[j], Fraction(centre * centre * d))    # a rounding bound, not a tolerance
    ind = np.stack([rng.choice(n_t, K, replace=False) for _ in range(6)]).astype(np.int64)
    # (the float64 evaluation before the global shift: the CPU engine's restatement of dis_sim.py:153-166, the oracle's lines)
    import torch
    from tests.cpu_engine import OracleEngine, _Mat
    ex = R.dsl_transform_exact(ind, src[2:8], tgt, got)
    bd = R.dsl_transform_bound(ind, src[2:8], tgt, got)
    want, _ = OracleEngine().dsl_transform(torch.from_numpy(ind), _Mat(torch.from_numpy(src), "sqeuclidean"), 2,
                                           _Mat(torch.from_numpy(tgt), "sqeuclidean"), torch.from_numpy(got))
    want = want.numpy()
    for i in range(6):
        for m in range(K):
            assert abs(Fraction(float(want[i, m])) - ex[i][m]) <= bd[i][m], (i, m, float(want[i, m]), float(ex[i][m]), float(bd[i][m]))
