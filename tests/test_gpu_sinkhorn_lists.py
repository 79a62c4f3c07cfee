"""Sinkhorn and the inverted softmax on the candidate lists on the device (kz_softmin_lists.hip): the transposition against numpy,
exactly; the row and the column soft-min against the numpy restatement (tests/sinkhorn_lists_restate.py) at every k branch, around
the chunk size and with every special value; the summation-order rule; kz_sinkhorn_lists against the same iteration composed from
its step calls; the fitted classes with support="candidates" against the restatement and through every inherited call.
`pytest -m gpu`.

Brackets (tests/test_gpu_sinkhorn.py's).  One soft-min: |got - want| <= 1e-12 (|want| + eps) = SR.bracket.  Potentials after L
iterations: 2 L times that -- the soft-min is 1-Lipschitz in the sup norm on a restricted support too, so the errors add and do not
grow.  Special values (NaN = no pair, +-inf) are compared exactly."""
import math
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import sinkhorn_lists_restate as LR
from tests import sinkhorn_restate as SR
from tests.test_gpu_sinkhorn import FIT_CASES, _distances, _matrices

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
INT_MAX = np.iinfo(np.int32).max
EPS = (1e-3, 0.05, 1.0, 50.0)


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _assert_in_bracket(got, want, eps, where, factor=1):
    """Non-finite restated values (NaN: no pair; +-inf) exactly, the others within factor x SR.bracket.  -> worst share of the bracket"""
    assert got.shape == want.shape and got.dtype == np.float64, where
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite], err_msg=where)
    err = np.abs(got[finite] - want[finite])
    bound = factor * SR.bracket(want[finite], eps)
    worst = float((err / bound).max()) if err.size else 0.0
    assert (err <= bound).all(), f"{where}: {worst:.3g} of the bracket"
    return worst


def _random_lists(rng, n_q, k, n_index, plain=False):
    """Lists with ids in [0, n_index); unless `plain`: rows with -1, INT_MAX and n_index as ids, a target repeated inside a row, one
    column listed by every row, and (n_index > 2) column 1 empty."""
    ind = rng.integers(0, n_index, (n_q, k)).astype(np.int64)
    dist = rng.standard_normal((n_q, k))
    if plain:
        return dist, ind
    if n_index > 2:
        ind[ind == 1] = 2
    ind[:, 0] = 0
    for row, bad in zip(rng.permutation(n_q)[:3], (-1, INT_MAX, n_index)):
        ind[row, rng.integers(0, k)] = bad
    if k >= 3:
        ind[n_q // 2, 1:3] = n_index - 1
    return dist, ind


# ---- the transposition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_index", [1, 7, 257, 70_000])
def test_transposition_is_numpys_stable_sort(ctx, n_index):
    """(n_index = 70 000 puts a third radix digit in play; 300 x 130 entries are 20 sort tiles.)"""
    from kiez_amd import _native as N
    for n_q in (1, 63, 300):
        for k in (1, 5, 64, 65, 130):
            rng = np.random.default_rng(1000 * n_q + k)
            dist, ind = _random_lists(rng, n_q, k, n_index)
            view = N.lists_transpose(ctx, ctx.to_device(dist), ctx.to_device(ind), n_index)
            colptr, col_row, col_val = LR.transpose(dist, ind, n_index)
            where = f"n_q={n_q} k={k} n_index={n_index}"
            assert view.nnz == colptr[-1] == LR.pairs(ind, n_index).sum(), where
            assert view.colptr.dtype == np.int64 and view.col_row.dtype == np.int32 and view.col_val.dtype == np.float64
            np.testing.assert_array_equal(view.colptr.numpy(), colptr, err_msg=where)
            np.testing.assert_array_equal(view.col_row.numpy()[:view.nnz], col_row, err_msg=where)
            np.testing.assert_array_equal(_bits(view.col_val.numpy()[:view.nnz]), _bits(col_val), err_msg=where)
            if n_q >= 63:
                assert colptr[1] - colptr[0] >= n_q - 3, where             # (column 0: listed by every row)
            if n_index > 2:
                assert colptr[2] == colptr[1], where                       # (an empty column)
    # a row of nothing but padding, and no rows at all
    ind = np.array([[-1, INT_MAX, n_index]], dtype=np.int64)
    view = N.lists_transpose(ctx, ctx.to_device(np.zeros((1, 3))), ctx.to_device(ind), n_index)
    assert view.nnz == 0 and not view.colptr.numpy().any()
    view = N.lists_transpose(ctx, ctx.empty((0, 3), np.float64), ctx.empty((0, 3), np.int64), n_index)
    assert view.nnz == 0 and not view.colptr.numpy().any()


# ---- the two soft-mins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 129, 4096])
def test_row_and_column_softmin_against_the_restatement(ctx, k):
    from kiez_amd import _native as N
    n_index = 97
    worst = 0.0
    for n_q in (1, 63, 64, 65, 257):
        rng = np.random.default_rng(100 * k + n_q)
        dist, ind = _random_lists(rng, n_q, k, n_index)
        if n_q >= 63:
            dist[5, 0], dist[6, k - 1] = np.nan, np.inf                   # (ignored entries)
            ind[7] = -1                                                   # a row without a pair
            dist[8, 0], ind[8, 0] = -np.inf, 0                            # a -inf entry: row 8 and column 0
            dist[9], ind[9] = np.inf, np.arange(k) % 5 + 10               # a row of +inf only
        off_t, off_q = 0.5 * rng.standard_normal(n_index), 0.5 * rng.standard_normal(n_q)
        d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
        offt_dev, offq_dev = ctx.to_device(off_t), ctx.to_device(off_q)
        view = N.lists_transpose(ctx, d_dev, i_dev, n_index)
        csc = LR.transpose(dist, ind, n_index)
        for eps in EPS:
            for with_off, shift in ((False, 0.75), (True, -1.25), (True, 0.0)):
                where = f"k={k} n_q={n_q} eps={eps} off={with_off} shift={shift}"
                got = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=offt_dev if with_off else None, shift=shift).numpy()
                want = LR.softmin_rows(dist, ind, n_index, eps, off=off_t if with_off else None, shift=shift)
                worst = max(worst, _assert_in_bracket(got, want, eps, "rows " + where))
                if n_q >= 63:
                    assert np.isnan(got[7]) and got[8] == -np.inf and got[9] == np.inf, where
                    assert np.isnan(got).sum() == (~LR.pairs(ind, n_index).any(axis=1)).sum() <= 4, where
                got = N.softmin_list_cols(ctx, view, eps, off=offq_dev if with_off else None, shift=shift).numpy()
                want = LR.softmin_cols(*csc, eps, off=off_q if with_off else None, shift=shift)
                worst = max(worst, _assert_in_bracket(got, want, eps, "columns " + where))
                assert np.isnan(got[1]), where                            # (the empty column)
                if n_q >= 63:
                    assert got[0] == -np.inf, where
    print(f"k={k}: worst error {worst:.2e} of the bracket")


def _hub_lists(rng, n_q, n_index=40):
    """k = 2, every row lists column 0: a column of n_q entries."""
    ind = np.stack([np.zeros(n_q, dtype=np.int64), rng.integers(1, n_index, n_q)], axis=1)
    return rng.standard_normal((n_q, 2)), ind


def test_columns_around_the_chunk_size(ctx):
    from kiez_amd import _native as N
    C = N.SOFTMIN_LIST_CHUNK
    n_index = 40
    for n_q in (C - 1, C, C + 1, 2 * C + 1, 64 * C + 3):                  # (the last: more parts than the folding wave has lanes)
        rng = np.random.default_rng(n_q)
        dist, ind = _hub_lists(rng, n_q, n_index)
        dist[3, 0], dist[n_q - 1, 0] = np.nan, np.inf
        off = 0.5 * rng.standard_normal(n_q)
        off_dev = ctx.to_device(off)
        view = N.lists_transpose(ctx, ctx.to_device(dist), ctx.to_device(ind), n_index)
        csc = LR.transpose(dist, ind, n_index)
        assert csc[0][1] == n_q == view.colptr.numpy()[1]
        for eps in EPS:
            for o, shift in ((None, 0.75), (off, -1.25)):
                got = N.softmin_list_cols(ctx, view, eps, off=None if o is None else off_dev, shift=shift).numpy()
                worst = _assert_in_bracket(got, LR.softmin_cols(*csc, eps, off=o, shift=shift), eps, f"column of {n_q} eps={eps}")
                assert np.isfinite(got).all()
        print(f"column of {n_q} entries: worst error {worst:.2e} of the bracket")
    # special values in a long column: a chunk of +inf only beside finite ones; everything +inf; a -inf in the last chunk
    n_q = 2 * C + 1
    dist, ind = _hub_lists(np.random.default_rng(2), n_q, n_index)
    csc = LR.transpose(dist, ind, n_index)
    i_dev = ctx.to_device(ind)
    for lo, hi, value, want0 in ((0, C, np.inf, None), (0, n_q, np.inf, np.inf + 2.0), (n_q - 1, n_q, -np.inf, -np.inf)):
        d = dist.copy()
        d[lo:hi, 0] = value
        got = N.softmin_list_cols(ctx, N.lists_transpose(ctx, ctx.to_device(d), i_dev, n_index), 0.05, shift=2.0).numpy()
        want = LR.softmin_cols(*LR.transpose(d, ind, n_index), 0.05, shift=2.0)
        _assert_in_bracket(got, want, 0.05, f"long column with {value} in [{lo}, {hi})")
        assert want0 is None or got[0] == want0


def test_far_from_unit_scale(ctx):
    """Values 1000 +- 40, eps = 0.02: exp(-d / eps) underflows for every entry -- without the minimum taken out the result is +inf."""
    from kiez_amd import _native as N
    C = N.SOFTMIN_LIST_CHUNK
    rng = np.random.default_rng(1000)
    n_q, n_index, eps = C + 9, 40, 0.02
    for k, (dist, ind) in ((2, _hub_lists(rng, n_q, n_index)), (70, _random_lists(rng, n_q, 70, n_index, plain=True))):
        dist = 1000.0 + 40.0 * dist
        with np.errstate(divide="ignore"):
            assert np.isinf(-eps * np.log(np.exp(-dist / eps).sum(axis=1))).all()
        d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
        view = N.lists_transpose(ctx, d_dev, i_dev, n_index)
        for off_t, off_q in ((None, None), (1000.0 + 40.0 * rng.standard_normal(n_index), 1000.0 + 40.0 * rng.standard_normal(n_q))):
            got = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=None if off_t is None else ctx.to_device(off_t), shift=3.0).numpy()
            assert np.isfinite(got).all()
            _assert_in_bracket(got, LR.softmin_rows(dist, ind, n_index, eps, off=off_t, shift=3.0), eps, f"far rows k={k}")
            got = N.softmin_list_cols(ctx, view, eps, off=None if off_q is None else ctx.to_device(off_q), shift=3.0).numpy()
            assert np.isfinite(got).all()
            _assert_in_bracket(got, LR.softmin_cols(*LR.transpose(dist, ind, n_index), eps, off=off_q, shift=3.0), eps, f"far columns k={k}")


def test_special_offsets_and_errors_at_the_abi(ctx):
    from kiez_amd import _native as N
    rng = np.random.default_rng(7)
    n_q, k, n_index, eps = 70, 5, 30, 0.05
    dist, ind = _random_lists(rng, n_q, k, n_index, plain=True)
    d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
    view = N.lists_transpose(ctx, d_dev, i_dev, n_index)
    # a NaN offset: the entry is ignored; all offsets -inf: every term +inf; one offset +inf: a -inf term
    off = 0.1 * rng.standard_normal(n_index)
    off[ind[0, 0]] = np.nan
    keep = ~np.isnan(off[ind])
    want = LR.softmin_rows(np.where(keep, dist, np.inf), ind, n_index, eps, off=np.nan_to_num(off), shift=2.0)
    _assert_in_bracket(N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=ctx.to_device(off), shift=2.0).numpy(), want, eps, "NaN offset")
    got = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=ctx.to_device(np.full(n_index, -np.inf)), shift=2.0).numpy()
    np.testing.assert_array_equal(got, np.full(n_q, np.inf))
    off = np.zeros(n_q)
    off[11] = np.inf
    got = N.softmin_list_cols(ctx, view, eps, off=ctx.to_device(off)).numpy()
    np.testing.assert_array_equal(got == -np.inf, np.isin(np.arange(n_index), ind[11]))
    # what the calls refuse
    for bad in (0.0, -0.05, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="eps"):
            N.softmin_list_rows(ctx, d_dev, i_dev, n_index, bad)
        with pytest.raises(ValueError, match="eps"):
            N.softmin_list_cols(ctx, view, bad)
        with pytest.raises(ValueError, match="eps"):
            N.sinkhorn_lists(ctx, d_dev, i_dev, n_index, bad, 3)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="shift"):
            N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, shift=bad)
        with pytest.raises(ValueError, match="shift"):
            N.softmin_list_cols(ctx, view, eps, shift=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_iter"):
            N.sinkhorn_lists(ctx, d_dev, i_dev, n_index, eps, bad)
    with pytest.raises(ValueError, match="n_index"):
        N.softmin_list_rows(ctx, d_dev, i_dev, 0, eps)
    wide = ctx.empty((2, 4097), np.float64), ctx.empty((2, 4097), np.int64)
    for call in (lambda: N.lists_transpose(ctx, *wide, n_index), lambda: N.softmin_list_rows(ctx, *wide, n_index, eps),
                 lambda: N.sinkhorn_lists(ctx, *wide, n_index, eps, 2)):
        with pytest.raises(ValueError, match="k = 4097"):
            call()
    lib, h = ctx.lib, ctx.handle
    assert lib.kz_softmin_list_rows(h, d_dev.ptr, i_dev.ptr, 2 ** 29, 4, n_index, eps, None, 0.0, d_dev.ptr) == 1   # (2^31 entries)
    assert b"entries" in lib.kz_last_error()
    assert lib.kz_softmin_list_rows(h, None, i_dev.ptr, n_q, k, n_index, eps, None, 0.0, d_dev.ptr) == 1
    assert b"null" in lib.kz_last_error()
    assert lib.kz_sinkhorn_lists(h, d_dev.ptr, i_dev.ptr, n_q, k, n_index, eps, 2, -1.0, None, None, None, None, None) == 1
    assert b"null" in lib.kz_last_error()
    assert lib.kz_lists_transpose(h, d_dev.ptr, i_dev.ptr, n_q, k, n_index, None, None, None, None) == 1
    assert lib.kz_softmin_list_cols(h, None, None, None, n_index, 0, eps, None, 0.0, d_dev.ptr) == 1
    with pytest.raises(ValueError, match="float64"):
        N.softmin_list_rows(ctx, ctx.to_device(dist.astype(np.float32)), i_dev, n_index, eps)
    with pytest.raises(ValueError, match="off"):
        N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=ctx.to_device(np.zeros(n_index - 1)))
    with pytest.raises(ValueError, match="off"):
        N.softmin_list_cols(ctx, view, eps, off=ctx.to_device(np.zeros(n_q + 1)))
    # no rows: nothing to do
    none = ctx.empty((0, k), np.float64), ctx.empty((0, k), np.int64)
    assert N.softmin_list_rows(ctx, *none, n_index, eps).shape == (0,)
    assert N.sinkhorn_lists(ctx, *none, n_index, eps, 3)[2:] == (0, None)


# ---- the order rule ---------------------------------------------------------------------------------------------------------------
def test_the_summation_order_is_a_function_of_the_row_or_column_alone(ctx):
    from kiez_amd import _native as N
    C = N.SOFTMIN_LIST_CHUNK
    rng = np.random.default_rng(70)
    n_index, eps = 100, 0.05
    for k in (3, 70):
        n_q = 2 * C + 77
        # the base rows list the columns 50 .. 99, column 50 by every row (a long column); the appended rows list 0 .. 49: every
        # base column moves to another place of the view, by a count that is no multiple of the chunk
        ind = rng.integers(51, n_index, (n_q, k)).astype(np.int64)
        ind[:, 0] = 50
        dist = rng.standard_normal((n_q, k))
        more_ind = rng.integers(0, 50, (301, k)).astype(np.int64)
        more_dist = rng.standard_normal((301, k))
        off_t, off_q = ctx.to_device(0.3 * rng.standard_normal(n_index)), 0.3 * rng.standard_normal(n_q + 301)
        d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
        # rows: two runs; a slice of the rows (an odd start: other places in the wave, another workgroup)
        whole = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=off_t, shift=0.5).numpy()
        again = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=off_t, shift=0.5).numpy()
        part = N.softmin_list_rows(ctx, d_dev.view_rows(299, 401), i_dev.view_rows(299, 401), n_index, eps, off=off_t, shift=0.5).numpy()
        assert np.isfinite(whole).all()
        np.testing.assert_array_equal(_bits(again), _bits(whole))
        np.testing.assert_array_equal(_bits(part), _bits(whole[299:700]))
        # columns: two runs (each with its own transposition); rows appended that list other columns
        base = N.softmin_list_cols(ctx, N.lists_transpose(ctx, d_dev, i_dev, n_index), eps, off=ctx.to_device(off_q[:n_q]), shift=0.5).numpy()
        again = N.softmin_list_cols(ctx, N.lists_transpose(ctx, d_dev, i_dev, n_index), eps, off=ctx.to_device(off_q[:n_q]), shift=0.5).numpy()
        both = N.lists_transpose(ctx, ctx.to_device(np.concatenate([dist, more_dist])), ctx.to_device(np.concatenate([ind, more_ind])), n_index)
        assert both.colptr.numpy()[50] == 301 * k and both.colptr.numpy()[51] - both.colptr.numpy()[50] == n_q > 2 * C
        longer = N.softmin_list_cols(ctx, both, eps, off=ctx.to_device(off_q), shift=0.5).numpy()
        assert np.isfinite(base[50:]).all() and np.isnan(base[:50]).all() and np.isfinite(longer).all()
        np.testing.assert_array_equal(_bits(again), _bits(base))
        np.testing.assert_array_equal(_bits(longer[50:]), _bits(base[50:]))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def _composed(ctx, d_dev, i_dev, n_index, eps, n_iter, tol=None):
    """Sinkhorn._potentials' loop over the two step calls and kz_max_abs_diff -> (f, g, iterations, change), f and g as numpy."""
    from kiez_amd import _native as N
    view = N.lists_transpose(ctx, d_dev, i_dev, n_index)
    shift = eps * math.log(d_dev.shape[0] / n_index)
    f = g = change = None
    for it in range(1, n_iter + 1):
        g_new = N.softmin_list_cols(ctx, view, eps, off=f, shift=shift)
        if g is not None:
            change = N.max_abs_diff(ctx, g_new, g)
        g = g_new
        f = N.softmin_list_rows(ctx, d_dev, i_dev, n_index, eps, off=g)
        if tol is not None and change is not None and change <= tol:
            break
    return f.numpy(), g.numpy(), it, change


def _device_lists(ctx, s, t, K):
    from kiez_amd import _native as N
    sm, tm = _matrices(ctx, s, t, "cosine")
    dist, ind, _ = N.knn(ctx, sm, tm, K)
    return dist, ind


def test_the_loop_is_the_composition_of_its_steps(ctx):
    from kiez_amd import _native as N
    for (n_s, n_t, eps, L, noise), K in ((FIT_CASES[0], 10), (FIT_CASES[1], 5)):
        s, t, _ = SR.alignment_case(n_s, n_t, noise)
        d_dev, i_dev = _device_lists(ctx, s, t, K)
        for n_iter in (1, 2, 7):
            f, g, done, change = N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, n_iter)
            f_want, g_want, done_want, change_want = _composed(ctx, d_dev, i_dev, n_t, eps, n_iter)
            assert done == done_want == n_iter and change == change_want and (change is None) == (n_iter == 1)
            np.testing.assert_array_equal(_bits(f.numpy()), _bits(f_want))
            np.testing.assert_array_equal(_bits(g.numpy()), _bits(g_want))
            assert np.isnan(g_want).sum() == (0 if K == 10 else np.setdiff1d(np.arange(n_t), i_dev.numpy()).size)


def test_the_loop_stops_on_the_device_where_the_class_would(ctx):
    """(200, 200, eps 0.1), K = 10, tol = 1e-3: the numpy restatement stops at iteration 40 (tests/test_sinkhorn_lists.py), the
    change at 39 still 5e-6 above the tolerance."""
    from kiez_amd import _native as N
    n_s, n_t, eps, L, noise = FIT_CASES[0]
    s, t, _ = SR.alignment_case(n_s, n_t, noise)
    d_dev, i_dev = _device_lists(ctx, s, t, 10)
    f, g, n, change = N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, L, tol=1e-3)
    assert n == 40 and change <= 1e-3
    f_want, g_want, n_want, change_want = _composed(ctx, d_dev, i_dev, n_t, eps, L, tol=1e-3)
    assert n == n_want and change == change_want
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(f_want))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(g_want))
    # the change is kz_max_abs_diff of the last two column steps, and the stop was the first one possible
    f_b, g_b, n_b, change_b = N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, n - 1)
    f_s, g_s, n_s_, change_s = N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, n)
    assert n_b == n - 1 and n_s_ == n
    assert change == N.max_abs_diff(ctx, g_s, g_b) == change_s == np.abs(g_s.numpy() - g_b.numpy()).max()
    assert change_b > 1e-3
    # the row step behind the last column step was taken: the state is that of n whole iterations
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(f_s.numpy()))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(g_s.numpy()))
    # a tolerance met at once stops at 2 (the first measured change); a single iteration measures none; tol = 0 is allowed
    assert N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, L, tol=1e9)[2] == 2
    assert N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, 1, tol=1e-3)[2:] == (1, None)
    assert N.sinkhorn_lists(ctx, d_dev, i_dev, n_t, eps, 3, tol=0.0)[2] == 3


# ---- the fitted classes -------------------------------------------------------------------------------------------------------------
LIST_FIT_CASES = [(FIT_CASES[0], 10), (FIT_CASES[1], 10), (FIT_CASES[2], 10), (FIT_CASES[1], 5)]
LIST_FIT_IDS = [f"{c[0]}x{c[1]}_eps{c[2]}_K{K}" for c, K in LIST_FIT_CASES]


def _kiez(hubness, K, metric="cosine", **kw):
    from kiez_amd import Kiez
    return Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=kw)


@pytest.fixture(scope="module")
def list_fits():
    """Per case: the data, the device's own distances of all pairs, the fitted instance's own lists, its potentials and the
    restatement's over those lists, and the searches `fit` + `kneighbors(5)` ran -- once; read-only."""
    from kiez_amd import Sinkhorn
    from kiez_amd import _native as N
    ctx = N.Context.get()
    out = {}
    for case, K in LIST_FIT_CASES:
        n_s, n_t, eps, L, noise = case
        s, t, gold = SR.alignment_case(n_s, n_t, noise)
        D = _distances(ctx, *_matrices(ctx, s, t, "cosine"), "cosine")
        searches = []
        real_knn = N.knn

        def counted(*a, **k):
            searches.append(a[3])
            return real_knn(*a, **k)
        N.knn = counted
        try:
            kz = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, support="candidates").fit(s, t)
            cached_k, cd_dev, ci_dev = kz.algorithm._forward           # (the lists are left in the backend's one-shot cache)
            cd, ci = cd_dev.numpy(), ci_dev.numpy()
            d5, i5 = kz.kneighbors(5)
        finally:
            N.knn = real_knn
        f_want, g_want, _, _ = LR.sinkhorn_potentials(cd, ci, n_t, eps, L)
        hub = kz.hubness
        res = dict(s=s, t=t, gold=gold, D=D, cd=cd, ci=ci, d5=d5, i5=i5, f=hub.source_potential_, g=hub.target_potential_, f_want=f_want,
                   g_want=g_want, searches=tuple(searches), cached_k=cached_k, n_iter_=hub.n_iter_, change=hub.potential_change_)
        for a in res.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(case, K)] = (kz, res)
    return out


@pytest.mark.parametrize("case,K", LIST_FIT_CASES, ids=LIST_FIT_IDS)
def test_fit_on_the_candidate_lists(list_fits, case, K):
    from kiez_amd import matching
    n_s, n_t, eps, L, noise = case
    kz, r = list_fits[(case, K)]
    f, g, cd, ci, D = r["f"], r["g"], r["cd"], r["ci"], r["D"]
    # ONE search for fit + kneighbors, over the device's own distances
    assert r["searches"] == (K,) and r["cached_k"] == K
    assert cd.shape == ci.shape == (n_s, K) and cd.dtype == np.float64 and ci.dtype == np.int64
    np.testing.assert_array_equal(cd, np.take_along_axis(D, ci, axis=1))
    np.testing.assert_array_equal(ci, LR.candidate_lists(D, K)[1])
    assert r["n_iter_"] == L and r["change"] is not None and f.shape == (n_s,) and g.shape == (n_t,) and f.dtype == g.dtype == np.float64
    # the potentials: the restatement's, NaN exactly where no row lists the target
    unlisted = np.setdiff1d(np.arange(n_t), ci)
    if (case, K) == LIST_FIT_CASES[3]:
        print("unlisted targets:", unlisted.size)
        assert unlisted.size >= 1                                      # (7 on the CPU)
    np.testing.assert_array_equal(np.nonzero(np.isnan(g))[0], unlisted)
    assert not np.isnan(f).any()
    print("worst error of f:", _assert_in_bracket(f, r["f_want"], eps, f"f after {L} iterations", factor=2 * L), "of the bracket; of g:",
          _assert_in_bracket(g, r["g_want"], eps, f"g after {L} iterations", factor=2 * L))
    # kneighbors(5): exactly the stable sort of (d - f) - g over the candidates with the device's potentials ...
    w5, want_i5 = LR.topk_lists(LR.list_w(cd, ci, f, g), ci, 5)
    np.testing.assert_array_equal(r["i5"], want_i5)
    np.testing.assert_array_equal(r["d5"], w5)
    # ... and the restatement's lists, except where its neighbouring values stand closer than twice the bracket
    W = LR.list_w(cd, ci, r["f_want"], r["g_want"])
    w_bracket = 2 * L * (SR.bracket(r["f_want"], eps)[:, None] + np.nanmax(SR.bracket(r["g_want"], eps)))
    clear = (np.diff(np.sort(W, axis=1)[:, :6], axis=1) > 2 * w_bracket).all(axis=1)
    print("rows whose first restated values stand clear of each other:", int(clear.sum()), "of", n_s, "=", clear.mean())
    assert clear.mean() >= 0.95
    np.testing.assert_array_equal(r["i5"][clear], LR.topk_lists(W, ci, 5)[1][clear])
    # the whole-index calls work on these potentials: position == rank, and the targets without a potential come last, by row
    wi_w, wi_i = kz.kneighbors_whole_index(10)
    assert not np.isin(wi_i, unlisted).any() and not np.isnan(wi_w).any()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(wi_i, np.argsort(np.where(np.isnan(g), np.inf, SR.w(D, f, g)), axis=1, kind="stable")[:, :10])
    for c in (0, 4, 9):
        np.testing.assert_array_equal(kz.gold_ranks(np.ascontiguousarray(wi_i[:, c]), reduced=True), np.full(n_s, c))
    rank = kz.gold_ranks(r["gold"], reduced=True)
    listed = wi_i == r["gold"][:, None]
    np.testing.assert_array_equal(rank[listed.any(axis=1)], np.argmax(listed, axis=1)[listed.any(axis=1)])
    assert (rank[~listed.any(axis=1)] >= 10).all()
    for pos, u in enumerate(unlisted[:3]):
        np.testing.assert_array_equal(kz.gold_ranks(np.full(n_s, u, dtype=np.int64), reduced=True), np.full(n_s, n_t - unlisted.size + pos))
    # match(10) = the stable matching over the lists kneighbors(10) returns
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # (K = 5: k is clamped to n_candidates, with a warning)
        m_dist, m_ind = kz.match(10)
        want_dist, want_ind = matching.one_to_one(*kz.kneighbors(10), n_t)
    np.testing.assert_array_equal(m_ind, want_ind)
    np.testing.assert_array_equal(m_dist, want_dist)
    matched = m_ind[m_ind >= 0]
    assert len(set(matched.tolist())) == matched.size > 0.5 * n_s
    # matching.sinkhorn_lists on the numpy lists: the class's potentials, bit for bit; padding changes nothing
    f2, g2, info = matching.sinkhorn_lists(cd, ci, n_t, temperature=eps, n_iter=L, return_info=True)
    np.testing.assert_array_equal(_bits(f2), _bits(f))
    np.testing.assert_array_equal(_bits(g2), _bits(g))
    assert info == {"n_iter": L, "potential_change": r["change"]}
    if K == 5:
        pad_i = np.concatenate([ci, np.full((n_s, 1), INT_MAX), np.full((n_s, 2), -1)], axis=1)
        pad_d = np.concatenate([cd, np.full((n_s, 3), np.nan)], axis=1)
        f3, g3 = matching.sinkhorn_lists(pad_d, pad_i, n_t, temperature=eps, n_iter=L)
        np.testing.assert_array_equal(_bits(f3), _bits(f))             # (k = 8 pads the group of 8 lanes that k = 5 uses)
        np.testing.assert_array_equal(_bits(g3), _bits(g))
    if (case, K) == LIST_FIT_CASES[2]:
        hits = (r["i5"][:, 0] == r["gold"]).mean()
        print("hits@1 over 10 candidates:", hits, "raw distance:", (D.argmin(axis=1) == r["gold"]).mean())
        assert hits == (LR.topk_lists(W, ci, 1)[1][:, 0] == r["gold"]).mean()


@pytest.mark.parametrize("case,K", [LIST_FIT_CASES[0], LIST_FIT_CASES[3]], ids=[LIST_FIT_IDS[0], LIST_FIT_IDS[3]])
def test_precomputed_matrix_early_stopping_and_the_whole_index_support(ctx, list_fits, case, K):
    from kiez_amd import Sinkhorn
    n_s, n_t, eps, L, noise = case
    _, r = list_fits[(case, K)]
    s, t, D = r["s"], r["t"], r["D"]
    # metric="precomputed" on the device's own float64 matrix: the bits of the embeddings fit
    pre = _kiez(Sinkhorn, K, metric="precomputed", temperature=eps, n_iter=L, support="candidates").fit(np.array(D))
    np.testing.assert_array_equal(_bits(pre.hubness.source_potential_), _bits(r["f"]))
    np.testing.assert_array_equal(_bits(pre.hubness.target_potential_), _bits(r["g"]))
    d5, i5 = pre.kneighbors(5)
    np.testing.assert_array_equal(i5, r["i5"])
    np.testing.assert_array_equal(d5, r["d5"])
    # tol through the class
    if K == 10:
        hub = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, tol=1e-3, support="candidates").fit(s, t).hubness
        assert hub.n_iter_ == 40 and hub.potential_change_ <= 1e-3
        one = _kiez(Sinkhorn, K, temperature=eps, n_iter=1, tol=1e-3, support="candidates").fit(s, t).hubness
        assert one.n_iter_ == 1 and one.potential_change_ is None
    # support="index" is the code path it was: the default's bits, within the whole-index restatement's bracket
    a = _kiez(Sinkhorn, K, temperature=eps, n_iter=L).fit(s, t).hubness
    b = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, support="index").fit(s, t).hubness
    assert a.support == b.support == "index" and a.n_iter_ == b.n_iter_ == L and a.potential_change_ == b.potential_change_
    np.testing.assert_array_equal(_bits(a.source_potential_), _bits(b.source_potential_))
    np.testing.assert_array_equal(_bits(a.target_potential_), _bits(b.target_potential_))
    f_want, g_want = SR.sinkhorn_potentials(D, eps, L)
    _assert_in_bracket(b.source_potential_, f_want, eps, "support='index' f", factor=2 * L)
    _assert_in_bracket(b.target_potential_, g_want, eps, "support='index' g", factor=2 * L)
    assert not np.isnan(b.target_potential_).any()
    assert a.nn_algo._forward is None                                   # (and it caches no lists)


def test_inverted_softmax_on_the_candidate_lists(list_fits):
    from kiez_amd import InvertedSoftmax
    case, K = LIST_FIT_CASES[3]
    n_s, n_t, eps = case[:3]
    _, r = list_fits[(case, K)]
    kz = _kiez(InvertedSoftmax, K, temperature=eps, support="candidates").fit(r["s"], r["t"])
    hub = kz.hubness
    f, g = hub.source_potential_, hub.target_potential_
    np.testing.assert_array_equal(f, np.zeros(n_s))
    assert hub.n_iter_ == 1 and hub.potential_change_ is None
    want = LR.inverted_softmax_potential(r["cd"], r["ci"], n_t, eps)
    assert np.isnan(want).sum() >= 1
    print("worst error of g:", _assert_in_bracket(g, want, eps, "inverted softmax g"), "of the bracket")
    # the lists are ranked by d - g_j over the candidates
    d5, i5 = kz.kneighbors(5)
    w5, want_i5 = LR.topk_lists(LR.list_w(r["cd"], r["ci"], f, g), r["ci"], 5)
    np.testing.assert_array_equal(i5, want_i5)
    np.testing.assert_array_equal(d5, w5)
    both = _kiez(InvertedSoftmax, K, temperature=eps).fit(r["s"], r["t"]).hubness
    assert both.support == "index" and not np.isnan(both.target_potential_).any()


TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd import Kiez, Sinkhorn
from tests import sinkhorn_restate as SR
s, t, gold = SR.alignment_case(180, 257, 0.3)
kw = dict(n_candidates=5, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=Sinkhorn,
          hubness_kwargs={"temperature": 0.05, "n_iter": 5, "support": "candidates"})
kz = Kiez(**kw).fit(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda())
d5, i5 = kz.kneighbors(5)
assert isinstance(d5, torch.Tensor) and isinstance(i5, torch.Tensor) and d5.is_cuda and d5.dtype == torch.float64 and i5.dtype == torch.int64
d, i = kz.kneighbors_whole_index(10)
assert isinstance(d, torch.Tensor) and d.shape == (180, 10)
ref = Kiez(**kw).fit(s, t)
rd5, ri5 = ref.kneighbors(5)
rd, ri = ref.kneighbors_whole_index(10)
assert isinstance(rd5, np.ndarray)
assert np.array_equal(i5.cpu().numpy(), ri5) and np.array_equal(d5.cpu().numpy(), rd5)
assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(d.cpu().numpy(), rd)
g = kz.hubness.target_potential_
assert np.isnan(g).sum() >= 1 and np.array_equal(g, ref.hubness.target_potential_, equal_nan=True)
assert np.array_equal(kz.hubness.source_potential_, ref.hubness.source_potential_)
print("TORCH_OK")
"""


def test_tensors_in_tensors_out():
    """A fit on torch tensors with support="candidates" returns tensors, with the values of the numpy fit: the inherited path (in a
    child process: torch must load its HIP runtime first)."""
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
