"""The CSR (ragged) pair-list calls on the device -- kz_match_csr, kz_assign_csr, kz_csr_transpose, kz_softmin_csr_rows,
kz_sinkhorn_csr -- against the fixed-width calls on the padded lists (where the longest row fits their 4 096 columns) and against the
numpy restatements of those calls on the padded arrays (every case, the 4 100-entry rows included).  Shapes: 300 rows, 600 or 5 000
targets; the row lengths of tests/csr_lists_restate.py, each once as the first and once as the last row."""
import math
import zlib

import numpy as np
import pytest

from tests import assignment_restate as AR
from tests import csr_lists_restate as CR
from tests import match_restate as MR
from tests import radius_restate as RR
from tests import sinkhorn_lists_restate as LR
from tests import sinkhorn_restate as SR

pytestmark = pytest.mark.gpu

CASES = CR.cases()
_cache = {}


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _case(name, dtype=np.float64, plain=False):
    """(indptr, ind, dist, n_index, padded dist, padded ind) of a case, built once and left unchanged."""
    key = (name, np.dtype(dtype).name, plain)
    if key not in _cache:
        _, n_index, lengths = next(c for c in CASES if c[0] == name)
        indptr, ind, dist = CR.random_csr(np.random.default_rng(zlib.crc32(name.encode())), 300, n_index, lengths, plain=plain, dtype=dtype)
        _cache[key] = (indptr, ind, dist, n_index) + CR.pad(indptr, ind, dist)
    return _cache[key]


def _dev(ctx, *arrays):
    return tuple(ctx.to_device(a) for a in arrays)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_match_csr(ctx, name, dtype):
    from kiez_amd import _native as N
    indptr, ind, dist, n_index, p_dist, p_ind = _case(name, dtype)
    d_ptr, d_ind, d_dist = _dev(ctx, indptr, ind, dist)
    match, col, rounds = N.match_csr(ctx, d_ptr, d_ind, d_dist, n_index)
    match, col = match.numpy(), col.numpy()
    want = MR.gale_shapley(p_dist, p_ind, n_index)
    np.testing.assert_array_equal(match, want[0])
    np.testing.assert_array_equal(col, want[1])
    assert MR.blocking_pairs(p_dist, p_ind, n_index, (match, col)) == []
    assert 1 <= rounds <= ind.size + n_index
    if p_ind.shape[1] <= 4096:
        l_match, l_col, l_rounds = N.match_lists(ctx, *_dev(ctx, p_dist, p_ind), n_index)
        np.testing.assert_array_equal(match, l_match.numpy())
        np.testing.assert_array_equal(col, l_col.numpy())
        assert rounds == l_rounds
    values = N.match_values_csr(ctx, d_ptr, d_dist, ctx.to_device(col)).numpy()
    assert values.dtype == dtype
    np.testing.assert_array_equal(values, np.where(col >= 0, p_dist[np.arange(300), np.maximum(col, 0)], np.nan))


def _assign_all(ctx, indptr, ind, dist, n_index, u, eps, tail_rows=0):
    from kiez_amd import _native as N
    match, col, price, rounds, converged = N.assign_csr(ctx, *_dev(ctx, indptr, ind, dist), n_index, u, eps, 1_000_000, tail_rows=tail_rows,
                                                        want_prices=True)
    return match.numpy(), col.numpy(), price.numpy(), rounds, converged


def _assert_same_auction(got, want, where):
    for g, w, what in zip(got[:2], want[:2], ("match", "col")):
        np.testing.assert_array_equal(g, w, err_msg=f"{where}: {what}")
    np.testing.assert_array_equal(_bits(got[2]), _bits(want[2]), err_msg=f"{where}: price bits")
    assert (got[3], bool(got[4])) == (want[3], bool(want[4])), f"{where}: rounds / converged {got[3:]} != {want[3:]}"


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_assign_csr(ctx, name):
    from kiez_amd import _native as N
    indptr, ind, dist, n_index, p_dist, p_ind = _case(name)
    u, _ = AR.defaults(p_dist, p_ind, n_index)
    u = 0.7 * u
    eps = 1.0 / 256                                   # (the values lie on a grid of 1 / 128: a run of a few hundred rounds)
    got = _assign_all(ctx, indptr, ind, dist, n_index, u, eps)
    want = AR.auction(p_dist, p_ind, n_index, u, eps)
    assert want[4]
    _assert_same_auction(got, want, "against the restated auction")
    for tail_rows in (-1, 64):
        _assert_same_auction(_assign_all(ctx, indptr, ind, dist, n_index, u, eps, tail_rows), got, f"tail_rows={tail_rows}")
    if p_ind.shape[1] <= 4096:
        m, c, p, rounds, conv = N.assign_lists(ctx, *_dev(ctx, p_dist, p_ind), n_index, u, eps, 1_000_000, want_prices=True)
        _assert_same_auction(got, (m.numpy(), c.numpy(), p.numpy(), rounds, conv), "against kz_assign_lists on the padded lists")
    cost = AR.cost(p_dist, p_ind, n_index, u, got[0], got[1])
    best = AR.optimum(p_dist, p_ind, n_index, u)
    print(f"{name}: {got[3]} rounds, cost {cost:.6f}, optimum {best:.6f}, bound {300 * eps:.6f}")
    assert cost <= best + 300 * eps + 1e-9 * max(1.0, abs(best))          # (the sums themselves round)
    lo_hi = N.assign_range_csr(ctx, *_dev(ctx, indptr, ind, dist), n_index)
    assert lo_hi == AR.value_range(p_dist, p_ind, n_index)


def test_a_displaced_long_row_bids_again_with_the_wave(ctx):
    """Two long rows share their best target: one loses the first round or is displaced later, and bids again -- the wave kernel runs
    in a late round, behind prices that moved."""
    rng = np.random.default_rng(3)
    n_index, long_len = 600, CR.LONG_ROW + 40
    indptr, ind, dist = CR.random_csr(rng, 300, n_index, {10: long_len, 200: long_len, 299: 5}, plain=True)
    for row in (10, 200):
        a = indptr[row]
        ind[a:a + long_len] = rng.permutation(np.arange(1, n_index - 1))[:long_len]      # distinct targets, the shared best one last
        dist[a:a + long_len] = 0.5 + rng.integers(0, 64, size=long_len) / 128.0
        ind[a + long_len - 1], dist[a + long_len - 1] = 5, 0.0
    p_dist, p_ind = CR.pad(indptr, ind, dist)
    u, eps = 2.0, 1.0 / 256
    want = AR.auction(p_dist, p_ind, n_index, u, eps)
    got = _assign_all(ctx, indptr, ind, dist, n_index, u, eps)
    _assert_same_auction(got, want, "two long rows, one best target")
    for tail_rows in (-1, 64):
        _assert_same_auction(_assign_all(ctx, indptr, ind, dist, n_index, u, eps, tail_rows), got, f"tail_rows={tail_rows}")
    assert got[3] >= 2 and not (got[0][10] == 5 and got[0][200] == 5)
    assert got[0][10] >= 0 and got[0][200] >= 0          # (the one that lost the shared target bid again and holds another)


def _assert_in_bracket(got, want, eps, where, factor=1):
    """tests/test_gpu_sinkhorn_lists.py's helper: non-finite restated values exactly, the others within factor x SR.bracket."""
    assert got.shape == want.shape and got.dtype == np.float64, where
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite], err_msg=where)
    err = np.abs(got[finite] - want[finite])
    bound = factor * SR.bracket(want[finite], eps)
    worst = float((err / bound).max()) if err.size else 0.0
    assert (err <= bound).all(), f"{where}: {worst:.3g} of the bracket"
    return worst


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_softmin_csr_rows(ctx, name):
    from kiez_amd import _native as N
    rng = np.random.default_rng(11)
    # the row tree IS the column tree: bit for bit kz_softmin_list_cols on the view (colptr = indptr, col_row = ind, col_val = dist)
    indptr, ind, dist, n_index, _, _ = _case(name, plain=True)
    d_ptr, d_ind, d_dist = _dev(ctx, indptr, ind, dist)
    view = N.ListsTransposed(d_ptr, ctx.to_device(ind.astype(np.int32)), d_dist, ind.size, n_index, 300)
    off = ctx.to_device(rng.standard_normal(n_index))
    for eps in (1e-3, 0.05, 1.0):
        for o, shift in ((None, 0.0), (off, 0.25)):
            got = N.softmin_csr_rows(ctx, d_ptr, d_ind, d_dist, n_index, eps, off=o, shift=shift).numpy()
            np.testing.assert_array_equal(_bits(got), _bits(N.softmin_list_cols(ctx, view, eps, off=o, shift=shift).numpy()),
                                          err_msg=f"eps={eps} shift={shift}")
    # ... and with ids that are no pair in the rows: within the bracket of the restated row soft-min on the padded arrays
    indptr, ind, dist, n_index, p_dist, p_ind = _case(name)
    d_ptr, d_ind, d_dist = _dev(ctx, indptr, ind, dist)
    worst = 0.0
    for eps in (1e-3, 0.05, 1.0):
        for o, shift in ((None, 0.0), (off, 0.25)):
            got = N.softmin_csr_rows(ctx, d_ptr, d_ind, d_dist, n_index, eps, off=o, shift=shift).numpy()
            want = LR.softmin_rows(p_dist, p_ind, n_index, eps, off=None if o is None else o.numpy(), shift=shift)
            worst = max(worst, _assert_in_bracket(got, want, eps, f"rows eps={eps} shift={shift}"))
            assert np.isnan(got[np.diff(indptr) == 0]).all()                       # an empty row has no value
    print(f"{name}: worst error {worst:.2e} of the bracket")
    # the transposition: numpy's stable sort of (target id, flat position)
    t = N.csr_transpose(ctx, d_ptr, d_ind, d_dist, n_index)
    ok = (ind >= 0) & (ind < n_index)
    order = np.argsort(np.where(ok, ind, n_index), kind="stable")[:int(ok.sum())]
    rows = np.repeat(np.arange(300), np.diff(indptr))
    assert t.nnz == int(ok.sum())
    np.testing.assert_array_equal(t.colptr.numpy(), np.searchsorted(ind[order], np.arange(n_index + 1), side="left"))
    np.testing.assert_array_equal(t.col_row.numpy()[:t.nnz], rows[order])
    np.testing.assert_array_equal(t.col_val.numpy()[:t.nnz], dist[order])


def _composed(ctx, d_ptr, d_ind, d_dist, n_index, eps, n_iter, tol=None):
    """kz_sinkhorn_csr's loop over its own step calls and kz_max_abs_diff -> (f, g, iterations, change)."""
    from kiez_amd import _native as N
    view = N.csr_transpose(ctx, d_ptr, d_ind, d_dist, n_index)
    shift = eps * math.log((d_ptr.shape[0] - 1) / n_index)
    f = g = change = None
    for it in range(1, n_iter + 1):
        g_new = N.softmin_list_cols(ctx, view, eps, off=f, shift=shift)
        if g is not None:
            change = N.max_abs_diff(ctx, g_new, g)
        g = g_new
        f = N.softmin_csr_rows(ctx, d_ptr, d_ind, d_dist, n_index, eps, off=g)
        if tol is not None and change is not None and change <= tol:
            break
    return f.numpy(), g.numpy(), it, change


@pytest.mark.parametrize("name", [CASES[0][0], CASES[5][0], CASES[11][0]])
def test_sinkhorn_csr_is_the_composition_of_its_steps(ctx, name):
    from kiez_amd import _native as N
    indptr, ind, dist, n_index, p_dist, p_ind = _case(name)
    dev = _dev(ctx, indptr, ind, dist)
    eps = 0.05
    f, g, done, change = N.sinkhorn_csr(ctx, *dev, n_index, eps, 6)
    cf, cg, c_done, c_change = _composed(ctx, *dev, n_index, eps, 6)
    assert (done, change) == (c_done, c_change) == (6, c_change)
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(cf))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(cg))
    f2, g2, _, _ = N.sinkhorn_csr(ctx, *dev, n_index, eps, 6)                      # the same bits twice in a row
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(f2.numpy()))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(g2.numpy()))
    # an empty row and a row without a pair: NaN; a target nobody lists: NaN
    listed = np.zeros(n_index, dtype=bool)
    listed[ind[(ind >= 0) & (ind < n_index)]] = True
    assert not listed[n_index - 1] and np.isnan(g.numpy()[~listed]).all() and not np.isnan(g.numpy()[listed]).any()
    no_pair = ~((p_ind >= 0) & (p_ind < n_index)).any(axis=1)
    assert np.isnan(f.numpy()[no_pair]).all() and not np.isnan(f.numpy()[~no_pair]).any()
    # the restated loop on the padded arrays, 2 L brackets as tests/test_gpu_sinkhorn_lists.py allows L iterations
    wf, wg, _, _ = LR.sinkhorn_potentials(p_dist, p_ind, n_index, eps, 6)
    _assert_in_bracket(f.numpy(), wf, eps, "f after 6 iterations", factor=12)
    _assert_in_bracket(g.numpy(), wg, eps, "g after 6 iterations", factor=12)
    # the stopping rule, decided on the device: the iteration the composition stops at
    changes = [_composed(ctx, *dev, n_index, eps, L)[3] for L in (2, 3, 4, 5)]
    tol = changes[1] * 1.0000001                                                    # (met at iteration 3 at the latest)
    cf, cg, c_done, c_change = _composed(ctx, *dev, n_index, eps, 30, tol)
    f, g, done, change = N.sinkhorn_csr(ctx, *dev, n_index, eps, 30, tol)
    assert (done, change) == (c_done, c_change) and done <= 3
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(cf))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(cg))


# ---- the ONE loop behind kz_sinkhorn_lists and kz_sinkhorn_csr (kz_sl_sinkhorn_run), on both layouts ----------------------------------
def _loop_lists(shape):
    """(dist, ind [n_q, k], n_index), seeded.  "small": 5 x 7, k = 3.  "long column": 600 x 3, k = 2 and every row lists target 0 -- a
    column of more than SOFTMIN_LIST_CHUNK = 512 entries: two chunks and the fold of their parts."""
    rng = np.random.default_rng(5)
    if shape == "small":
        return rng.random((5, 3)), np.stack([rng.permutation(7)[:3] for _ in range(5)]).astype(np.int64), 7
    return rng.random((600, 2)), np.stack([np.zeros(600, dtype=np.int64), rng.integers(1, 3, 600)], axis=1), 3


def _composed_lists(ctx, d_dev, i_dev, n_index, eps, n_iter, tol=None):
    """`_composed` for fixed-width lists (tests/test_gpu_sinkhorn_lists.py's helper)."""
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


@pytest.mark.parametrize("layout", ["lists", "csr", "csr with an empty row"])
@pytest.mark.parametrize("shape,n_iter,stop_at", [("small", 1, None), ("small", 30, 4), ("small", 30, 5), ("long column", 3, None)],
                         ids=["one iteration", "tol met at an even iteration", "tol met at an odd iteration", "a column of two chunks"])
def test_the_loop_on_both_layouts(ctx, layout, shape, n_iter, stop_at):
    """One iteration (nothing measured), a tolerance met at an even and at an odd iteration >= 3 (either half of the double-buffered g
    is the one copied out) and a column of more than one chunk, on the fixed-width lists, on the same pairs as a CSR and on that CSR
    with its middle row emptied.  Bit for bit the composition of the step calls; the numpy restatement (tests/sinkhorn_lists_restate.py
    on the padded arrays) stops at the same iteration and agrees within 2 L brackets, as everywhere in this file -- its exp and log are
    numpy's, so its bits are not the device's."""
    from kiez_amd import _native as N
    eps = 0.2
    p_dist, p_ind, n_index = _loop_lists(shape)
    if layout == "lists":
        dev = _dev(ctx, p_dist, p_ind)
        run, composed = N.sinkhorn_lists, _composed_lists
    else:
        lens = np.full(p_ind.shape[0], p_ind.shape[1])
        if layout == "csr with an empty row":
            lens[p_ind.shape[0] // 2] = 0
        keep = np.repeat(lens > 0, p_ind.shape[1])
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        dev = _dev(ctx, indptr, p_ind.ravel()[keep], p_dist.ravel()[keep])
        p_dist, p_ind = CR.pad(indptr, p_ind.ravel()[keep], p_dist.ravel()[keep])
        run, composed = N.sinkhorn_csr, _composed
    tol = None
    if stop_at is not None:   # a tolerance between the restated changes of iterations stop_at - 1 and stop_at, far from both
        changes = [LR.sinkhorn_potentials(p_dist, p_ind, n_index, eps, L)[3] for L in range(2, stop_at + 1)]
        tol = math.sqrt(changes[-1] * min(changes[:-1]))
        assert changes[-1] * 1.02 < tol < min(changes[:-1]) / 1.02, changes
    wf, wg, w_done, _ = LR.sinkhorn_potentials(p_dist, p_ind, n_index, eps, n_iter, tol)
    f, g, done, change = run(ctx, *dev, n_index, eps, n_iter, tol)
    cf, cg, c_done, c_change = composed(ctx, *dev, n_index, eps, n_iter, tol)
    assert done == c_done == w_done == (stop_at or n_iter) and change == c_change and (change is None) == (done == 1)
    np.testing.assert_array_equal(_bits(f.numpy()), _bits(cf))
    np.testing.assert_array_equal(_bits(g.numpy()), _bits(cg))
    _assert_in_bracket(f.numpy(), wf, eps, f"f after {done} iterations", factor=2 * done)
    _assert_in_bracket(g.numpy(), wg, eps, f"g after {done} iterations", factor=2 * done)
    if layout == "csr with an empty row":
        assert np.isnan(f.numpy()[p_ind.shape[0] // 2]) and np.isnan(f.numpy()).sum() == 1


def test_the_loop_without_an_entry_and_without_a_row(ctx):
    from kiez_amd import _native as N
    none_i, none_d = np.zeros(0, dtype=np.int64), np.zeros(0)
    # a CSR with nnz = 0 (colptr is a memset, the view has no place): no row and no column has a pair
    dev = _dev(ctx, np.zeros(5, dtype=np.int64), none_i, none_d)
    for tol, want_done in ((None, 3), (0.0, 2)):                                   # (the change of all-NaN vectors is 0.0: met at once)
        f, g, done, change = N.sinkhorn_csr(ctx, *dev, 3, 0.05, 3, tol)
        cf, cg, c_done, c_change = _composed(ctx, *dev, 3, 0.05, 3, tol)
        assert (done, change) == (c_done, c_change) == (want_done, 0.0)
        assert f.shape == (4,) and g.shape == (3,) and np.isnan(f.numpy()).all() and np.isnan(g.numpy()).all()
        assert np.isnan(cf).all() and np.isnan(cg).all()
    # n_q = 0: nothing runs, nothing is measured
    for got in (N.sinkhorn_csr(ctx, *_dev(ctx, np.zeros(1, dtype=np.int64), none_i, none_d), 3, 0.05, 3),
                N.sinkhorn_lists(ctx, *_dev(ctx, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)), 3, 0.05, 3)):
        assert (got[0].shape, got[1].shape, got[2], got[3]) == ((0,), (3,), 0, None)


def test_a_decreasing_device_indptr_is_a_value_error(ctx):
    """[0, 5, 3, 8]: inside bounds everywhere -- an unchecked walk over it would read nothing out of bounds either."""
    from kiez_amd import _native as N
    from kiez_amd import matching
    d_ptr, d_ind = _dev(ctx, np.array([0, 5, 3, 8], dtype=np.int64), np.arange(8, dtype=np.int64) % 4)
    d_dist = ctx.to_device(np.linspace(0.0, 1.0, 8))
    for call in (lambda: N.match_csr(ctx, d_ptr, d_ind, d_dist, 4),
                 lambda: N.match_values_csr(ctx, d_ptr, d_dist, ctx.to_device(np.zeros(3, dtype=np.int64))),
                 lambda: N.assign_csr(ctx, d_ptr, d_ind, d_dist, 4, 1.0, 0.01, 100),
                 lambda: N.csr_transpose(ctx, d_ptr, d_ind, d_dist, 4),
                 lambda: N.softmin_csr_rows(ctx, d_ptr, d_ind, d_dist, 4, 0.05),
                 lambda: N.sinkhorn_csr(ctx, d_ptr, d_ind, d_dist, 4, 0.05, 3),
                 lambda: matching.one_to_one_csr(d_ptr, d_ind, d_dist, 4),
                 lambda: matching.assignment_csr(d_ptr, d_ind, d_dist, 4),
                 lambda: matching.sinkhorn_csr(d_ptr, d_ind, d_dist, 4)):
        with pytest.raises(ValueError, match="never decrease"):
            call()
    good = ctx.to_device(np.array([0, 5, 5, 8], dtype=np.int64))                   # (and the context is as usable as before)
    assert N.match_csr(ctx, good, d_ind, d_dist, 4)[0].numpy().tolist() == [0, -1, 1]


def test_matching_functions_take_numpy_and_device_csr(ctx):
    from kiez_amd import _native as N
    from kiez_amd import matching
    indptr, ind, dist, n_index, p_dist, p_ind = _case(CASES[3][0], np.float32)
    md, mi = matching.one_to_one_csr(indptr, ind, dist, n_index)
    want = MR.gale_shapley(p_dist, p_ind, n_index)
    np.testing.assert_array_equal(mi, want[0])
    assert md.dtype == np.float32 and isinstance(mi, np.ndarray)
    dd, di = matching.one_to_one_csr(ctx.to_device(indptr), ctx.to_device(ind), ctx.to_device(dist), n_index)
    assert isinstance(dd, N.DeviceArray)
    np.testing.assert_array_equal(di.numpy(), mi)
    np.testing.assert_array_equal(dd.numpy(), md)
    u, eps = AR.defaults(p_dist, p_ind, n_index)
    ad, ai, prices = matching.assignment_csr(indptr, ind, dist, n_index, eps=1.0 / 256, return_prices=True)
    w = AR.auction(p_dist, p_ind, n_index, u, 1.0 / 256)
    np.testing.assert_array_equal(ai, w[0])
    np.testing.assert_array_equal(_bits(prices), _bits(w[2]))
    bi = matching.assignment_csr(ctx.to_device(indptr), ctx.to_device(ind), ctx.to_device(dist), n_index, eps=1.0 / 256, return_distance=False)
    np.testing.assert_array_equal(bi.numpy(), ai)
    with pytest.raises(RuntimeError, match="max_rounds"):
        matching.assignment_csr(indptr, ind, dist, n_index, eps=1.0 / 256, max_rounds=1)
    f, g, info = matching.sinkhorn_csr(indptr, ind, dist, n_index, n_iter=3, return_info=True)
    wf, wg, _, _ = LR.sinkhorn_potentials(p_dist.astype(np.float64), p_ind, n_index, 0.05, 3)
    _assert_in_bracket(f, wf, 0.05, "f", factor=6)
    _assert_in_bracket(g, wg, 0.05, "g", factor=6)
    assert info["n_iter"] == 3


@pytest.mark.parametrize("hubness", ["CSLS", None], ids=["csls", "plain"])
def test_facade_radius_then_one_to_one(hubness):
    from kiez_amd import Kiez, evaluate, matching
    s, t, gold = SR.alignment_case(300, 300, 0.3)
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=hubness)
    kz.fit(s, t)
    if hubness:
        w_all, i_all = kz.kneighbors_whole_index(300)
        w = np.empty((300, 300))
        w[np.arange(300)[:, None], i_all] = w_all
    else:
        w = 1.0 - s @ t.T
    r, gap = RR.gap_radius(w, per_row=20)
    indptr, ind, dist = kz.radius_neighbors(r, reduced=True)
    p_dist, p_ind = CR.pad(indptr, ind, dist)
    md, mi = kz.match_radius(r, reduced=True)
    wd, wi = matching.one_to_one(p_dist, p_ind, 300)
    np.testing.assert_array_equal(mi, wi)
    np.testing.assert_array_equal(md, wd)
    np.testing.assert_array_equal(kz.match_radius(r, reduced=True, return_distance=False), wi)
    ad, ai = kz.assign_radius(r, reduced=True)
    xd, xi = matching.assignment(p_dist, p_ind, 300)
    np.testing.assert_array_equal(ai, xi)
    np.testing.assert_array_equal(ad, xd)
    hits = evaluate.hits(mi[:, None], dict(enumerate(gold.tolist())), k=[1])
    print(f"hubness={hubness}: radius {r:.6f} (gap {gap:.2e}), {ind.size / 300:.1f} pairs a row, matched {int((mi >= 0).sum())}, hits {hits}")
    if hubness:                       # every pair: a row of at most 512 entries is the head of the whole-index list
        fd, fi = kz.match_radius(np.inf, reduced=True)
        gd, gi = kz.match(300, whole_index=True)
        np.testing.assert_array_equal(fi, gi)
        np.testing.assert_array_equal(fd, gd)
        fd, fi = kz.assign_radius(np.inf, reduced=True)
        gd, gi = kz.assign(300, whole_index=True)
        np.testing.assert_array_equal(fi, gi)
        np.testing.assert_array_equal(fd, gd)
