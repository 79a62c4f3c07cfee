"""Sinkhorn and the inverted softmax over the whole index on the device: kz_softmin_rows against the numpy restatement
(tests/sinkhorn_restate.py) over the device's own distances, around the chunk size and for every branch of the distance conversion;
special values at the ABI; the summation tree rule (same bits whatever the batch split and the row's alignment); the pointwise kind
KZ_RANK_DUAL through kz_gold_ranks_reduced / kz_knn_reduced / kz_dual_shift; the fitted classes against the restatement and through
every inherited call.  `pytest -m gpu`.

Brackets.  One soft-min: |got - want| <= 1e-12 (|want| + eps) -- the project's bracket for the exp-based kinds; a different summation
order costs a relative ~log2(n) 2^-53 on the sum, an absolute eps 2e-15 on the result, plus one rounding of m.  Potentials after L
iterations: 2 L times that (soft-min is 1-Lipschitz in the sup norm: the errors add and do not grow)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import sinkhorn_restate as SR
from tests import whole_index_restate as WI

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _matrices(ctx, q, y, metric, p=2):
    from kiez_amd import _native as N
    from kiez_amd.neighbors import canonical_metric
    name = canonical_metric(metric, p)
    return N.DeviceMatrix(ctx, q, name), N.DeviceMatrix(ctx, y, name)


def _distances(ctx, qm, ym, metric, p=2):
    """[n_q, n_i] float64: the distance kz_knn returns for every pair -- kz_pair_values (the device's own ranking values) converted as
    kz_output_distance converts them."""
    from kiez_amd import _native as N
    n_q, n_i = qm.shape[0], ym.shape[0]
    ind = ctx.to_device(np.tile(np.arange(n_i, dtype=np.int64), (n_q, 1)))
    val = ctx.empty((n_q, n_i), np.float64)
    N._check(ctx.lib.kz_pair_values(ctx.handle, qm.handle, 0, n_q, ym.handle, ind.ptr, n_i, val.ptr), "kz_pair_values")
    v = val.numpy()
    f32 = qm.dtype == np.float32
    if metric == "euclidean":
        return np.sqrt(v.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64) if f32 else np.sqrt(v)
    if metric == "minkowski":
        d = v ** (1.0 / p)
        return d.astype(np.float32).astype(np.float64) if f32 else d
    if metric == "correlation":
        return np.where(np.isinf(v), np.nan, v)
    return v


def _assert_in_bracket(got, want, eps, where, factor=1):
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite], err_msg=where)
    err = np.abs(got[finite] - want[finite])
    bound = factor * SR.bracket(want[finite], eps)
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{where}: worst error {worst:.2e} of the bracket")
    assert (err <= bound).all(), f"{where}: {worst:.3g} of the bracket"


# one (metric, p, dtype) per branch of kz_output_distance, and correlation for the NaN distances
CASES = [("euclidean", 2, np.float32), ("euclidean", 2, np.float64), ("cosine", 2, np.float32), ("minkowski", 3, np.float32),
         ("correlation", 2, np.float64)]
CASE_IDS = [f"{m}{p if m == 'minkowski' else ''}_{np.dtype(t).name}" for m, p, t in CASES]
EPS = (1e-3, 0.05, 1.0, 50.0)


@pytest.mark.parametrize("metric,p,dtype", CASES, ids=CASE_IDS)
def test_softmin_rows_against_the_restatement(ctx, metric, p, dtype):
    from kiez_amd import _native as N
    C = N.SOFTMIN_CHUNK
    n_q, d = 33, 8
    for n_i in (1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1):
        rng = np.random.default_rng(n_i)
        q, y = rng.standard_normal((n_q, d)).astype(dtype), rng.standard_normal((n_i, d)).astype(dtype)
        if metric == "correlation":
            y[n_i // 2] = 1.5                                   # a constant index row: a NaN in every row
            q[5] = -0.25                                        # a constant query row: NaN only
        qm, ym = _matrices(ctx, q, y, metric, p)
        D = _distances(ctx, qm, ym, metric, p)
        if metric == "correlation":
            assert np.isnan(D[:, n_i // 2]).all() and np.isnan(D[5]).all()
        off = 0.5 * rng.standard_normal(n_i)
        off_dev = ctx.to_device(off)
        for eps in EPS:
            for with_off, shift in ((False, 0.75), (True, -1.25), (True, 0.0)):
                got = N.softmin_rows(ctx, qm, ym, eps, off=off_dev if with_off else None, shift=shift).numpy()
                want = SR.softmin(D - off[None, :] if with_off else D, eps, axis=1) + shift
                where = f"{metric} {np.dtype(dtype).name} n_index={n_i} eps={eps} off={with_off} shift={shift}"
                assert got.shape == (n_q,) and got.dtype == np.float64
                if metric == "correlation":
                    assert got[5] == np.inf and (np.isfinite(np.delete(got, 5)).all() or n_i == 1), where
                _assert_in_bracket(got, want, eps, where)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_softmin_rows_far_from_unit_scale(ctx, dtype):
    """Rows 1000 + 40 N(0, 1), eps = 0.02: exp(-d / eps) underflows for every pair -- without the minimum taken out the result is +inf."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(1000)
    n_i = N.SOFTMIN_CHUNK + 1
    q = (1000.0 + 40.0 * rng.standard_normal((33, 8))).astype(dtype)
    y = (1000.0 + 40.0 * rng.standard_normal((n_i, 8))).astype(dtype)
    qm, ym = _matrices(ctx, q, y, "euclidean")
    D = _distances(ctx, qm, ym, "euclidean")
    with np.errstate(divide="ignore"):
        assert np.isinf(-0.02 * np.log(np.exp(-D / 0.02).sum(axis=1))).all()
    off = 1000.0 + 40.0 * rng.standard_normal(n_i)
    for o in (None, off):
        got = N.softmin_rows(ctx, qm, ym, 0.02, off=None if o is None else ctx.to_device(o), shift=3.0).numpy()
        assert np.isfinite(got).all()
        _assert_in_bracket(got, SR.softmin(D if o is None else D - o[None, :], 0.02, axis=1) + 3.0, 0.02, f"far from unit scale {np.dtype(dtype).name}")


def test_special_values_and_errors_at_the_abi(ctx):
    from kiez_amd import _native as N
    rng = np.random.default_rng(7)
    C = N.SOFTMIN_CHUNK
    n_q, n_i, eps = 33, C + 65, 0.05
    q, y = rng.standard_normal((n_q, 8)), rng.standard_normal((n_i, 8))
    qm, ym = _matrices(ctx, q, y, "euclidean")
    D = _distances(ctx, qm, ym, "euclidean")

    def run(off, shift=0.0, e=eps):
        return N.softmin_rows(ctx, qm, ym, e, off=ctx.to_device(off), shift=shift).numpy()
    # a NaN offset: that column is ignored -- here the column of row 0's nearest neighbour, and one in the other chunk
    off = 0.1 * rng.standard_normal(n_i)
    off[int(np.argmin(D[0]))] = off[C + 3] = np.nan
    keep = ~np.isnan(off)
    _assert_in_bracket(run(off, 2.0), SR.softmin((D - off[None, :])[:, keep], eps, axis=1) + 2.0, eps, "NaN offsets")
    # all offsets -inf: every term +inf
    np.testing.assert_array_equal(run(np.full(n_i, -np.inf), 2.0), np.full(n_q, np.inf))
    # a whole chunk of +inf terms beside a finite one: the finite chunk alone
    off = np.zeros(n_i)
    off[:C] = -np.inf
    _assert_in_bracket(run(off), SR.softmin(D[:, C:], eps, axis=1), eps, "first chunk +inf")
    # one offset +inf: one term -inf, in either chunk
    for col in (17, C + 17):
        off = 0.1 * rng.standard_normal(n_i)
        off[col] = np.inf
        np.testing.assert_array_equal(run(off, 2.0), np.full(n_q, -np.inf))
    # no rows: nothing to do
    assert N.softmin_rows(ctx, qm, ym, eps, q_begin=5, q_count=0).shape == (0,)
    # what the call refuses
    for bad in (0.0, -0.05, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="eps"):
            N.softmin_rows(ctx, qm, ym, bad)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="shift"):
            N.softmin_rows(ctx, qm, ym, eps, shift=bad)
    with pytest.raises(ValueError, match="different metrics"):
        N.softmin_rows(ctx, _matrices(ctx, q, y, "cosine")[0], ym, eps)
    with pytest.raises(ValueError, match="same dtype"):
        N.softmin_rows(ctx, _matrices(ctx, q.astype(np.float32), y, "euclidean")[0], ym, eps)
    with pytest.raises(ValueError, match="out of bounds"):
        N.softmin_rows(ctx, qm, ym, eps, q_begin=30, q_count=4)
    with pytest.raises(ValueError, match="off"):
        N.softmin_rows(ctx, qm, ym, eps, off=ctx.to_device(np.zeros(n_i - 1)))
    # kz_max_abs_diff: NaN differences are ignored
    a, b = rng.standard_normal(1000), rng.standard_normal(1000)
    a[3], b[4], a[5], b[5] = np.nan, np.nan, np.inf, np.inf
    with np.errstate(invalid="ignore"):
        assert N.max_abs_diff(ctx, ctx.to_device(a), ctx.to_device(b)) == np.nanmax(np.abs(a - b))
    assert N.max_abs_diff(ctx, ctx.to_device(a[3:5]), ctx.to_device(b[3:5])) == 0.0
    b[700] = -np.inf
    assert N.max_abs_diff(ctx, ctx.to_device(a), ctx.to_device(b)) == np.inf


def test_the_summation_tree_is_a_function_of_the_index_row_alone(ctx):
    """70 001 index rows (odd: the value rows of a batch start at both parities), 600 queries = two batches of values: the same bits
    from the whole call, from a second run, and from the rows [0, 299) and [299, 600) called apart -- the odd split moves every later
    row to the other alignment and to another place in its batch."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(70)
    n_q, n_i, eps = 600, 70_001, 0.05
    q, y = rng.standard_normal((n_q, 8)).astype(np.float32), rng.standard_normal((n_i, 8)).astype(np.float32)
    qm, ym = _matrices(ctx, q, y, "euclidean")
    off = ctx.to_device(0.3 * rng.standard_normal(n_i))
    assert n_q > (256 << 20) // (n_i * 8) > 299                 # two batches; the split lies inside the first
    for o in (off, None):
        whole = N.softmin_rows(ctx, qm, ym, eps, off=o, shift=0.5).numpy()
        again = N.softmin_rows(ctx, qm, ym, eps, off=o, shift=0.5).numpy()
        parts = np.concatenate([N.softmin_rows(ctx, qm, ym, eps, off=o, shift=0.5, q_begin=0, q_count=299).numpy(),
                                N.softmin_rows(ctx, qm, ym, eps, off=o, shift=0.5, q_begin=299, q_count=301).numpy()])
        assert np.isfinite(whole).all()
        np.testing.assert_array_equal(again.view(np.int64), whole.view(np.int64))
        np.testing.assert_array_equal(parts.view(np.int64), whole.view(np.int64))
    # (and the values are the restatement's: rows of both batches and their edge)
    rows = np.array([0, 1, 298, 299, 478, 479, 480, 599])
    D = _distances(ctx, _matrices(ctx, q[rows], y, "euclidean")[0], ym, "euclidean")
    _assert_in_bracket(whole[rows], SR.softmin(D, eps, axis=1) + 0.5, eps, "70 001 index rows")


def _potential_vectors(rng, n_q, n_i):
    """Random f and g with negative values, a NaN and both infinities on each side."""
    f, g = rng.standard_normal(n_q), rng.standard_normal(n_i)
    f[2], f[7], f[11] = np.nan, np.inf, -np.inf
    g[n_i // 3], g[n_i // 2], g[n_i - 1] = np.nan, np.inf, -np.inf
    g[0] = -np.inf if n_i > 1000 else g[0]                      # (two -inf: a tie at the head of every list)
    return f, g


@pytest.mark.parametrize("metric,dtype", [("euclidean", np.float32), ("cosine", np.float64)], ids=["euclidean_float32", "cosine_float64"])
def test_dual_kind_position_is_rank(ctx, metric, dtype):
    """kz_knn_reduced(kind = 8): the rank kz_gold_ranks_reduced gives the row at column c is c."""
    from kiez_amd import _native as N
    n_q = 96
    for n_i in (65, 4096, 4097):
        rng = np.random.default_rng(n_i)
        q, y = rng.standard_normal((n_q, 8)).astype(dtype), rng.standard_normal((n_i, 8)).astype(dtype)
        qm, ym = _matrices(ctx, q, y, metric)
        f, g = _potential_vectors(rng, n_q, n_i)
        f_dev, g_dev = ctx.to_device(f), ctx.to_device(g)
        for k in (1, 10, 64):
            w, ind = N.knn_reduced(ctx, qm, ym, k, N.RANK_DUAL, f_dev, g_dev)
            w, ind = w.numpy(), ind.numpy()
            where = f"{metric} n_i={n_i} k={k}"
            assert ((ind >= 0) & (ind < n_i)).all() and WI.non_decreasing(w), where
            for c in sorted({0, 1, k // 2, k - 1} & set(range(k))):
                rank = N.gold_ranks_reduced(ctx, qm, ym, ctx.to_device(np.ascontiguousarray(ind[:, c])), N.RANK_DUAL, f_dev, g_dev).numpy()
                np.testing.assert_array_equal(rank, np.full(n_q, c), err_msg=f"{where} column {c}")


@pytest.mark.parametrize("metric,p,dtype", CASES[:4], ids=CASE_IDS[:4])
def test_dual_kind_lists_are_the_sort_of_dual_shift_and_numpy(ctx, metric, p, dtype):
    """Lists over the whole index (K = n_index): kz_dual_shift's row by index id is numpy's (d - f) - g exactly, and the whole-index
    list is its sort by (value, row), bit for bit."""
    from kiez_amd import _native as N
    n_q = 120
    for n_i in (63, 65, 257):
        rng = np.random.default_rng(n_i)
        q, y = rng.standard_normal((n_q, 8)).astype(dtype), rng.standard_normal((n_i, 8)).astype(dtype)
        y[n_i - 2] = y[1]                                       # two identical index rows ...
        qm, ym = _matrices(ctx, q, y, metric, p)
        f, g = _potential_vectors(rng, n_q, n_i)
        g[n_i - 2] = g[1]                                       # ... with one potential: equal w
        f_dev, g_dev = ctx.to_device(f), ctx.to_device(g)
        dist, ind, _ = N.knn(ctx, qm, ym, n_i)
        w = N.dual_shift(ctx, dist, ind, f_dev, g_dev).numpy()
        dist, ind = dist.numpy(), ind.numpy()
        by_id, d_by_id = np.empty_like(w), np.empty_like(dist)
        np.put_along_axis(by_id, ind, w, axis=1)
        np.put_along_axis(d_by_id, ind, dist, axis=1)
        with np.errstate(invalid="ignore"):
            want = (d_by_id - f[:, None]) - g[None, :]
        real = ~np.isnan(want)
        np.testing.assert_array_equal(np.isnan(by_id), ~real)
        np.testing.assert_array_equal(by_id.view(np.int64)[real], want.view(np.int64)[real])
        assert (by_id[0, 1] == by_id[0, n_i - 2]) and (want < 0).any() and np.isinf(want).any() and (~real).any()
        for k in (1, 10, n_i):
            got_w, got_i = N.knn_reduced(ctx, qm, ym, k, N.RANK_DUAL, f_dev, g_dev)
            want_w, want_i = WI.topk(by_id, k)
            where = f"{metric} {np.dtype(dtype).name} n_i={n_i} k={k}"
            np.testing.assert_array_equal(got_i.numpy(), want_i, err_msg=where)
            keep = ~np.isnan(want_w)
            np.testing.assert_array_equal(np.isnan(got_w.numpy()), ~keep, err_msg=where)
            np.testing.assert_array_equal(got_w.numpy().view(np.int64)[keep], want_w.view(np.int64)[keep], err_msg=where)


def test_dual_kind_errors(ctx):
    from kiez_amd import _native as N
    rng = np.random.default_rng(5)
    q, y = rng.standard_normal((40, 8)), rng.standard_normal((70, 8))
    qm, ym = _matrices(ctx, q, y, "euclidean")
    f, g = ctx.to_device(rng.standard_normal(40)), ctx.to_device(rng.standard_normal(70))
    gold = ctx.to_device(rng.integers(0, 70, 40).astype(np.int64))
    for kind in (5, 6, 7, 0, 9, -1):
        with pytest.raises(ValueError, match="unknown kind"):
            N.gold_ranks_reduced(ctx, qm, ym, gold, kind, f, g)
        with pytest.raises(ValueError, match="unknown kind"):
            N.knn_reduced(ctx, qm, ym, 3, kind, f, g)
    with pytest.raises(ValueError, match="must be NULL"):
        N.gold_ranks_reduced(ctx, qm, ym, gold, N.RANK_DUAL, (f, f), (g, g))
    with pytest.raises(ValueError, match="must be NULL"):
        N.knn_reduced(ctx, qm, ym, 3, N.RANK_DUAL, (f, f), (g, g))
    assert N.gold_ranks_reduced(ctx, qm, ym, gold, N.RANK_DUAL, f, g).shape == (40,)
    with pytest.raises(ValueError, match="f must be a float64 device vector of shape \\(40,\\)"):
        N.dual_shift(ctx, ctx.empty((40, 3), np.float64), ctx.empty((40, 3), np.int64), g, g)
    with pytest.raises(ValueError, match="g must be a float64 device vector$"):
        N.dual_shift(ctx, ctx.empty((40, 3), np.float64), ctx.empty((40, 3), np.int64), f, ctx.empty((70, 1), np.float64))


# (n_s, n_t, eps, L, noise)
FIT_CASES = [(200, 200, 0.1, 50, 0.3), (180, 257, 0.05, 50, 0.3), (300, 300, 0.02, 100, 1.0)]


def _kiez(hubness, **kw):
    from kiez_amd import Kiez
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=hubness, hubness_kwargs=kw)


@pytest.fixture(scope="module")
def fit_cases():
    """Per case: the data, the device's own distances of all pairs and the restatement's potentials, once; read-only."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    out = {}
    for case in FIT_CASES:
        n_s, n_t, eps, L, noise = case
        s, t, gold = SR.alignment_case(n_s, n_t, noise)
        D = _distances(ctx, *_matrices(ctx, s, t, "cosine"), "cosine")
        f, g = SR.sinkhorn_potentials(D, eps, L)
        for a in (s, t, gold, D, f, g):
            a.setflags(write=False)
        out[case] = (s, t, gold, D, f, g)
    return out


@pytest.mark.parametrize("case", FIT_CASES, ids=[f"{c[0]}x{c[1]}_eps{c[2]}" for c in FIT_CASES])
def test_fit_against_the_restatement(fit_cases, case):
    from kiez_amd import Sinkhorn, matching
    n_s, n_t, eps, L, noise = case
    s, t, gold, D, f_want, g_want = fit_cases[case]
    kz = _kiez(Sinkhorn, temperature=eps, n_iter=L).fit(s, t)
    hub = kz.hubness
    assert hub.n_iter_ == L
    f, g = hub.source_potential_, hub.target_potential_
    assert f.shape == (n_s,) and g.shape == (n_t,) and f.dtype == g.dtype == np.float64
    _assert_in_bracket(f, f_want, eps, f"f after {L} iterations", factor=2 * L)
    _assert_in_bracket(g, g_want, eps, f"g after {L} iterations", factor=2 * L)
    # whole-index lists: the restatement's, except where its neighbouring w stand closer than twice the bracket
    W = SR.w(D, f_want, g_want)
    w_bracket = 2 * L * (SR.bracket(f_want, eps)[:, None] + SR.bracket(g_want, eps).max())
    want_w, want_i = WI.topk(W, 11)
    clear = (np.diff(want_w, axis=1) > 2 * w_bracket).all(axis=1)
    got_w, got_i = kz.kneighbors_whole_index(10)
    assert got_w.dtype == np.float64 and got_i.dtype == np.int64 and got_i.shape == (n_s, 10)
    print("rows whose first 11 restated values stand clear of each other:", int(clear.sum()), "of", n_s)
    assert clear.sum() >= 0.95 * n_s
    np.testing.assert_array_equal(got_i[clear], want_i[clear, :10])
    assert (np.abs(got_w - np.take_along_axis(W, got_i, axis=1)) <= w_bracket).all()
    # ... and exactly the sort of numpy's (D - f) - g over the device's own potentials
    np.testing.assert_array_equal(got_i, WI.topk(SR.w(D, f, g), 10)[1])
    # gold_ranks(reduced=True)[i] == c exactly when ind[i, c] == gold[i]
    rank = kz.gold_ranks(gold, reduced=True)
    listed = got_i == gold[:, None]
    assert listed.sum(axis=1).max() == 1 and listed.any(axis=1).mean() > 0.5
    np.testing.assert_array_equal(rank[listed.any(axis=1)], np.argmax(listed, axis=1)[listed.any(axis=1)])
    assert (rank[~listed.any(axis=1)] >= 10).all()
    # kneighbors(5) = the five best of the rescaled candidates
    nn = kz.algorithm
    cand_d, cand_i = nn.kneighbors_device(query=None, k=10)
    cand_w, _ = hub.transform(cand_d, cand_i, s)
    cand_w, cand_i = cand_w.numpy(), cand_i.numpy()
    np.testing.assert_array_equal(cand_w, (cand_d.numpy() - f[:, None]) - g[cand_i])
    order = np.argsort(cand_w, axis=1, kind="stable")[:, :5]
    d5, i5 = kz.kneighbors(5)
    np.testing.assert_array_equal(i5, np.take_along_axis(cand_i, order, axis=1))
    np.testing.assert_array_equal(d5, np.take_along_axis(cand_w, order, axis=1))
    # transform takes any caller's lists: ids that are no target row are refused, not read
    for bad in (-1, n_t):
        wrong = cand_i.copy()
        wrong[3, 2] = bad
        with pytest.raises(ValueError, match="neigh_ind holds ids"):
            hub.transform(cand_d.numpy(), wrong, s)
    with pytest.raises(ValueError, match="fitted source rows"):
        hub.transform(cand_d.numpy()[:-1], cand_i[:-1], s)
    # match(10, whole_index=True) = the stable matching over the whole-index lists
    m_dist, m_ind = kz.match(10, whole_index=True)
    want_dist, want_ind = matching.one_to_one(got_w, got_i, n_t)
    np.testing.assert_array_equal(m_ind, want_ind)
    np.testing.assert_array_equal(m_dist, want_dist)
    matched = m_ind[m_ind >= 0]
    assert len(set(matched.tolist())) == matched.size > 0.5 * n_s
    if case == FIT_CASES[0]:
        # the plan: the restatement's columns have converged (the guard), then the device potentials give the same plan
        P_want = np.exp(-W / eps)
        assert np.abs(P_want.sum(axis=0) - n_s / n_t).max() <= 1e-3
        P = np.exp(-SR.w(D, f, g) / eps)
        print("column sums off by", np.abs(P.sum(axis=0) - n_s / n_t).max(), "row sums off by", np.abs(P.sum(axis=1) - 1.0).max())
        assert np.abs(P.sum(axis=0) - n_s / n_t).max() <= 1e-3
        assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-9
    if case == FIT_CASES[2]:
        # a sanity line: Sinkhorn helps here (0.803 against 0.723 under the raw distance on the CPU); the device agrees with numpy
        hits_want, hits_raw = (W.argmin(axis=1) == gold).mean(), (D.argmin(axis=1) == gold).mean()
        print("hits@1: restated", hits_want, "raw distance", hits_raw, "device", (got_i[:, 0] == gold).mean())
        assert (got_i[:, 0] == gold).mean() == hits_want == (rank == 0).mean()


def test_inverted_softmax(fit_cases):
    from kiez_amd import InvertedSoftmax
    case = FIT_CASES[1]
    n_s, n_t, eps = case[:3]
    s, t, gold, D, _, _ = fit_cases[case]
    kz = _kiez(InvertedSoftmax, temperature=eps).fit(s, t)
    hub = kz.hubness
    f, g = hub.source_potential_, hub.target_potential_
    np.testing.assert_array_equal(f, np.zeros(n_s))
    _assert_in_bracket(g, SR.inverted_softmax_potential(D, eps), eps, "inverted softmax g")
    # the lists are ranked by d - g_j
    got_w, got_i = kz.kneighbors_whole_index(10)
    want_w, want_i = WI.topk(D - g[None, :], 10)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_w, want_w)
    rank = kz.gold_ranks(gold, reduced=True)
    np.testing.assert_array_equal(rank == 0, got_i[:, 0] == gold)
    d5, i5 = kz.kneighbors(5)
    assert i5.shape == (n_s, 5) and (np.diff(d5, axis=1) >= 0).all()


def test_early_stopping(ctx, fit_cases):
    from kiez_amd import Sinkhorn
    from kiez_amd import _native as N
    case = FIT_CASES[0]
    n_s, n_t, eps, L, _ = case
    s, t, gold, D, f_want, g_want = fit_cases[case]
    hub = _kiez(Sinkhorn, temperature=eps, n_iter=L, tol=1e-3).fit(s, t).hubness
    n = hub.n_iter_
    assert 2 <= n < L and hub.potential_change_ <= 1e-3
    # the change is kz_max_abs_diff of the last two column steps, and the stop was the first one possible
    before = _kiez(Sinkhorn, temperature=eps, n_iter=n - 1).fit(s, t).hubness
    same = _kiez(Sinkhorn, temperature=eps, n_iter=n).fit(s, t).hubness
    assert before.n_iter_ == n - 1 and same.n_iter_ == n
    assert hub.potential_change_ == N.max_abs_diff(ctx, same._g_dev, before._g_dev) == same.potential_change_
    assert hub.potential_change_ == np.abs(same.target_potential_ - before.target_potential_).max()
    assert n == 2 or before.potential_change_ > 1e-3
    # the row step behind the last column step was taken: the state is that of n whole iterations
    np.testing.assert_array_equal(hub.source_potential_, same.source_potential_)
    np.testing.assert_array_equal(hub.target_potential_, same.target_potential_)
    f_n, g_n = SR.sinkhorn_potentials(D, eps, n)
    _assert_in_bracket(hub.source_potential_, f_n, eps, f"f after {n} iterations", factor=2 * n)
    # tol = None runs exactly n_iter; tol = 0 is allowed and (here) never met
    assert _kiez(Sinkhorn, temperature=eps, n_iter=3).fit(s, t).hubness.n_iter_ == 3
    one = _kiez(Sinkhorn, temperature=eps, n_iter=1, tol=1e-3).fit(s, t).hubness
    assert one.n_iter_ == 1 and one.potential_change_ is None


TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd import Kiez, Sinkhorn
from tests import sinkhorn_restate as SR
s, t, gold = SR.alignment_case(200, 200, 0.3)
kw = dict(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=Sinkhorn)
kz = Kiez(hubness_kwargs={"temperature": 0.1, "n_iter": 5}, **kw).fit(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda())
d, i = kz.kneighbors_whole_index(10)
assert isinstance(d, torch.Tensor) and isinstance(i, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and i.dtype == torch.int64
d5, i5 = kz.kneighbors(5)
assert isinstance(d5, torch.Tensor) and d5.shape == (200, 5)
ref = Kiez(hubness_kwargs={"temperature": 0.1, "n_iter": 5}, **kw).fit(s, t)
rd, ri = ref.kneighbors_whole_index(10)
assert isinstance(rd, np.ndarray)
assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(d.cpu().numpy(), rd)
assert np.array_equal(kz.hubness.target_potential_, ref.hubness.target_potential_)
print("TORCH_OK")
"""


def test_tensors_in_tensors_out():
    """A fit on torch tensors returns tensors from kneighbors_whole_index: the inherited path (in a child process: torch must load
    its HIP runtime first)."""
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
