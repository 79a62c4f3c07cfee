"""The kernels of kiez_amd/csrc/kz_analysis.hip through the C ABI (ctx.lib, as kiez_amd/analysis.py calls them), each against its
restatement in tests/analysis_restate.py (validated on the CPU by tests/test_analysis_restate.py) at the sizes where a branch
changes: past one 1024-entry chunk of the single-workgroup scan (kz_kocc_select), past the cap of 1024 workgroups x 256 threads
= 262 144 threads of the grid-stride reductions (kz_minmax_i64, kz_minmax_i64_2d, kz_kocc_stats), around the 256-thread strided
loops of kz_max_abs_diff and kz_rank_stats, and with many workgroups on one histogram bin (kz_k_occurrence, kz_hit_positions).

Every integer result is compared with == / assert_array_equal.  A float sum S of n terms is held to
|got - fsum| <= 2 (n + 4) 2^-53 sum|term| (analysis_restate.sum_bound: the bound of a float64 summation in any order), and must
have the same bits from call to call: its order is fixed by construction."""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest

from tests import analysis_restate as AR

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = AR.INT64_MIN, AR.INT64_MAX
STRIDE = 1024 * 256                     # threads of a capped grid: element STRIDE is the first one of the second stride trip
MARKS = (0, 255, 256, STRIDE - 1, STRIDE, -1)


@pytest.fixture(scope="module")
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _check(rc, what):
    from kiez_amd import _native as N
    N._check(rc, what)


def _bits(x):
    return struct.pack("<d", float(x))


# ---- kz_kocc_select ---------------------------------------------------------------------------------------------------------
def _select(ctx, kocc, mode, thr):
    """(count, the whole output buffer): the buffer starts as -1 everywhere, so a write past `count` shows."""
    n = kocc.size
    d_kocc, d_out = ctx.to_device(kocc), ctx.to_device(np.full(n, -1, dtype=np.int64))
    cnt = C.c_int64(-1)
    _check(ctx.lib.kz_kocc_select(ctx.handle, d_kocc.ptr, n, mode, float(thr), d_out.ptr, C.byref(cnt)), "kz_kocc_select")
    return int(cnt.value), d_out.numpy()


def _select_masks(rng, n):
    idx = np.arange(n)
    last_chunk = ((n - 1) // 1024) * 1024
    return {
        "no hit": np.zeros(n, dtype=bool),
        "every entry": np.ones(n, dtype=bool),
        "last partial chunk only": idx >= last_chunk,
        "chunk positions 0 and 1023": (idx % 1024 == 0) | (idx % 1024 == 1023),
        "density 0.5": rng.random(n) < 0.5,
        "density 0.01": rng.random(n) < 0.01,
    }


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 70001])
def test_kocc_select_across_chunks(ctx, n):
    """The ordered scan carries its base from chunk to chunk: count and ids against np.flatnonzero, ascending, nothing written
    behind them.  Mode 1 with a non-integral threshold and with an integral one that entries equal exactly."""
    rng = np.random.default_rng(1000 + n)
    for what, mask in _select_masks(rng, n).items():
        for mode, thr in ((0, 7.5), (1, 7.5), (1, 8.0)):
            if mode == 0:
                kocc = np.where(mask, 0, rng.integers(1, 20, size=n))
            else:
                above = np.where(rng.random(n) < 0.5, math.ceil(thr), rng.integers(math.ceil(thr), 40, size=n))
                kocc = np.where(mask, above, rng.integers(0, 8, size=n))            # (7 < 7.5 and 7 < 8: no hit)
            kocc = kocc.astype(np.int64)
            want = AR.kocc_select(kocc, mode, thr)
            assert want.size == int(mask.sum()), (what, mode, thr)
            count, out = _select(ctx, kocc, mode, thr)
            assert count == want.size, (what, mode, thr)
            np.testing.assert_array_equal(out[:count], want, err_msg=f"{what}, mode {mode}, thr {thr}")
            assert np.all(np.diff(out[:count]) > 0)
            assert np.all(out[count:] == -1), (what, mode, thr)


# ---- kz_minmax_i64, kz_minmax_i64_2d ----------------------------------------------------------------------------------------
def _minmax_1d(ctx, a):
    d = ctx.to_device(a)
    lo, hi = C.c_int64(0), C.c_int64(0)
    _check(ctx.lib.kz_minmax_i64(ctx.handle, d.ptr, a.size, C.byref(lo), C.byref(hi)), "kz_minmax_i64")
    return int(lo.value), int(hi.value)


def _minmax_2d(ctx, m, k):
    d = ctx.to_device(m)
    lo, hi = C.c_int64(0), C.c_int64(0)
    _check(ctx.lib.kz_minmax_i64_2d(ctx.handle, d.ptr, m.shape[0], m.shape[1], k, C.byref(lo), C.byref(hi)), "kz_minmax_i64_2d")
    return int(lo.value), int(hi.value)


# count -> (rows, k) with rows * k == count, and the two widths: cols == k, cols > k
MINMAX_SHAPES = {1: (1, 1), 63: (9, 7), 65: (13, 5), 255: (51, 5), 256: (32, 8), 257: (257, 1), 262144: (32768, 8),
                 262145: (52429, 5), 600001: (600001, 1)}


@pytest.mark.parametrize("count", sorted(MINMAX_SHAPES))
def test_minmax_past_the_grid_cap(ctx, count):
    """INT64_MIN and INT64_MAX, each alone, at element 0, at the last element and at the first element of the second stride trip;
    the columns k.. of the 2-D call hold values beyond every extreme of the first k and must not be seen; consecutive calls on
    different data share one counter slot and must not carry over."""
    rows, k = MINMAX_SHAPES[count]
    assert rows * k == count
    rng = np.random.default_rng(2000 + count)
    base = rng.integers(-(1 << 40), 1 << 40, size=count)
    places = sorted({0, count - 1} | ({STRIDE} if count > STRIDE else set()))
    cases = [(None, None)] + [(pos, v) for pos in places for v in (I64_MIN, I64_MAX)]
    for pos, v in cases:
        a = base.copy()
        if pos is not None:
            a[pos] = v
        want = (int(a.min()), int(a.max()))
        assert AR.minmax(a.reshape(rows, k)) == want
        assert _minmax_1d(ctx, a) == want, (pos, v)
        assert _minmax_2d(ctx, a.reshape(rows, k), k) == want, ("k == cols", pos, v)
        wide = np.empty((rows, k + 2), dtype=np.int64)
        wide[:, :k] = a.reshape(rows, k)
        wide[:, k] = I64_MAX if v != I64_MAX else (1 << 62)        # beyond the extremes of the first k columns on both sides,
        wide[:, k + 1] = I64_MIN if v != I64_MIN else -(1 << 62)   # and never the value under test itself
        assert AR.minmax(wide, k) == want
        assert _minmax_2d(ctx, wide, k) == want, ("k < cols", pos, v)
    # a wide range, then a narrow one inside it, then a single value: nothing of the earlier call is left in the slot
    for a in (base, base % 1000, np.full(count, 5, dtype=np.int64)):
        assert _minmax_1d(ctx, a) == (int(a.min()), int(a.max()))
        assert _minmax_2d(ctx, a.reshape(rows, k), k) == (int(a.min()), int(a.max()))


# ---- kz_k_occurrence --------------------------------------------------------------------------------------------------------
def _k_occurrence(ctx, ind, k, n_bins):
    d_ind = ctx.to_device(ind)
    d_kocc = ctx.to_device(np.full(n_bins + 1, -7, dtype=np.int64))   # (the call clears n_bins entries; the one behind stays)
    _check(ctx.lib.kz_k_occurrence(ctx.handle, d_ind.ptr, ind.shape[0], ind.shape[1], k, n_bins, d_kocc.ptr), "kz_k_occurrence")
    out = d_kocc.numpy()
    assert out[n_bins] == -7
    return out[:n_bins]


@pytest.mark.parametrize(("n_rows", "cols", "k"), [(1, 1, 1), (257, 7, 3), (70001, 12, 10), (5000, 50, 50)])
@pytest.mark.parametrize("pattern", ["random", "one id", "negatives", "more bins than rows"])
def test_k_occurrence_against_bincount(ctx, n_rows, cols, k, pattern):
    rng = np.random.default_rng(3000 + n_rows)
    n_bins = n_rows + 1000 if pattern == "more bins than rows" else n_rows
    ind = rng.integers(0, n_bins, size=(n_rows, cols)).astype(np.int64)
    if pattern == "one id":
        ind[:] = n_bins // 2                                         # one bin takes n_rows * k increments
    if pattern == "negatives":
        ind[rng.random(ind.shape) < 0.3] = -1
        ind[0, 0] = I64_MIN
    if pattern != "one id" and n_rows > 1:
        ind[n_rows - 1, k - 1] = n_bins - 1                          # the last bin, from the last element of the first k columns
    ind[:, k:] = n_bins + 5                                          # dropped columns: ids that would be out of range
    want = AR.k_occurrence(ind, k, n_bins)
    assert int(want.sum()) == int(np.count_nonzero(ind[:, :k] >= 0))
    np.testing.assert_array_equal(_k_occurrence(ctx, ind, k, n_bins), want)


@pytest.mark.parametrize(("n_rows", "cols", "k"), [(1, 1, 1), (257, 7, 3), (70001, 12, 10), (5000, 50, 50)])
def test_k_occurrence_refuses_an_id_out_of_range(ctx, n_rows, cols, k):
    rng = np.random.default_rng(3500 + n_rows)
    n_bins = n_rows
    ind = rng.integers(0, n_bins, size=(n_rows, cols)).astype(np.int64)
    if k < cols:
        ind[n_rows - 1, k] = n_bins                                  # in a dropped column only: no error
        np.testing.assert_array_equal(_k_occurrence(ctx, ind, k, n_bins), AR.k_occurrence(ind, k, n_bins))
    ind[n_rows - 1, k - 1] = n_bins                                  # the last element of the first k columns, and only there
    with pytest.raises(ValueError, match="n_bins"):
        AR.k_occurrence(ind, k, n_bins)
    with pytest.raises(ValueError, match="neighbour id >= n_bins"):
        _k_occurrence(ctx, ind, k, n_bins)
    ind[n_rows - 1, k - 1] = n_bins - 1                              # the flag does not outlive the call
    np.testing.assert_array_equal(_k_occurrence(ctx, ind, k, n_bins), AR.k_occurrence(ind, k, n_bins))


# ---- kz_kocc_stats ----------------------------------------------------------------------------------------------------------
def _marks(n):
    return sorted({e if e >= 0 else n + e for e in MARKS if e < n})


@functools.lru_cache(maxsize=None)
def _heavy_tailed(n):
    """A heavy-tailed histogram -- bincount of min(floor(50 pareto(1.2)), n - 1) drawn 10 n times -- whose elements 0, 255, 256,
    262 143, 262 144 and n - 1 hold distinct values of their own (3001, 3500, ...), far from the mean of about 10."""
    rng = np.random.default_rng(4000 + n)
    draws = np.minimum(np.floor(50.0 * rng.pareto(1.2, size=10 * n)), n - 1).astype(np.int64)
    kocc = np.bincount(draws, minlength=n).astype(np.int64)
    for j, e in enumerate(_marks(n)):
        kocc[e] = 3001 + 499 * j
    kocc.setflags(write=False)
    return kocc


@functools.lru_cache(maxsize=None)
def _stats_want(n, thr_is_max, with_gini):
    kocc = _heavy_tailed(n)
    return AR.kocc_stats(kocc, float(kocc.max()) if thr_is_max else 7.5, with_gini=with_gini)


def _kocc_stats(ctx, d_kocc, n, thr, with_gini):
    st = (C.c_double * 10)(*([-1.0] * 10))
    _check(ctx.lib.kz_kocc_stats(ctx.handle, d_kocc.ptr, n, float(thr), int(with_gini), st), "kz_kocc_stats")
    return dict(zip(AR.STAT_ORDER, (float(x) for x in st)))


def _assert_stats(got, want, n, with_gini):
    for key in ("total", "kmax", "n_zero", "hub_sum", "n_hub"):
        assert want[key] < 1 << 53 and got[key] == want[key], key     # (a double holds these integers exactly)
    assert got["gini_num"] == (want["gini_num"] if with_gini else 0)
    for key in AR.FLOAT_SUMS:
        bound = AR.sum_bound(n, want["abs_terms"][key])
        err = abs(got[key] - want[key])
        print(f"n={n} {key}: got {got[key]!r} fsum {want[key]!r} |err| {err:.3e} bound {bound:.3e}")
        assert err <= bound, key


STATS_N = [1, 255, 257, 5000, 262144, 262145, 600001]


@pytest.mark.parametrize("n", STATS_N)
def test_kocc_stats_bound_is_sharp_enough(n):
    """On the CPU side: a kernel that skips one of the marked elements cannot pass.  For every float sum, the restatement without
    that element differs from the full one by more than ten times the bound the device is held to.  (n = 1: the only element is
    its own mean, the three centred terms are exactly 0 and only sum sqrt(x) can tell.)"""
    kocc = _heavy_tailed(n)
    want = _stats_want(n, False, False)
    terms = AR.kocc_float_terms(kocc, want["mean"])
    for key in AR.FLOAT_SUMS if n > 1 else ("sqrt_sum",):
        bound = AR.sum_bound(n, want["abs_terms"][key])
        for e in _marks(n):
            without = math.fsum(np.delete(terms[key], e))
            assert abs(want[key] - without) > 10.0 * bound, (key, e)
    values = [int(kocc[e]) for e in _marks(n)]
    assert len(set(values)) == len(values) and min(values) > 0
    print(n, {key: AR.sum_bound(n, want["abs_terms"][key]) for key in AR.FLOAT_SUMS})


@pytest.mark.parametrize("n", STATS_N)
def test_kocc_stats_past_the_grid_cap(ctx, n):
    """Integer outputs exact -- the hub sum and count at the non-integral threshold 7.5 and at max(kocc), which one entry equals --
    and each float sum inside the derived bound."""
    kocc = _heavy_tailed(n)
    d_kocc = ctx.to_device(kocc)
    _assert_stats(_kocc_stats(ctx, d_kocc, n, 7.5, 0), _stats_want(n, False, False), n, False)
    want = _stats_want(n, True, False)
    assert want["n_hub"] >= 1
    _assert_stats(_kocc_stats(ctx, d_kocc, n, float(kocc.max()), 0), want, n, False)


# kz_gini_kernel is O(n^2).  Its stride loop starts at n = 262 145: one kz_kocc_stats call with the Gini numerator took 0.037 s
# there and 0.143 s at n = 600 001 on an MI355X (one call each, host clock around the synchronising call) -- far below the two
# seconds a case may cost, so the smallest size that reaches the loop is part of the test.
@pytest.mark.parametrize("n", [1, 257, 5000, 20001, 262145])
def test_gini_numerator_is_exact(ctx, n):
    kocc = _heavy_tailed(n)
    want = _stats_want(n, False, True)
    assert 0 <= want["gini_num"] < 1 << 53
    _assert_stats(_kocc_stats(ctx, ctx.to_device(kocc), n, 7.5, 1), want, n, True)


@pytest.mark.parametrize("n", [600001, 300])
def test_kocc_stats_same_bits_every_call(ctx, n):
    """The float sums have no atomic in them: three calls on one histogram return the same ten doubles bit for bit.  n = 300 is
    the shape tests/test_gpu_analysis.py::test_device_input_from_the_hot_path compares two calls on (two workgroups)."""
    kocc = _heavy_tailed(n)
    d_kocc = ctx.to_device(kocc)
    calls = [_kocc_stats(ctx, d_kocc, n, 7.5, 0) for _ in range(3)]
    first = [_bits(calls[0][key]) for key in AR.STAT_ORDER]
    for other in calls[1:]:
        assert [_bits(other[key]) for key in AR.STAT_ORDER] == first
    # ... and on a second copy of the histogram at another address
    d_copy = ctx.to_device(kocc.copy())
    assert [_bits(v) for v in _kocc_stats(ctx, d_copy, n, 7.5, 0).values()] == first


# ---- kz_hit_positions -------------------------------------------------------------------------------------------------------
def _hit_positions(ctx, ind, gold):
    cols = ind.shape[1]
    d_ind, d_gold = ctx.to_device(ind), ctx.to_device(gold)
    d_hist = ctx.to_device(np.full(cols + 2, -7, dtype=np.int64))     # (the call clears cols + 1 entries; the one behind stays)
    _check(ctx.lib.kz_hit_positions(ctx.handle, d_ind.ptr, d_gold.ptr, ind.shape[0], cols, d_hist.ptr), "kz_hit_positions")
    out = d_hist.numpy()
    assert out[cols + 1] == -7
    return out[:cols + 1]


def _hit_case(n, cols, seed):
    """Rows by r % 6: gold in the first column / in the last / absent / there twice / no gold (INT64_MIN) / a random column."""
    rng = np.random.default_rng(seed)
    ind = rng.integers(0, 1 << 40, size=(n, cols)).astype(np.int64)
    r = np.arange(n)
    gold = ind[r, rng.integers(0, cols, size=n)].copy()
    kind = r % 6
    gold[kind == 0] = ind[kind == 0, 0]
    gold[kind == 1] = ind[kind == 1, cols - 1]
    gold[kind == 2] = (1 << 41) + r[kind == 2]                        # no neighbour id is that large
    if cols >= 3:
        twice = np.flatnonzero(kind == 3)
        first = rng.integers(0, cols - 1, size=twice.size)
        ind[twice, first] = ind[twice, cols - 1] = gold[twice] = (1 << 42) + twice
    gold[kind == 4] = AR.NO_GOLD
    return ind, gold


@pytest.mark.parametrize("cols", [1, 10, 100])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_hit_positions_against_argmax(ctx, n, cols):
    ind, gold = _hit_case(n, cols, 5000 + n + cols)
    want = AR.hit_positions(ind, gold)
    assert int(want.sum()) == int(np.count_nonzero(gold != AR.NO_GOLD))
    if n >= 255:
        assert want[0] > 0 and want[cols - 1] > 0 and want[cols] > 0
    np.testing.assert_array_equal(_hit_positions(ctx, ind, gold), want)
    # every row hits column 0: all the workgroups on one bin
    gold = ind[:, 0].copy()
    want = np.zeros(cols + 1, dtype=np.int64)
    want[0] = n
    np.testing.assert_array_equal(AR.hit_positions(ind, gold), want)
    np.testing.assert_array_equal(_hit_positions(ctx, ind, gold), want)


def test_hits_with_k_beyond_the_list(ctx):
    """evaluate.hits on 70 001 x 10 with k = [1, 5, 10, 25] (25 > cols counts the whole list), host and device input."""
    from kiez_amd.evaluate import hits
    n, cols = 70001, 10
    ind, gold = _hit_case(n, cols, 5500)
    gold_dict = {int(r): int(g) for r, g in enumerate(gold) if g != AR.NO_GOLD}
    gold_dict[n + 3] = 1                                              # a pair outside the matrix: denominator only
    hit = ind == gold[:, None]
    pos = np.where(hit.any(axis=1) & (gold != AR.NO_GOLD), hit.argmax(axis=1), cols)
    want = {kk: int(np.count_nonzero(pos < min(kk, cols))) / len(gold_dict) for kk in (1, 5, 10, 25)}
    assert 0.0 < want[1] < want[5] < want[10] == want[25] < 1.0
    assert hits(ind, gold_dict, [1, 5, 10, 25]) == want
    assert hits(ctx.to_device(ind), gold_dict, [25, 10, 5, 1]) == want


# ---- kz_max_abs_diff, kz_rank_stats -----------------------------------------------------------------------------------------
def _max_abs_diff(ctx, a, b):
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    h = C.c_double(-1.0)
    _check(ctx.lib.kz_max_abs_diff(ctx.handle, d_a.ptr, d_b.ptr, a.size, C.byref(h)), "kz_max_abs_diff")
    return float(h.value)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_max_abs_diff_strided_tail(ctx, n):
    rng = np.random.default_rng(6000 + n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    assert _max_abs_diff(ctx, a, b) == AR.max_abs_diff(a, b) == float(np.abs(a - b).max())
    a[n - 1], b[n - 1] = 50.0, -50.25                                 # the maximum in the last element
    assert _max_abs_diff(ctx, a, b) == AR.max_abs_diff(a, b) == 100.25
    # inf - inf (NaN) entries mixed in, the last element among them: ignored
    nan_at = rng.random(n) < 0.3
    nan_at[n - 1] = True
    a2, b2 = np.where(nan_at, np.inf, a), np.where(nan_at, np.inf, b)
    a2[n // 2], b2[n // 2] = (-np.inf, -np.inf) if nan_at[n // 2] else (a2[n // 2], b2[n // 2])
    want = AR.max_abs_diff(a2, b2)
    assert want == (float(np.abs(a - b)[~nan_at].max()) if not nan_at.all() else 0.0)
    assert _bits(_max_abs_diff(ctx, a2, b2)) == _bits(want)
    # all NaN: 0.0;  -0.0 against 0.0: +0.0
    assert _bits(_max_abs_diff(ctx, np.full(n, np.nan), b)) == _bits(0.0)
    assert _bits(_max_abs_diff(ctx, np.full(n, np.inf), np.full(n, np.inf))) == _bits(0.0)
    assert _bits(_max_abs_diff(ctx, np.full(n, -0.0), np.zeros(n))) == _bits(0.0) == _bits(AR.max_abs_diff([-0.0], [0.0]))
    # an infinite difference is a difference
    a[n - 1] = np.inf
    assert _max_abs_diff(ctx, a, b) == np.inf


def _rank_stats(ctx, rank, ks):
    d_rank = ctx.to_device(rank)
    n_k = len(ks)
    h_ks = (C.c_int64 * max(n_k, 1))(*[int(k) for k in ks])
    h_hits = (C.c_int64 * max(n_k, 1))(*([-1] * max(n_k, 1)))
    h_out = (C.c_double * 3)(-1.0, -1.0, -1.0)
    _check(ctx.lib.kz_rank_stats(ctx.handle, d_rank.ptr, rank.size, h_ks, n_k, h_hits, h_out), "kz_rank_stats")
    return [int(h_hits[j]) for j in range(n_k)], float(h_out[0]), float(h_out[1]), float(h_out[2])


def _assert_rank_stats(ctx, rank, ks):
    hits, n_ranked, pos_sum, recip, recip_abs = AR.rank_stats(rank, ks)
    got = _rank_stats(ctx, rank, ks)
    assert got[0] == hits
    assert pos_sum < 1 << 53 and (got[1], got[2]) == (n_ranked, pos_sum)
    bound = AR.sum_bound(n_ranked, recip_abs)
    print(f"n={rank.size} n_k={len(ks)}: sum 1/(rank+1) got {got[3]!r} fsum {recip!r} |err| {abs(got[3] - recip):.3e} bound {bound:.3e}")
    assert abs(got[3] - recip) <= bound
    again = _rank_stats(ctx, rank, ks)
    assert again[:3] == got[:3] and _bits(again[3]) == _bits(got[3])
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_rank_stats_strided_tail(ctx, n):
    rng = np.random.default_rng(7000 + n)
    rank = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 1000000, size=n)).astype(np.int64)
    rank[rng.random(n) < 0.2] = 0
    rank[rng.random(n) < 0.1] = 1
    rank[n - 1] = 0
    ks64 = [0, 1, 2, 1 << 62] + [int(v) for v in rng.integers(0, 1000000, size=60)]
    assert len(ks64) == 64
    for ks in ([0, 1, 1 << 62], ks64, []):
        _assert_rank_stats(ctx, rank, ks)
    # the only ranked entry is the last one
    only = np.full(n, -1, dtype=np.int64)
    only[n - 1] = 3
    assert _assert_rank_stats(ctx, only, [0, 1, 3, 4, 1 << 62]) == ([0, 0, 0, 1, 1], 1.0, 4.0, 0.25)
    # no ranked entry at all
    assert _assert_rank_stats(ctx, np.full(n, -1, dtype=np.int64), [1 << 62]) == ([0], 0.0, 0.0, 0.0)
    # 65 thresholds are refused
    with pytest.raises(ValueError, match="kz_rank_stats"):
        _rank_stats(ctx, rank, list(range(65)))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_hubness_score_with_more_bins_than_rows(ctx):
    """hubness_score on a 70 001 x 12 device matrix, k = 10, ids up to 89 999 in the first k columns (n_bins = 90 000 > n_train)
    and beyond in the dropped ones, against hubness_measures of the restated histogram.

    rel = 1e-9 on the four float-derived scalars: abs_dev, m2s and sqrt_sum are sums of non-negative terms, so the bound
    2 (n + 4) 2^-53 sum|t| is a RELATIVE error of 2 * 90 004 * 1.1e-16 = 2e-11 on each; m3s carries that times sum|t| / |S|, which
    the test holds below 2 (4e-11).  k_skewness = m3 / m2^1.5 adds 4e-11 + 1.5 * 2e-11 = 7e-11; the truncated-normal moment is a
    smooth function of a = -mean / std with |a| < 1 here (1e-11 on a, a condition number of a few); robinhood is one sum over an
    exact integer; atkinson = 1 - s^2 / mean has an absolute error of 2 * 2e-11 on a value above 0.1.  All below 1e-9 by a factor
    of ten, none close to what a dropped element or a float32 step would cost (1e-7 and up)."""
    from kiez_amd.analysis import hubness_score
    rng = np.random.default_rng(8000)
    n_train, cols, k, n_test = 70001, 12, 10, 90000
    ind = np.minimum(np.floor(n_test * rng.random((n_train, cols)) ** 3), n_test - 1).astype(np.int64)   # crowded towards id 0
    ind[rng.random(ind.shape) < 0.01] = -1
    ind[n_train - 1, k - 1] = n_test - 1
    ind[:, k:] += 5000                                                # ids up to 94 999 where nothing may look
    kocc = AR.k_occurrence(ind, k, n_test)
    assert AR.minmax(ind, k)[1] == n_test - 1 and AR.minmax(ind)[1] > n_test
    want = AR.hubness_measures(kocc, k, n_test, hub_size=2.0)
    st = AR.kocc_stats(kocc, 2.0 * k, with_gini=False)
    assert st["abs_terms"]["m3s"] <= 2.0 * abs(st["m3s"]) and want["atkinson"] > 0.1
    assert want["hubs"].size > 0 and want["antihubs"].size > 0
    got = hubness_score(ctx.to_device(ind), n_test, k=k, return_value="all", store_k_occurrence=True)
    assert set(got) == set(want)
    for key in ("k_occurrence", "hubs", "antihubs"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for key in ("antihub_occurrence", "hub_occurrence", "groupie_ratio", "gini"):
        assert got[key] == want[key], key
    for key in ("k_skewness", "k_skewness_truncnorm", "atkinson", "robinhood"):
        print(f"{key}: got {got[key]!r} want {want[key]!r}")
        assert got[key] == pytest.approx(want[key], rel=1e-9, abs=0.0), key
