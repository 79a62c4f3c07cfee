"""Every pair within a threshold over the whole index on the device (kz_radius_neighbors, kz_radius_neighbors_reduced and the
methods above them up to Kiez.radius_neighbors): with lists over the whole index the result is the threshold of the row `transform`
/ `kneighbors` writes, bit for bit, for every kind and four branches of the distance conversion (euclidean float32 / float64,
cosine, minkowski float32); the count, scan and fill passes around the chunk length and both parities of a value row's start; rows
of 9001 entries, beyond the LDS sort; NaN states; the capacity contract and the two-call allocation policy; batches and row ranges;
what the calls refuse; the facade.  The sort's size branches and key regimes, the scan beyond 256 chunks and the other conversions
and element types: tests/test_gpu_radius_sort.py.  `pytest -m gpu`."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import radius_restate as RA
from tests import reduced_rank_restate as RD
from tests import test_gpu_knn_reduced as KR
from tests import test_gpu_reduced_ranks as GR
from tests import whole_index_restate as WI

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

CONVERSION_IDS = KR.CONVERSION_IDS
KINDS = RD.KINDS + ("dual", "plain")      # kz_gold_ranks_reduced's four, KZ_RANK_DUAL, and kz_radius_neighbors itself


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _kind_id(kind):
    from kiez_amd import _native as N
    return None if kind == "plain" else N.RANK_DUAL if kind == "dual" else RD.kind_id(kind)


def _states(rng, kind, n):
    return None if kind == "plain" else KR._states(rng, "csls" if kind == "dual" else kind, n)


def _radius(ctx, qm, ym, radius, kind=None, q_state=None, t_state=None, **kw):
    """N.radius_neighbors -> numpy (indptr, ind, dist, total)."""
    from kiez_amd import _native as N
    indptr, ind, dist, total = N.radius_neighbors(ctx, qm, ym, radius, _kind_id(kind) if isinstance(kind, str) else kind, q_state, t_state, **kw)
    return indptr.numpy(), ind.numpy(), dist.numpy(), total


def _assert_csr(got, want, where, bits=True):
    """got (indptr, ind, dist, total) is the restatement's (indptr, ind, values): ids, and the values bit for bit."""
    indptr, ind, dist, total = got
    assert indptr.dtype == np.int64 and ind.dtype == np.int64 and dist.dtype == np.float64, where
    np.testing.assert_array_equal(indptr, want[0], err_msg=where)
    assert total == want[0][-1] == ind.size == dist.size, where
    np.testing.assert_array_equal(ind, want[1], err_msg=where)
    assert not np.isnan(dist).any(), where
    if bits:
        np.testing.assert_array_equal(dist.view(np.int64), want[2].view(np.int64), err_msg=f"{where} (bits)")


def _fitted(kind, n_t, metric, p, source, target):
    """(hub or None, nn, kind id, q_state, t_state, by_id): a reduction fitted with lists over the whole index and the [n_s, n_t] matrix
    of the values the device's own list calls return -- `transform`'s output row, or the distances of `kneighbors` (plain)."""
    from kiez_amd.hubness_reduction import Sinkhorn
    from kiez_amd.neighbors import SklearnNN
    if kind == "plain":
        hub, nn = None, SklearnNN(n_candidates=n_t, metric=metric, p=p)
        nn.fit(source, target)
    else:
        hub = Sinkhorn(temperature=0.5, n_iter=2, nn_algo=SklearnNN(n_candidates=n_t, metric=metric, p=p)) if kind == "dual" \
            else GR._reduction(kind, n_t, metric, p)
        hub.fit(source, target)
        nn = hub.nn_algo
    dist, ind = nn.kneighbors_device(query=None, k=n_t)
    if hub is None:
        kind_id = q_state = t_state = None
        w = dist
    else:
        kind_id, q_state, t_state = hub._forward_rank_state() if kind == "dual" else hub._rank_state(dist)
        w, _ = hub.transform(dist, ind, source)
    w, ind = w.numpy(), ind.numpy()
    by_id = np.empty_like(w)
    np.put_along_axis(by_id, ind, w, axis=1)
    return hub, nn, kind_id, q_state, t_state, by_id


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric,p,dtype", KR.CONVERSIONS, ids=CONVERSION_IDS)
def test_threshold_of_the_devices_own_lists_bit_for_bit(ctx, metric, p, dtype, kind):
    """n_candidates = n_target: `transform`'s output row (plain: the row of `kneighbors(k = n_target)`) holds w of every pair, and the
    radius result must be exactly {j : w_ij <= r} of it, ids and value bits, ties (two identical target rows) by row.  r comes from
    the data: the midpoint of a gap; exactly one pair's w, so that pair AND its tie are in (the rule is <=); below the minimum of
    half the rows, which are then empty; and +inf, which leaves out the NaN values only."""
    n_s, d = 96, 8
    for n_t in (63, 64, 65, 257):
        rng = np.random.default_rng(100 * n_t + d)
        source = rng.standard_normal((n_s, d)).astype(dtype)
        target = rng.standard_normal((n_t, d)).astype(dtype)
        target[n_t - 2] = target[1]                       # two identical index rows: equal distance, equal state, equal w
        source[1], source[3] = source[0], source[2]
        _, nn, kind_id, q_state, t_state, by_id = _fitted(kind, n_t, metric, p, source, target)
        tie = by_id[0, 1]
        assert tie == by_id[0, n_t - 2] or np.isnan(tie)
        radii = {"gap": RA.gap_radius(by_id, per_row=5, window=200)[0], "below half the row minima": float(np.median(np.nanmin(by_id, axis=1))),
                 "+inf": np.inf}
        if not np.isnan(tie):
            radii["one pair's own w"] = float(tie)
        for name, r in radii.items():
            for sort_results in (True, False):
                where = f"{kind} {metric} {np.dtype(dtype).name} n_target={n_t} radius {name} = {r!r} sorted={sort_results}"
                got = _radius(ctx, nn.source_index, nn.target_index, r, kind_id, q_state, t_state, sort_results=sort_results)
                want = RA.csr(by_id, r, sort_results)
                _assert_csr(got, want, where)
                counts = np.diff(got[0])
                if name == "one pair's own w":
                    row0 = got[1][:counts[0]]
                    assert 1 in row0 and n_t - 2 in row0, where
                    if sort_results:                          # the tie goes by row
                        assert list(row0).index(1) < list(row0).index(n_t - 2), where
                if name == "gap":
                    assert 2 * n_s <= counts.sum() <= 8 * n_s, where
                if name == "below half the row minima":
                    assert (counts == 0).sum() >= n_s // 2 - 2 and (counts > 0).any(), where
                if name == "+inf":
                    np.testing.assert_array_equal(counts, (~np.isnan(by_id)).sum(axis=1), err_msg=where)


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_and_parities(ctx, kind):
    """96 x n_index x 8 float64 euclidean, arbitrary positive states: one chunk; a full chunk of 8192; a one-entry last chunk; an odd
    row length of three chunks -- odd lengths start every other value row at an odd element.  The radius stands in a gap of
    numpy's w (about 20 pairs a row) that is asserted to be > 4e-12: device and numpy w differ by at most 1e-12 where exp / erfc
    are involved (tests/test_gpu_knn_reduced.py) and not at all for CSLS, NICDM, the dual form and the distances, so the ids are
    numpy's."""
    from kiez_amd import _native as N
    n_q, d = 96, 8
    for n_i in (65, 8192, 8193, 20_500):
        rng = np.random.default_rng(n_i)
        q, y = rng.standard_normal((n_q, d)), rng.standard_normal((n_i, d))
        qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
        dist = np.sqrt(GR._all_pair_values(ctx, qm, ym))
        qs, ts = _states(rng, kind, n_q), _states(rng, kind, n_i)
        if kind == "plain":
            w, q_dev, t_dev = dist, None, None
        else:
            w = (dist - qs[0][:, None]) - ts[0][None, :] if kind == "dual" else RD.reduce(kind, dist, qs, ts)
            q_dev, t_dev = KR._dev(ctx, qs), KR._dev(ctx, ts)
        r, gap = RA.gap_radius(w, per_row=20)
        assert gap > 4e-12
        counts = np.diff(RA.csr(w, r)[0])
        assert 10 * n_q <= counts.sum() <= 30 * n_q and counts.max() > counts.min()
        exact = kind not in ("ls", "mp_normal")
        for sort_results in (True, False):
            where = f"{kind} n_index={n_i} sorted={sort_results}"
            got = _radius(ctx, qm, ym, r, kind, q_dev, t_dev, sort_results=sort_results)
            want = RA.csr(w, r, sort_results)
            np.testing.assert_array_equal(got[0], want[0], err_msg=where)
            if exact or not sort_results:
                _assert_csr(got, want, where, bits=exact)
            else:                                             # (values within 1e-12 of each other may swap places: the sets)
                for a, b in zip(RA.rows(got[0], got[1]), RA.rows(want[0], want[1])):
                    np.testing.assert_array_equal(np.sort(a), np.sort(b), err_msg=where)
            for ids, vals in zip(RA.rows(got[0], got[1]), RA.rows(got[0], got[2])):
                if sort_results:
                    assert (np.diff(vals) >= 0).all(), where
                    assert (np.diff(ids)[np.diff(vals) == 0] > 0).all(), where
                else:
                    assert (np.diff(ids) > 0).all(), where
            assert np.abs(got[2] - w[np.repeat(np.arange(n_q), np.diff(got[0])), got[1]]).max(initial=0.0) <= 1e-12, where


@pytest.mark.parametrize("kind", ["csls", "mp_normal"])
def test_consistent_with_the_list_and_the_rank_calls(ctx, kind):
    """A sorted row of at most 512 entries IS the head of kz_knn_reduced's list, ids and bits; and kz_gold_ranks_reduced(gold)[i] <
    count_i exactly when gold[i] is in row i."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(5)
    n_q, n_i, d = 200, 8193, 8
    q, y = rng.standard_normal((n_q, d)).astype(np.float32), rng.standard_normal((n_i, d)).astype(np.float32)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    q_state, t_state = KR._dev(ctx, KR._states(rng, kind, n_q)), KR._dev(ctx, KR._states(rng, kind, n_i))
    list_w, list_i = N.knn_reduced(ctx, qm, ym, 512, RD.kind_id(kind), q_state, t_state)
    list_w, list_i = list_w.numpy(), list_i.numpy()
    gold = rng.integers(0, n_i, n_q).astype(np.int64)
    gold[::2] = list_i[::2, rng.integers(0, 40)]          # half of them near the head of the list
    rank = N.gold_ranks_reduced(ctx, qm, ym, ctx.to_device(gold), RD.kind_id(kind), q_state, t_state).numpy()
    for r in (float(np.median(list_w[:, 400])), float(np.median(list_w[:, 20]))):
        indptr, ind, dist, _ = _radius(ctx, qm, ym, r, kind, q_state, t_state)
        counts = np.diff(indptr)
        short = np.flatnonzero(counts <= 512)
        assert short.size >= n_q // 4 and counts.max() > 0
        for i in short:
            np.testing.assert_array_equal(ind[indptr[i]:indptr[i + 1]], list_i[i, :counts[i]], err_msg=f"{kind} radius {r} row {i}")
            np.testing.assert_array_equal(dist[indptr[i]:indptr[i + 1]].view(np.int64), list_w[i, :counts[i]].view(np.int64))
        inside = np.array([gold[i] in ind[indptr[i]:indptr[i + 1]] for i in range(n_q)])
        np.testing.assert_array_equal(rank < counts, inside)
        assert inside.any()
    assert not inside.all()


@pytest.mark.parametrize("kind", ["csls", "plain"])
def test_rows_that_hold_the_whole_index(ctx, kind):
    """3 x 9001 with radius = +inf: every row holds all 9001 index rows, beyond any LDS sort; signs mix under CSLS (index-side state
    in [-5, 15)), and ten copies of one index row tie by row.  float64 euclidean: numpy has the bits of sqrt and of 2 d - a - b.
    Then one NaN state: that index row is absent from every row."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(9001)
    n_q, n_i, d = 3, 9001, 8
    q, y = rng.standard_normal((n_q, d)), rng.standard_normal((n_i, d))
    copies = np.array([3, 17, 1000, 2048, 4095, 4096, 4097, 8191, 8192, 9000])
    y[copies] = y[3]
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    dist = np.sqrt(GR._all_pair_values(ctx, qm, ym))
    q_a, t_a = rng.random(n_q) + 0.5, rng.uniform(-5.0, 15.0, n_i)
    t_a[copies] = t_a[3]
    plant = 1234
    for t_state in ((t_a,), (np.where(np.arange(n_i) == plant, np.nan, t_a),)):
        if kind == "plain":
            w, q_dev, t_dev = dist, None, None
        else:
            w, q_dev, t_dev = RD.reduce("csls", dist, (q_a,), t_state), KR._dev(ctx, (q_a,)), KR._dev(ctx, t_state)
            assert (w[~np.isnan(w)] < 0).any() and (w[~np.isnan(w)] > 0).any()
        n_row = n_i - int(np.isnan(w[0]).sum())
        for sort_results in (True, False):
            where = f"{kind} sorted={sort_results} rows of {n_row}"
            got = _radius(ctx, qm, ym, np.inf, kind, q_dev, t_dev, sort_results=sort_results)
            _assert_csr(got, RA.csr(w, np.inf, sort_results), where)
            np.testing.assert_array_equal(got[0], n_row * np.arange(n_q + 1), err_msg=where)
            if sort_results:
                want_w, want_i = WI.topk(w, n_row)            # (the whole-index list's own order, NaN last: cut before it)
                np.testing.assert_array_equal(got[1].reshape(n_q, n_row), want_i, err_msg=where)
                for row in got[1].reshape(n_q, n_row):
                    at = np.flatnonzero(np.isin(row, copies))
                    assert (np.diff(at) == 1).all(), where
                    np.testing.assert_array_equal(row[at], copies, err_msg=where)
            if n_row < n_i:
                assert plant not in got[1], where
        if kind == "plain":
            break                                             # (no state to plant a NaN in)


def test_capacity_and_the_allocation_policy(ctx):
    from kiez_amd import _native as N
    rng = np.random.default_rng(32)
    n_q, n_i, d = 50, 3000, 8
    q, y = rng.standard_normal((n_q, d)), rng.standard_normal((n_i, d))
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    dist = np.sqrt(GR._all_pair_values(ctx, qm, ym))
    q_a, t_a = rng.random(n_q) + 0.5, rng.random(n_i) + 0.5
    q_dev, t_dev = ctx.to_device(q_a), ctx.to_device(t_a)
    w = RD.reduce("csls", dist, (q_a,), (t_a,))
    for kind, values, state in (("plain", dist, (None, None)), ("csls", w, (q_dev, t_dev))):
        # about 20 pairs a row: the first call of the policy holds them
        r, _ = RA.gap_radius(values, per_row=20)
        want = RA.csr(values, r)
        assert 10 * n_q <= want[0][-1] <= N.RADIUS_FIRST_CAPACITY_PER_ROW * n_q
        _assert_csr(_radius(ctx, qm, ym, r, kind, *state), want, f"{kind} first call")
        # capacity 0: the counts alone, and radius_counts
        indptr0, ind0, dist0, total0 = _radius(ctx, qm, ym, r, kind, *state, capacity=0)
        np.testing.assert_array_equal(indptr0, want[0])
        assert total0 == want[0][-1] and ind0.size == dist0.size == 0
        c_indptr, c_total = N.radius_counts(ctx, qm, ym, r, _kind_id(kind), *state)
        np.testing.assert_array_equal(c_indptr.numpy(), want[0])
        assert c_total == total0
        # a capacity that ends inside row `cut`: the rows before it complete, indptr and total exact
        cut = n_q // 2
        while want[0][cut + 1] == want[0][cut]:
            cut += 1
        capacity = int(want[0][cut]) + 1 if want[0][cut + 1] - want[0][cut] > 1 else int(want[0][cut])
        assert want[0][cut] <= capacity < want[0][cut + 1] or capacity == want[0][cut]
        for sort_results in (True, False):
            indptr, ind, dist_c, total = _radius(ctx, qm, ym, r, kind, *state, capacity=capacity, sort_results=sort_results)
            full = RA.csr(values, r, sort_results)
            np.testing.assert_array_equal(indptr, full[0])
            assert total == full[0][-1] and ind.size == dist_c.size == capacity
            done = int(full[0][cut])
            np.testing.assert_array_equal(ind[:done], full[1][:done])
            np.testing.assert_array_equal(dist_c[:done].view(np.int64), full[2][:done].view(np.int64))
        # more than 32 pairs a row: the policy's second call, with the exact allocation
        r, _ = RA.gap_radius(values, per_row=80)
        want = RA.csr(values, r)
        assert want[0][-1] > N.RADIUS_FIRST_CAPACITY_PER_ROW * n_q
        for sort_results in (True, False):
            _assert_csr(_radius(ctx, qm, ym, r, kind, *state, sort_results=sort_results), RA.csr(values, r, sort_results), f"{kind} second call")
    with pytest.raises(ValueError, match="capacity"):
        N.radius_neighbors(ctx, qm, ym, 1.0, capacity=-1)


def test_batches_row_ranges_and_refusals(ctx):
    """70 000 index rows: 479 rows of values per batch of the exact stage, 1 000 query rows in three batches; the pieces of the call
    over row ranges -- cut at, before and behind a batch edge -- concatenated are the single call, bit for bit."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(70)
    n_q, n_i, d = 1000, 70_000, 8
    q, y = rng.standard_normal((n_q, d)).astype(np.float32), rng.standard_normal((n_i, d)).astype(np.float32)
    q_a, t_a = rng.random(n_q) + 0.5, rng.random(n_i) + 0.5
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    t_dev = ctx.to_device(t_a)
    list_w, list_i = N.knn_reduced(ctx, qm, ym, 10, N.RANK_CSLS, ctx.to_device(q_a), t_dev)
    list_w, list_i = list_w.numpy(), list_i.numpy()
    r = float(np.median(list_w[:, 9]))                        # about half the rows hold ten pairs or more

    def call(begin, count, **kw):
        return _radius(ctx, qm, ym, r, N.RANK_CSLS, ctx.to_device(q_a[begin:begin + count]), t_dev, q_begin=begin, q_count=count, **kw)
    for sort_results in (True, False):
        indptr, ind, dist, total = call(0, n_q, sort_results=sort_results)
        counts = np.diff(indptr)
        assert total == ind.size == indptr[-1] and counts.min() < 10 <= counts.max()
        for cuts in ((0, 500, 1000), (0, 479, 1000), (0, 300, 480, 1000)):
            parts = [call(b, e - b, sort_results=sort_results) for b, e in zip(cuts[:-1], cuts[1:])]
            assert sum(p[3] for p in parts) == total
            np.testing.assert_array_equal(np.concatenate([p[0][1:] - p[0][:-1] for p in parts]), counts)
            assert all(p[0][0] == 0 for p in parts)
            np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), ind)
            np.testing.assert_array_equal(np.concatenate([p[2] for p in parts]).view(np.int64), dist.view(np.int64))
        again = call(0, n_q, sort_results=sort_results)       # (and the same from call to call)
        np.testing.assert_array_equal(again[1], ind)
        np.testing.assert_array_equal(again[2].view(np.int64), dist.view(np.int64))
        if sort_results:                                      # rows of both batches' edges against the list call
            for i in (0, 478, 479, 480, 957, 958, 959, 999):
                head = min(counts[i], 10)
                np.testing.assert_array_equal(ind[indptr[i]:indptr[i] + head], list_i[i, :head])
                np.testing.assert_array_equal(dist[indptr[i]:indptr[i] + head].view(np.int64), list_w[i, :head].view(np.int64))
                assert counts[i] == (list_w[i] <= r).sum() or counts[i] > 10
    # what the calls refuse
    q_dev = ctx.to_device(q_a)
    with pytest.raises(ValueError, match="NaN"):
        N.radius_neighbors(ctx, qm, ym, float("nan"), N.RANK_CSLS, q_dev, t_dev)
    with pytest.raises(ValueError, match="radius is NaN"):       # (the library's own refusal, behind the host's)
        N._radius_call(ctx, qm, ym, float("nan"), True, 0, None, None, 0, n_q)
    with pytest.raises(ValueError, match="radius is NaN"):
        N._radius_call(ctx, qm, ym, float("nan"), True, 0, N.RANK_CSLS, (q_dev.ptr, None, t_dev.ptr, None), 0, n_q)
    with pytest.raises(ValueError, match="are required"):
        N.radius_neighbors(ctx, qm, ym, r, N.RANK_CSLS)
    with pytest.raises(ValueError, match="name its kind"):
        N.radius_neighbors(ctx, qm, ym, r, None, q_dev, t_dev)
    with pytest.raises(ValueError, match="unknown kind"):
        N.radius_neighbors(ctx, qm, ym, r, 5, q_dev, t_dev)
    with pytest.raises(ValueError, match="KZ_RANK_MP_NORMAL needs"):
        N.radius_neighbors(ctx, qm, ym, r, N.RANK_MP_NORMAL, q_dev, t_dev)
    with pytest.raises(ValueError, match="must be NULL"):
        N.radius_neighbors(ctx, qm, ym, r, N.RANK_NICDM, (q_dev, q_dev), (t_dev, t_dev))
    with pytest.raises(ValueError, match="different metrics"):
        N.radius_neighbors(ctx, N.DeviceMatrix(ctx, q, "cosine"), ym, r)
    with pytest.raises(ValueError, match="out of bounds"):
        N.radius_neighbors(ctx, qm, ym, r, q_begin=990, q_count=11)
    indptr, ind, dist, total = _radius(ctx, qm, ym, r, q_begin=5, q_count=0)     # an empty range: one offset
    assert indptr.tolist() == [0] and total == 0 and ind.size == dist.size == 0


def _kiez(hubness=None, metric="euclidean", n_candidates=10, **kw):
    from kiez_amd import Kiez
    return Kiez(n_candidates=n_candidates, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=kw or None)


def _assert_heads(res, counts_fn, list_dist, list_ind, radius):
    """The CSR `res` against lists of k columns by the same values: every row is the list's head, or longer than the list."""
    indptr, ind, dist = res
    k = list_ind.shape[1]
    counts = np.diff(indptr)
    assert indptr[0] == 0 and indptr[-1] == ind.size == dist.size and ind.dtype == indptr.dtype == np.int64
    assert dist.dtype == list_dist.dtype
    with np.errstate(invalid="ignore"):
        inside = (list_dist.astype(np.float64) <= radius).sum(axis=1)
    for i in range(len(counts)):
        head = min(counts[i], k)
        np.testing.assert_array_equal(ind[indptr[i]:indptr[i] + head], list_ind[i, :head], err_msg=f"row {i}")
        np.testing.assert_array_equal(dist[indptr[i]:indptr[i] + head], list_dist[i, :head], err_msg=f"row {i}")
    short = counts < k
    assert short.any() and (counts > 0).any()
    np.testing.assert_array_equal(counts[short], inside[short])
    np.testing.assert_array_equal(counts_fn(), counts)


def test_facade():
    from kiez_amd.neighbors import NotFittedError
    rng = np.random.default_rng(21)
    source = rng.standard_normal((300, 16)).astype(np.float32)
    target = np.concatenate([source + 0.6 * rng.standard_normal((300, 16)).astype(np.float32),
                             rng.standard_normal((100, 16)).astype(np.float32)])
    for hubness, kw in ((None, {}), ("CSLS", {}), ("LocalScaling", {"method": "nicdm"}), ("MutualProximity", {"method": "normal"})):
        kz = _kiez(hubness, **kw).fit(source, target)
        # under the search metric, whatever the reduction
        d50, i50 = kz.algorithm.kneighbors(k=50)
        r = float(np.median(d50[:, 9]))
        res = kz.radius_neighbors(r)
        assert all(isinstance(a, np.ndarray) for a in res) and res[2].dtype == np.float64 and res[0].shape == (301,)
        _assert_heads(res, lambda: kz.radius_counts(r), d50, i50, r)
        # under the reduced distances
        w50, j50 = kz.kneighbors_whole_index(50)
        rw = float(np.median(w50[:, 9]))
        res_w = kz.radius_neighbors(rw, reduced=True)
        _assert_heads(res_w, lambda: kz.radius_counts(rw, reduced=True), w50, j50, rw)
        if hubness == "MutualProximity":                   # a probability: "all pairs with MP <= 0.05" is a query
            indptr, ind, p = kz.radius_neighbors(0.05, reduced=True)
            assert ((p >= 0) & (p <= 0.05)).all() and ind.size == indptr[-1]
        # return_distance, sort_results, ragged
        indptr, ind = kz.radius_neighbors(rw, reduced=True, return_distance=False)
        np.testing.assert_array_equal(indptr, res_w[0])
        np.testing.assert_array_equal(ind, res_w[1])
        indptr_u, ind_u, w_u = kz.radius_neighbors(rw, reduced=True, sort_results=False)
        np.testing.assert_array_equal(indptr_u, res_w[0])
        for a, b in zip(RA.rows(indptr_u, ind_u), RA.rows(res_w[0], res_w[1])):
            assert (np.diff(a) > 0).all()
            np.testing.assert_array_equal(a, np.sort(b))
        rag_d, rag_i = kz.radius_neighbors(rw, reduced=True, ragged=True)
        assert rag_d.dtype == rag_i.dtype == object and rag_d.shape == rag_i.shape == (300,)
        for i in (0, 1, 150, 299):
            np.testing.assert_array_equal(rag_i[i], res_w[1][res_w[0][i]:res_w[0][i + 1]])
            np.testing.assert_array_equal(rag_d[i], res_w[2][res_w[0][i]:res_w[0][i + 1]])
        only_i = kz.radius_neighbors(rw, reduced=True, ragged=True, return_distance=False)
        assert only_i.dtype == object and all(np.array_equal(a, b) for a, b in zip(only_i, rag_i))
        d5, i5 = kz.kneighbors(5)                             # kneighbors afterwards is what it was
        fresh_d, fresh_i = _kiez(hubness, **kw).fit(source, target).kneighbors(5)
        np.testing.assert_array_equal(i5, fresh_i)
        np.testing.assert_array_equal(d5, fresh_d)
        # the device variants
        dev = kz.hubness.radius_neighbors_device(rw)
        for a, b in zip(dev, res_w):
            np.testing.assert_array_equal(a.numpy(), b)
        with pytest.raises(ValueError, match="NaN"):
            kz.radius_neighbors(float("nan"))
        with pytest.raises(TypeError, match="real number"):
            kz.radius_counts(True)
    # the reverse direction exists under the search metric only
    kz = _kiez("CSLS").fit(source, target)
    d_ts, i_ts = kz.algorithm.kneighbors(k=50, s_to_t=False)
    r = float(np.median(d_ts[:, 9]))
    _assert_heads(kz.algorithm.radius_neighbors(r, s_to_t=False), lambda: kz.algorithm.radius_counts(r, s_to_t=False), d_ts, i_ts, r)
    with pytest.raises(ValueError, match="s_to_t=True"):
        kz.hubness.radius_neighbors(r, s_to_t=False)
    # float32 cosine: float32 values, rounded after the comparison
    kz = _kiez("CSLS", metric="cosine").fit(source, target)
    d50, i50 = kz.algorithm.kneighbors(k=50)
    assert d50.dtype == np.float32
    r = float(np.median(d50[:, 9].astype(np.float64)))
    res = kz.radius_neighbors(r)
    assert res[2].dtype == np.float32
    counts = np.diff(res[0])
    for i in range(300):
        head = min(counts[i], 50)
        np.testing.assert_array_equal(res[1][res[0][i]:res[0][i] + head], i50[i, :head])
        np.testing.assert_array_equal(res[2][res[0][i]:res[0][i] + head], d50[i, :head])
    assert kz.radius_neighbors(float(np.median(kz.kneighbors_whole_index(10)[0][:, 9])), reduced=True)[2].dtype == np.float32
    # metric="precomputed": the matrix' own entries
    D = np.abs(rng.standard_normal((120, 90)))
    kz = _kiez("CSLS", metric="precomputed", n_candidates=6).fit(D)
    r = float(np.median(np.sort(D, axis=1)[:, 7]))
    want = RA.csr(D, r)
    for got, exp in zip(kz.radius_neighbors(r), want):
        np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(kz.radius_counts(r), np.diff(want[0]))
    w20, j20 = kz.kneighbors_whole_index(20)
    rw = float(np.median(w20[:, 5]))
    _assert_heads(kz.radius_neighbors(rw, reduced=True), lambda: kz.radius_counts(rw, reduced=True), w20, j20, rw)
    # a boolean metric: few distinct values, long ties by row, NaN-free
    bs, bt = (rng.random((100, 24)) < 0.3).astype(np.float32), (rng.random((150, 24)) < 0.3).astype(np.float32)
    kz = _kiez(None, metric="jaccard").fit(bs, bt)
    d_all, i_all = kz.algorithm.kneighbors(k=150)
    r = float(np.median(d_all[:, 9]))
    _assert_heads(kz.radius_neighbors(r), lambda: kz.radius_counts(r), d_all, i_all, r)
    # what the facade refuses
    for hubness, kw in (("MutualProximity", {"method": "empiric"}), ("DisSimLocal", {})):
        kz = _kiez(hubness, **kw).fit(source, target)
        with pytest.raises(NotImplementedError, match="outside the list"):
            kz.radius_neighbors(1.0, reduced=True)
        with pytest.raises(NotImplementedError, match="outside the list"):
            kz.radius_counts(1.0, reduced=True)
        assert kz.radius_neighbors(float(np.median(kz.algorithm.kneighbors(k=10)[0][:, 5])))[1].size > 0   # (the plain call is served)
    for reduced in (False, True):
        with pytest.raises(NotImplementedError, match="two-sided"):
            _kiez("CSLS").fit(source).radius_neighbors(1.0, reduced=reduced)
        with pytest.raises(NotImplementedError, match="two-sided"):
            _kiez("CSLS").fit(source).radius_counts(1.0, reduced=reduced)
        with pytest.raises(NotFittedError):
            _kiez("CSLS").radius_neighbors(1.0, reduced=reduced)


TENSOR_SCRIPT = r"""
import sys, warnings
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd import Kiez
warnings.simplefilter("ignore")
rng = np.random.default_rng(3)
s, t = rng.random((200, 16)).astype(np.float32), rng.random((260, 16)).astype(np.float32)
def kiez():
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
base = kiez().fit(s, t)
r = float(np.median(base.kneighbors_whole_index(10)[0][:, 9]))
want = base.radius_neighbors(r, reduced=True)
want_plain = base.radius_neighbors(1.0)
for dev in ("cuda", "cpu"):
    kz = kiez().fit(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev))
    for got, exp in ((kz.radius_neighbors(r, reduced=True), want), (kz.radius_neighbors(1.0), want_plain)):
        assert all(isinstance(a, torch.Tensor) and a.device.type == dev for a in got), [type(a) for a in got]
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float64
        for a, b in zip(got, exp):
            assert np.array_equal(a.cpu().numpy(), b), dev
    counts = kz.radius_counts(r, reduced=True)
    assert isinstance(counts, torch.Tensor) and np.array_equal(counts.cpu().numpy(), np.diff(want[0]))
    rag_d, rag_i = kz.radius_neighbors(r, reduced=True, ragged=True)
    assert rag_i.dtype == object and np.array_equal(rag_i[7], want[1][want[0][7]:want[0][8]])
    empty = kz.radius_neighbors(-1e9, reduced=True)
    assert empty[1].numel() == 0 and empty[2].numel() == 0 and int(empty[0].abs().sum()) == 0
print("RADIUS_TENSORS_OK")
"""


def test_fitted_on_tensors_subprocess():
    """Tensors in, tensors out on the source's device (torch has to be imported before the library is loaded: a process of its own)."""
    r = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RADIUS_TENSORS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
