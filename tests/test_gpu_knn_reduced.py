"""Neighbour lists by the hubness-reduced distance over the whole index on the device (kz_knn_reduced,
HubnessReduction.kneighbors_whole_index, Kiez.kneighbors_whole_index): position in the list is the rank kz_gold_ranks_reduced gives,
for every kind and every branch of the distance conversion, over one chunk, a full chunk, a one-entry last chunk and a last chunk
shorter than k; with lists over the whole index the list is the sort of `transform`'s output, bit for bit; with short lists it is
the numpy restatement (tests/whole_index_restate.py) -- exactly where numpy reproduces the bits, inside 1e-12 where exp / erfc
differ; negative values, ties across chunks, NaN and infinities at the ABI; batches and row ranges.  `pytest -m gpu`."""
import warnings

import numpy as np
import pytest

from tests import reduced_rank_restate as RD
from tests import test_gpu_reduced_ranks as GR
from tests import whole_index_restate as WI
from tests.test_gpu_reduced_ranks import short_lists  # noqa: F401  (the fixture: 300 x 1 000 x 8, float64 euclidean)

pytestmark = pytest.mark.gpu

CONVERSIONS = GR.CONVERSIONS
CONVERSION_IDS = [f"{m}{p if m == 'minkowski' else ''}_{np.dtype(t).name}" for m, p, t in CONVERSIONS]


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _states(rng, kind, n):
    """Arbitrary positive state vectors of one side: one, or (mean, deviation) for MP normal."""
    if kind == "mp_normal":
        return (rng.random(n) + 0.5, rng.random(n) + 0.1)
    return (rng.random(n) + 0.5,)


def _dev(ctx, state):
    return tuple(ctx.to_device(v) for v in state)


def _lists_of(hub):
    """(kind id, device q_state, device t_state, forward distances) of a fitted reduction: what kneighbors_whole_index passes."""
    nn = hub.nn_algo
    dist, _ = nn.kneighbors_device(query=None, k=nn.n_candidates)
    kind_id, q_state, t_state = hub._rank_state(dist)
    return kind_id, q_state, t_state, dist


@pytest.mark.parametrize("kind", RD.KINDS)
@pytest.mark.parametrize("metric,p,dtype", CONVERSIONS, ids=CONVERSION_IDS)
def test_position_is_rank(ctx, metric, p, dtype, kind):
    """The defining property: kz_gold_ranks_reduced of the row at column c, same inputs, is c."""
    from kiez_amd import _native as N
    from kiez_amd.neighbors import canonical_metric
    n_q, d = 96, 8
    for n_i in (65, 4096, 4097, 20_500):       # one chunk; a full one; a one-entry last chunk; six, the last of 20 entries (< k)
        rng = np.random.default_rng(n_i)
        q, y = rng.standard_normal((n_q, d)).astype(dtype), rng.standard_normal((n_i, d)).astype(dtype)
        qm, ym = N.DeviceMatrix(ctx, q, canonical_metric(metric, p)), N.DeviceMatrix(ctx, y, canonical_metric(metric, p))
        q_state, t_state = _dev(ctx, _states(rng, kind, n_q)), _dev(ctx, _states(rng, kind, n_i))
        for k in (1, 10, 64):
            w, ind = N.knn_reduced(ctx, qm, ym, k, RD.kind_id(kind), q_state, t_state)
            w, ind = w.numpy(), ind.numpy()
            where = f"{kind} {metric} {np.dtype(dtype).name} n_i={n_i} k={k}"
            assert w.shape == ind.shape == (n_q, k) and ind.dtype == np.int64 and w.dtype == np.float64
            assert ((ind >= 0) & (ind < n_i)).all(), where
            assert WI.non_decreasing(w), where
            for c in sorted({0, 1, k // 2, k - 1} & set(range(k))):
                rank = N.gold_ranks_reduced(ctx, qm, ym, ctx.to_device(np.ascontiguousarray(ind[:, c])), RD.kind_id(kind), q_state,
                                            t_state).numpy()
                np.testing.assert_array_equal(rank, np.full(n_q, c), err_msg=f"{where} column {c}")


@pytest.mark.parametrize("kind", RD.KINDS)
@pytest.mark.parametrize("metric,p,dtype", CONVERSIONS, ids=CONVERSION_IDS)
def test_whole_index_lists_bit_for_bit(ctx, metric, p, dtype, kind):
    """n_candidates = n_target: the forward list of a row holds every index row, so the whole-index list is the sort of the row
    `transform` writes for it by (value, index id) -- the same bits, ties (two identical target rows) included."""
    from kiez_amd import _native as N
    n_s = 300
    for d in (3, 64):
        for n_t in (63, 64, 65, 257):
            rng = np.random.default_rng(100 * n_t + d)
            source = rng.standard_normal((n_s, d)).astype(dtype)
            target = rng.standard_normal((n_t, d)).astype(dtype)
            target[n_t - 2] = target[1]                       # two identical index rows: equal distance, equal state, equal w
            source[1], source[3] = source[0], source[2]       # (and two pairs of identical queries)
            hub = GR._reduction(kind, n_t, metric, p)
            hub.fit(source, target)
            nn = hub.nn_algo
            dist, ind = nn.kneighbors_device(query=None, k=n_t)
            kind_id, q_state, t_state = hub._rank_state(dist)
            w, _ = hub.transform(dist, ind, source)
            w, ind = w.numpy(), ind.numpy()
            by_id = np.empty_like(w)
            np.put_along_axis(by_id, ind, w, axis=1)
            where = f"{kind} {metric} {np.dtype(dtype).name} d={d} n_target={n_t}"
            assert by_id[0, 1] == by_id[0, n_t - 2] or np.isnan(by_id[0, 1])      # (the tie is there)
            for k in (1, 10, n_t):
                got_w, got_i = N.knn_reduced(ctx, nn.source_index, nn.target_index, k, kind_id, q_state, t_state)
                want_w, want_i = WI.topk(by_id, k)
                np.testing.assert_array_equal(got_i.numpy(), want_i, err_msg=f"{where} k={k}")
                np.testing.assert_array_equal(got_w.numpy(), want_w, err_msg=f"{where} k={k}")
                real = ~np.isnan(want_w)
                np.testing.assert_array_equal(got_w.numpy().view(np.int64)[real], want_w.view(np.int64)[real], err_msg=f"{where} k={k} (bits)")


@pytest.mark.parametrize("kind", ["csls", "nicdm"])
def test_short_lists_equal_numpy_where_numpy_has_the_bits(ctx, short_lists, kind):  # noqa: F811
    """K = 10 of 1 000, k = 64: 2 d - a - b and d / sqrt(a b) are single correctly rounded operations in numpy as on the device."""
    from kiez_amd import _native as N
    source, target, _, dist, _ = short_lists
    hub = GR._reduction(kind, 10, "euclidean")
    hub.fit(source, target)
    kind_id, q_state, t_state, _ = _lists_of(hub)
    got_w, got_i = N.knn_reduced(ctx, hub.nn_algo.source_index, hub.nn_algo.target_index, 64, kind_id, q_state, t_state)
    as_np = lambda s: tuple(v.numpy() for v in ((s,) if not isinstance(s, tuple) else s))   # noqa: E731
    want_w, want_i = WI.knn_reduced(kind, dist, as_np(q_state), as_np(t_state), 64)
    np.testing.assert_array_equal(got_i.numpy(), want_i)
    np.testing.assert_array_equal(got_w.numpy().view(np.int64), want_w.view(np.int64))
    assert (want_w < 0).any() or kind != "csls"                # (CSLS: negative values are routine)


@pytest.mark.parametrize("kind,K", [("ls", 10), ("mp_normal", 50)])
@pytest.mark.parametrize("k", [10, 64])
def test_short_lists_inside_numpys_bracket(ctx, short_lists, kind, K, k):  # noqa: F811
    """exp / erfc of the device are not numpy's: |w - numpy's| <= 1e-12 everywhere, and the rows are numpy's wherever numpy's first
    k + 1 values stand more than 2e-12 apart (two values each off by less than 1e-12 cannot swap).  With numpy's own distances numpy
    leaves out 0 of 300 rows for LS at both k and for MP normal at k = 10, and 3 for MP normal at k = 64, where pairs saturated at
    exactly 1.0 begin; at most 6 may be left out here."""
    from kiez_amd import _native as N
    source, target, _, dist, _ = short_lists
    hub = GR._reduction(kind, K, "euclidean")
    hub.fit(source, target)
    kind_id, q_state, t_state, _ = _lists_of(hub)
    got_w, got_i = N.knn_reduced(ctx, hub.nn_algo.source_index, hub.nn_algo.target_index, k, kind_id, q_state, t_state)
    got_w, got_i = got_w.numpy(), got_i.numpy()
    as_np = lambda s: tuple(v.numpy() for v in ((s,) if not isinstance(s, tuple) else s))   # noqa: E731
    want_w, want_i = WI.knn_reduced(kind, dist, as_np(q_state), as_np(t_state), k + 1)
    clear = np.diff(want_w, axis=1).min(axis=1) > 2e-12
    err = np.abs(got_w - want_w[:, :k]).max()
    print(kind, "k", k, "rows left out:", int((~clear).sum()), "of", clear.size, "max |w - numpy|:", float(err), "rows that differ:",
          int((got_i != want_i[:, :k]).any(axis=1).sum()))
    assert WI.non_decreasing(got_w)
    assert err <= 1e-12
    np.testing.assert_array_equal(got_i[clear], want_i[clear, :k])
    assert (~clear).sum() <= 6


def test_signs_ties_nan_and_infinities_at_the_abi(ctx):
    """float64 euclidean, CSLS with q_a = 0: w = 2 d - 0 - t_a, whose bits numpy has."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(4)
    n_q, d = 8, 8

    def run(q, y, t_a, k):
        qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
        dist = np.sqrt(GR._all_pair_values(ctx, qm, ym))
        got_w, got_i = N.knn_reduced(ctx, qm, ym, k, N.RANK_CSLS, ctx.to_device(np.zeros(q.shape[0])), ctx.to_device(t_a))
        got_w, got_i = got_w.numpy(), got_i.numpy()
        want_w, want_i = WI.knn_reduced("csls", dist, (np.zeros(q.shape[0]),), (t_a,), k)
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_w, want_w)          # (NaN where numpy has NaN)
        np.testing.assert_array_equal(np.isnan(got_w), np.isnan(want_w))
        return got_w, got_i
    # (a) ten copies of one index row across both chunks, the query on top of them: equal w, by ascending id
    n_i = 5000
    q, y = rng.standard_normal((n_q, d)), rng.standard_normal((n_i, d))
    copies = np.array([3, 17, 1000, 2048, 4095, 4096, 4097, 4500, 4998, 4999])
    y[copies] = y[3]
    q[0] = y[3]
    w, ind = run(q, y, np.zeros(n_i), 64)
    np.testing.assert_array_equal(ind[0, :10], copies)
    assert (w[0, :10] == w[0, 0]).all() and w[0, 10] > w[0, 0]
    for r in range(1, n_q):                                   # (elsewhere the ten sit side by side, ascending)
        at = np.flatnonzero(np.isin(ind[r], copies))
        assert at.size in (0, 10) or at[-1] == 63
        np.testing.assert_array_equal(ind[r, at], copies[:at.size])
    # (b) every w negative
    w, ind = run(q, y, np.full(n_i, 1e3), 64)
    assert (w < 0).all()
    np.testing.assert_array_equal(ind[0, :10], copies)
    # (c) the sign changes inside the list
    t_a = rng.uniform(-5.0, 5.0, n_i)
    w, _ = run(q, y, t_a, 64)
    assert ((w[:, 0] < 0) & (w[:, -1] > 0)).all()
    # (d) 20 finite values, then NaN rows by id, returned as NaN
    n_i = 300
    y = rng.standard_normal((n_i, d))
    t_a = rng.random(n_i)
    finite = np.sort(rng.permutation(n_i)[:20])
    t_nan = np.where(np.isin(np.arange(n_i), finite), t_a, np.nan)
    w, ind = run(q, y, t_nan, 64)
    assert np.isfinite(w[:, :20]).all() and np.isnan(w[:, 20:]).all()
    np.testing.assert_array_equal(np.sort(ind[:, :20], axis=1), np.tile(finite, (n_q, 1)))
    np.testing.assert_array_equal(ind[:, 20:], np.tile(np.setdiff1d(np.arange(n_i), finite)[:44], (n_q, 1)))
    # (e) t_a = +inf: w = -inf, first, by id; t_a = -inf: w = +inf, tying with the NaN rows by id
    t_e = t_nan.copy()
    minus = np.array([5, 140, 299])
    t_e[minus] = np.inf
    plus = np.setdiff1d(np.arange(n_i), np.concatenate([finite, minus]))[[0, 3, 10]]
    t_e[plus] = -np.inf
    w, ind = run(q, y, t_e, 64)
    n_fin = 20 - int(np.isin(minus, finite).sum())
    np.testing.assert_array_equal(ind[:, :3], np.tile(minus, (n_q, 1)))
    assert (w[:, :3] == -np.inf).all() and np.isfinite(w[:, 3:3 + n_fin]).all()
    rest = np.setdiff1d(np.arange(n_i), np.concatenate([np.setdiff1d(finite, minus), minus]))[:64 - 3 - n_fin]
    np.testing.assert_array_equal(ind[:, 3 + n_fin:], np.tile(rest, (n_q, 1)))
    assert (w[:, 3 + n_fin:][:, np.isin(rest, plus)] == np.inf).all() and np.isnan(w[:, 3 + n_fin:][:, ~np.isin(rest, plus)]).all()
    assert np.isin(plus, rest).all()


def test_batches_row_ranges_and_refusals(ctx):
    """70 000 index rows: 479 rows of values per batch, 1 000 query rows; arbitrary positive states."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(70)
    n_q, n_i, d, k = 1000, 70_000, 8, 10
    q, y = rng.standard_normal((n_q, d)).astype(np.float32), rng.standard_normal((n_i, d)).astype(np.float32)
    q_a, t_a = rng.random(n_q) + 0.5, rng.random(n_i) + 0.5
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    t_dev = ctx.to_device(t_a)

    def lists(begin, count):
        w, ind = N.knn_reduced(ctx, qm, ym, k, N.RANK_CSLS, ctx.to_device(q_a[begin:begin + count]), t_dev, begin, count)
        return w.numpy(), ind.numpy()
    w, ind = lists(0, n_q)
    assert ((ind >= 0) & (ind < n_i)).all() and WI.non_decreasing(w)
    for part, whole in zip(zip(lists(0, 500), lists(500, 500)), (w, ind)):
        np.testing.assert_array_equal(np.concatenate(part), whole)
    for again, whole in zip(lists(0, n_q), (w, ind)):           # (and the same from call to call)
        np.testing.assert_array_equal(again, whole)
    rows = np.array([0, 1, 2, 300, 478, 479, 480, 600, 998, 999])      # both batches, and their edge
    vals = GR._all_pair_values(ctx, N.DeviceMatrix(ctx, q[rows], "euclidean"), ym)
    dist = np.sqrt(vals.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    want_w, want_i = WI.knn_reduced("csls", dist, (q_a[rows],), (t_a,), k)
    np.testing.assert_array_equal(ind[rows], want_i)
    np.testing.assert_array_equal(w[rows].view(np.int64), want_w.view(np.int64))
    # what the call refuses
    q_dev = ctx.to_device(q_a)
    with pytest.raises(ValueError, match="unknown kind"):
        N.knn_reduced(ctx, qm, ym, k, 5, q_dev, t_dev)
    with pytest.raises(ValueError, match="KZ_RANK_MP_NORMAL needs"):
        N.knn_reduced(ctx, qm, ym, k, N.RANK_MP_NORMAL, q_dev, t_dev)
    with pytest.raises(ValueError, match="must be NULL"):
        N.knn_reduced(ctx, qm, ym, k, N.RANK_NICDM, (q_dev, q_dev), (t_dev, t_dev))
    with pytest.raises(ValueError, match="different metrics"):
        N.knn_reduced(ctx, N.DeviceMatrix(ctx, q, "cosine"), ym, k, N.RANK_CSLS, q_dev, t_dev)
    with pytest.raises(ValueError, match="n_neighbors"):
        N.knn_reduced(ctx, qm, ym, 0, N.RANK_CSLS, q_dev, t_dev)
    with pytest.raises(ValueError, match="n_neighbors"):
        N.knn_reduced(ctx, qm, ym, n_i + 1, N.RANK_CSLS, q_dev, t_dev)
    with pytest.raises(NotImplementedError, match="512"):
        N.knn_reduced(ctx, qm, ym, 513, N.RANK_CSLS, q_dev, t_dev)


def test_api():
    from kiez_amd import Kiez, evaluate
    from kiez_amd.neighbors import NotFittedError
    rng = np.random.default_rng(21)
    source = rng.standard_normal((300, 16)).astype(np.float32)
    target = np.concatenate([source + 0.6 * rng.standard_normal((300, 16)).astype(np.float32),
                             rng.standard_normal((100, 16)).astype(np.float32)])
    gold = {i: i for i in range(0, 300, 2)}
    gold_arr = np.where(np.arange(300) % 2 == 0, np.arange(300), -1)
    has = gold_arr >= 0

    def kiez(hubness, **kw):
        return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hubness, hubness_kwargs=kw or None)
    for hubness, kw in (("CSLS", {}), ("LocalScaling", {"method": "standard"}), ("LocalScaling", {"method": "nicdm"}),
                        ("MutualProximity", {"method": "normal"})):
        kz = kiez(hubness, **kw).fit(source, target)
        ind = kz.kneighbors_whole_index(10, return_distance=False)
        r = kz.gold_ranks(gold, reduced=True)
        assert isinstance(ind, np.ndarray) and ind.shape == (300, 10) and ind.dtype == np.int64
        inside = has & (r < 10)
        assert (r[has] >= 0).all() and inside.any()
        np.testing.assert_array_equal(ind[inside, r[inside]], gold_arr[inside])          # position is rank ...
        assert not (ind[has & (r >= 10)] == gold_arr[has & (r >= 10), None]).any()       # ... and a rank beyond the list is absent
        assert evaluate.hits(ind, gold, k=[1, 10]) == evaluate.rank_metrics(r, gold, k=[1, 10])["hits"]
        with warnings.catch_warnings():
            warnings.simplefilter("error")                     # k > n_candidates: no clamp, no warning
            dist50, ind50 = kz.kneighbors_whole_index(50)
        assert dist50.shape == ind50.shape == (300, 50) and dist50.dtype == np.float64 and WI.non_decreasing(dist50)
        np.testing.assert_array_equal(ind50[:, :10], ind)
        dev_w, dev_i = kz.kneighbors_whole_index_device(10)
        np.testing.assert_array_equal(dev_i.numpy(), ind)
        np.testing.assert_array_equal(dev_w.numpy(), dist50[:, :10])
        dist5, ind5 = kz.kneighbors(5)                         # kneighbors afterwards is what it was
        fresh_dist, fresh_ind = kiez(hubness, **kw).fit(source, target).kneighbors(5)
        np.testing.assert_array_equal(ind5, fresh_ind)
        np.testing.assert_array_equal(dist5, fresh_dist)
        with pytest.raises(ValueError, match="n_neighbors"):
            kz.kneighbors_whole_index(401)
    # no reduction: the plain lists
    kz = kiez(None).fit(source, target)
    for got, want in zip(kz.kneighbors_whole_index(7), kz.kneighbors(7)):
        np.testing.assert_array_equal(got, want)
    # the reductions without a value outside the list, single-source fits, unfitted instances
    for hubness, kw in (("MutualProximity", {"method": "empiric"}), ("DisSimLocal", {})):
        kz = kiez(hubness, **kw).fit(source, target)
        with pytest.raises(NotImplementedError, match="outside the list"):
            kz.kneighbors_whole_index(5)
    with pytest.raises(NotImplementedError, match="two-sided"):
        kiez("CSLS").fit(source).kneighbors_whole_index(5)
    with pytest.raises(NotFittedError):
        kiez("CSLS").kneighbors_whole_index(5)
