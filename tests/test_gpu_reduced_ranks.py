"""Gold ranks under a hubness reduction on the device (kz_gold_ranks_reduced, HubnessReduction.gold_ranks,
Kiez.gold_ranks(reduced=True)): with lists over the whole index the rank is the count over `transform`'s output, bit for bit, for
every branch of the distance conversion; with short lists it is the numpy restatement over all pairs (tests/reduced_rank_restate.py)
-- exactly where numpy reproduces the bits (CSLS, NICDM), inside a 1e-12 bracket where exp / erfc differ (LS, MP normal) -- over
more than one chunk and more than one batch of values; and it is the position in the reference's own reduced lists
(tests/golden/reduced_ranks.npz).  `pytest -m gpu`."""
from pathlib import Path

import numpy as np
import pytest

from tests import rank_restate as RR
from tests import reduced_rank_restate as RD

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "reduced_ranks.npz"
NO_GOLD = RR.NO_GOLD


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _reduction(kind, n_candidates, metric, p=2):
    from kiez_amd.hubness_reduction import CSLS, LocalScaling, MutualProximity
    from kiez_amd.neighbors import SklearnNN
    nn = SklearnNN(n_candidates=n_candidates, metric=metric, p=p)
    if kind == "csls":
        return CSLS(nn_algo=nn)
    if kind in ("ls", "nicdm"):
        return LocalScaling(method="standard" if kind == "ls" else "nicdm", nn_algo=nn)
    return MutualProximity(method="normal", nn_algo=nn)


def _all_pair_values(ctx, qm, ym):
    """[n_q, n_i] float64: kz_pair_values of every pair -- the values the search ranks by."""
    from kiez_amd import _native as N
    n_q, n_i = qm.shape[0], ym.shape[0]
    ind = ctx.to_device(np.tile(np.arange(n_i, dtype=np.int64), (n_q, 1)))
    val = ctx.empty((n_q, n_i), np.float64)
    N._check(ctx.lib.kz_pair_values(ctx.handle, qm.handle, 0, n_q, ym.handle, ind.ptr, n_i, val.ptr), "kz_pair_values")
    return val.numpy()


def _device_states(hub, kind):
    """(q_state, t_state) as numpy vectors, read back from the device: the fit state, and the statistics of the forward lists."""
    nn = hub.nn_algo
    dist, _ = nn.kneighbors_device(query=None, k=nn.n_candidates)
    _, q_state, t_state = hub._rank_state(dist)
    as_np = lambda s: tuple(v.numpy() for v in ((s,) if not isinstance(s, tuple) else s))   # noqa: E731
    return as_np(q_state), as_np(t_state)


# one (metric, dtype) per branch of kz_output_distance
CONVERSIONS = [("euclidean", 2, np.float32), ("euclidean", 2, np.float64), ("cosine", 2, np.float32), ("minkowski", 3, np.float32)]


@pytest.mark.parametrize("kind", RD.KINDS)
@pytest.mark.parametrize("metric,p,dtype", CONVERSIONS, ids=[f"{m}{p if m == 'minkowski' else ''}_{np.dtype(t).name}" for m, p, t in CONVERSIONS])
def test_whole_index_lists_give_the_count_over_transforms_output(metric, p, dtype, kind):
    """n_candidates = n_target: the forward list of a row holds every index row, so the rank is the (value, index id) count over
    the row `transform` writes for it -- the same bits, ties (two identical target rows) included."""
    n_s = 300
    for d in (3, 64):
        for n_t in (63, 64, 65, 257):
            rng = np.random.default_rng(100 * n_t + d)
            source = rng.standard_normal((n_s, d)).astype(dtype)
            target = rng.standard_normal((n_t, d)).astype(dtype)
            target[n_t - 2] = target[1]                       # two identical index rows: equal distance, equal state, equal w
            source[1], source[3] = source[0], source[2]       # (and two pairs of identical queries, one gold on each copy)
            gold = rng.integers(0, n_t, n_s).astype(np.int64)
            gold[0:4] = [1, n_t - 2, n_t - 2, 1]
            gold[10:300:9] = -1
            hub = _reduction(kind, n_t, metric, p)
            hub.fit(source, target)
            got = hub.gold_ranks(gold)
            nn = hub.nn_algo
            dist, ind = nn.kneighbors_device(query=None, k=n_t)
            w, _ = hub.transform(dist, ind, source)
            w, ind = w.numpy(), ind.numpy()
            assert all(sorted(r) == list(range(n_t)) for r in ind[:5].tolist())
            by_id = np.empty_like(w)
            np.put_along_axis(by_id, ind, w, axis=1)
            where = f"{kind} {metric} {np.dtype(dtype).name} d={d} n_target={n_t}"
            np.testing.assert_array_equal(got, RR.gold_ranks(by_id, gold), err_msg=where)
            assert got.dtype == np.int64 and (got[gold < 0] == -1).all() and (got[gold >= 0] >= 0).all()
            assert by_id[0, 1] == by_id[0, n_t - 2] or np.isnan(by_id[0, 1])      # (the tie is there)
            assert got[1] > got[0] and got[2] > got[3]                            # the later copy behind the earlier one


def test_a_nan_in_every_list_ranks_by_row():
    """correlation against a constant index row is NaN: every full-length list ends in it, the mean of every list is NaN, every CSLS
    value is NaN, all of them rank as +inf by row -- the rank is the gold id."""
    rng = np.random.default_rng(65)
    source, target = rng.standard_normal((300, 8)), rng.standard_normal((65, 8))
    target[32] = 1.5
    gold = rng.integers(0, 65, 300).astype(np.int64)
    gold[:3] = [32, 0, 64]
    hub = _reduction("csls", 65, "correlation")
    hub.fit(source, target)
    dist, _ = hub.nn_algo.kneighbors_device(query=None, k=65)
    assert np.isnan(dist.numpy()[:, -1]).all()
    np.testing.assert_array_equal(hub.gold_ranks(gold), gold)


@pytest.fixture(scope="module")
def short_lists():
    """300 noisy copies among 1 000 index rows, float64 euclidean: the distances of all pairs from kz_pair_values, once."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(20240)
    n_s, n_t, d = 300, 1000, 8
    target = rng.standard_normal((n_t, d))
    perm = rng.permutation(n_t)
    source = target[perm[:n_s]] + 1.2 * rng.standard_normal((n_s, d))
    gold = perm[:n_s].astype(np.int64)
    ctx = N.Context.get()
    dist = np.sqrt(_all_pair_values(ctx, N.DeviceMatrix(ctx, source, "euclidean"), N.DeviceMatrix(ctx, target, "euclidean")))
    dist.setflags(write=False)
    return source, target, gold, dist, rng.integers(0, n_t, 40)


@pytest.mark.parametrize("kind", ["csls", "nicdm"])
def test_short_lists_equal_numpy_where_numpy_has_the_bits(short_lists, kind):
    """K = 10 of 1 000: 2 d - a - b and d / sqrt(a b) are single correctly rounded operations in numpy as on the device."""
    source, target, gold, dist, random_rows = short_lists
    gold = gold.copy()
    gold[:40] = random_rows                                    # golds far from the query too
    hub = _reduction(kind, 10, "euclidean")
    hub.fit(source, target)
    got = hub.gold_ranks(gold)
    q_state, t_state = _device_states(hub, kind)
    want = RD.ranks(kind, dist, q_state, t_state, gold)
    print(kind, "rank quartiles", np.percentile(want, [25, 50, 75]), "max", want.max())
    np.testing.assert_array_equal(got, want)
    assert want.max() > 100 and (want == 0).any()


@pytest.mark.parametrize("kind,K,cap", [("ls", 10, 0.05), ("mp_normal", 50, 0.10)])
def test_short_lists_inside_numpys_bracket(short_lists, kind, K, cap):
    """exp / erfc of the device are not numpy's: every rank lies in #{w < w_g - 1e-12} <= rank <= #{w <= w_g + 1e-12} - 1 of numpy's
    w, and the bracket is a single value on all but a few rows (MP normal: far pairs saturate at exactly 1.0 and tie by row, which
    the bracket's <= counts the same way; numpy alone leaves out 0 of 300 rows for LS and 9 for MP normal)."""
    source, target, gold, dist, _ = short_lists
    hub = _reduction(kind, K, "euclidean")
    hub.fit(source, target)
    got = hub.gold_ranks(gold)
    q_state, t_state = _device_states(hub, kind)
    w = RD.reduce(kind, dist, q_state, t_state)
    lo, hi = RD.bracket(w, gold, 1e-12)
    wide = hi > lo
    print(kind, "rows with a bracket wider than one value:", int(wide.sum()), "of", gold.size, "saturated pairs:",
          float((w == 1.0).mean()), "outside:", int(((got < lo) | (got > hi)).sum()))
    assert ((lo <= got) & (got <= hi)).all()
    np.testing.assert_array_equal(got[~wide], lo[~wide])
    assert wide.sum() <= cap * gold.size


@pytest.mark.parametrize("n_t", [8191, 8192, 8193, 9000])
def test_csls_beyond_one_chunk_and_beyond_any_list(ctx, n_t):
    """Index rows around the 8 192 values of a count chunk and two chunks of values per row (an odd count: value rows start at both
    parities), ranks past the 4 096 neighbours a list can hold."""
    rng = np.random.default_rng(n_t)
    n_s, d = 64, 8
    source, target = rng.standard_normal((n_s, d)), rng.standard_normal((n_t, d))
    gold = rng.integers(0, n_t, n_s).astype(np.int64)
    gold[0], gold[1] = 0, n_t - 1
    gold[4], gold[5] = min(8191, n_t - 1), min(8192, n_t - 1)   # the two sides of the count chunk's edge
    hub = _reduction("csls", 10, "euclidean")
    hub.fit(source, target)
    got = hub.gold_ranks(gold)
    dist = np.sqrt(_all_pair_values(ctx, hub.nn_algo.source_index, hub.nn_algo.target_index))
    q_state, t_state = _device_states(hub, "csls")
    np.testing.assert_array_equal(got, RD.ranks("csls", dist, q_state, t_state, gold))
    assert got.max() >= 4096                                   # some gold row lies beyond any list


def test_batches_and_row_ranges_of_the_native_call(ctx):
    """70 000 index rows: 479 rows of values per batch, 1 000 query rows, a third of them without gold; arbitrary positive states."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(70)
    n_q, n_i, d = 1000, 70_000, 8
    q, y = rng.standard_normal((n_q, d)).astype(np.float32), rng.standard_normal((n_i, d)).astype(np.float32)
    gold = rng.integers(0, n_i, n_q).astype(np.int64)
    gold[::3] = NO_GOLD
    gold[1], gold[4], gold[998] = n_i, -7, n_i + 12345          # out of range
    missing = (gold < 0) | (gold >= n_i)
    assert (~missing).sum() > 479
    q_a, t_a = rng.random(n_q) + 0.5, rng.random(n_i) + 0.5
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    t_dev = ctx.to_device(t_a)

    def ranks(begin, count):
        return N.gold_ranks_reduced(ctx, qm, ym, ctx.to_device(gold[begin:begin + count]), N.RANK_CSLS,
                                    ctx.to_device(q_a[begin:begin + count]), t_dev, begin, count).numpy()
    rank = ranks(0, n_q)
    np.testing.assert_array_equal(rank == -1, missing)
    assert (rank[~missing] >= 0).all() and (rank < n_i).all()
    np.testing.assert_array_equal(np.concatenate([ranks(0, 500), ranks(500, 500)]), rank)
    np.testing.assert_array_equal(ranks(0, n_q), rank)          # (and the same from call to call)
    rows = np.flatnonzero(~missing)[[0, 1, 2, 300, 478, 479, 480, 600, -2, -1]]      # both batches, and their edge
    vals = _all_pair_values(ctx, N.DeviceMatrix(ctx, q[rows], "euclidean"), ym)
    dist = np.sqrt(vals.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(rank[rows], RD.ranks("csls", dist, (q_a[rows],), (t_a,), gold[rows]))
    # what the call refuses
    g_dev, q_dev = ctx.to_device(gold), ctx.to_device(q_a)
    with pytest.raises(ValueError, match="unknown kind"):
        N.gold_ranks_reduced(ctx, qm, ym, g_dev, 5, q_dev, t_dev)
    with pytest.raises(ValueError, match="KZ_RANK_MP_NORMAL needs"):
        N.gold_ranks_reduced(ctx, qm, ym, g_dev, N.RANK_MP_NORMAL, q_dev, t_dev)
    with pytest.raises(ValueError, match="must be NULL"):
        N.gold_ranks_reduced(ctx, qm, ym, g_dev, N.RANK_NICDM, (q_dev, q_dev), (t_dev, t_dev))
    with pytest.raises(ValueError, match="different metrics"):
        N.gold_ranks_reduced(ctx, N.DeviceMatrix(ctx, q, "cosine"), ym, g_dev, N.RANK_CSLS, q_dev, t_dev)


def test_api():
    from kiez_amd import Kiez, evaluate
    from kiez_amd.neighbors import NotFittedError
    rng = np.random.default_rng(21)
    source = rng.standard_normal((300, 16)).astype(np.float32)
    target = np.concatenate([source + 0.6 * rng.standard_normal((300, 16)).astype(np.float32),
                             rng.standard_normal((100, 16)).astype(np.float32)])
    gold = {i: i for i in range(0, 300, 2)}
    gold_arr = np.where(np.arange(300) % 2 == 0, np.arange(300), -1)

    def kiez(hubness, **kw):
        return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hubness, hubness_kwargs=kw or None)
    # no reduction: the plain ranks
    kz = kiez(None).fit(source, target)
    plain = kz.algorithm.gold_ranks(gold)
    np.testing.assert_array_equal(kz.gold_ranks(gold, reduced=True), plain)
    # CSLS: reduced=False is the plain call; reduced=True takes the dict and the array alike, and leaves kneighbors as it was
    kz = kiez("CSLS").fit(source, target)
    np.testing.assert_array_equal(kz.gold_ranks(gold, reduced=False), kz.algorithm.gold_ranks(gold))
    np.testing.assert_array_equal(kz.gold_ranks(gold), plain)
    reduced = kz.gold_ranks(gold, reduced=True)
    assert isinstance(reduced, np.ndarray) and reduced.dtype == np.int64 and reduced.shape == (300,)
    np.testing.assert_array_equal(reduced, kz.gold_ranks(gold_arr, reduced=True))
    np.testing.assert_array_equal(reduced == -1, gold_arr < 0)
    assert (reduced != plain).any()                             # (the reduction decides something)
    dist, ind = kz.kneighbors(5)
    fresh_dist, fresh_ind = kiez("CSLS").fit(source, target).kneighbors(5)
    np.testing.assert_array_equal(ind, fresh_ind)
    np.testing.assert_array_equal(dist, fresh_dist)
    with pytest.raises(ValueError, match="s_to_t"):
        kz.gold_ranks(gold, s_to_t=False, reduced=True)
    # rank_metrics takes the host vector and the device vector
    from kiez_amd import _native as N
    dev = kz.hubness.gold_ranks_device(gold)
    assert isinstance(dev, N.DeviceArray)
    m = evaluate.rank_metrics(reduced, gold, k=[1, 10, 400])
    assert m == evaluate.rank_metrics(dev, gold, k=[1, 10, 400])
    assert m["n_ranked"] == 150 and m["hits"][400] == 1.0 and 0.0 < m["hits"][1] <= m["hits"][10] and 0.0 < m["mrr"] <= 1.0
    # the reductions without a value outside the list, single-source fits, unfitted instances
    for hubness, kw in (("MutualProximity", {"method": "empiric"}), ("DisSimLocal", {})):
        kz = kiez(hubness, **kw).fit(source, target)
        with pytest.raises(NotImplementedError, match="outside the list"):
            kz.gold_ranks(gold, reduced=True)
        np.testing.assert_array_equal(kz.gold_ranks(gold), plain)
    with pytest.raises(NotImplementedError, match="two-sided"):
        kiez("CSLS").fit(source).gold_ranks(gold, reduced=True)
    with pytest.raises(NotFittedError):
        kiez("CSLS").gold_ranks(gold, reduced=True)
    for hubness, kw in (("LocalScaling", {"method": "standard"}), ("LocalScaling", {"method": "nicdm"}), ("MutualProximity", {"method": "normal"})):
        r = kiez(hubness, **kw).fit(source, target).gold_ranks(gold, reduced=True)
        assert ((r >= 0) == (gold_arr >= 0)).all() and (r < 400).all()


def test_golden_from_the_reference():
    """On the rows whose gold stands clear of its neighbours in the reference's reduced list, the device rank is the position there."""
    from kiez_amd import Kiez
    g = np.load(GOLDEN)
    source, target, gold = g["source"], g["target"], g["gold"]
    names = {"csls": ("CSLS", {}), "ls": ("LocalScaling", {"method": "standard"}), "nicdm": ("LocalScaling", {"method": "nicdm"}),
             "mp_normal": ("MutualProximity", {"method": "normal"})}
    for metric in g["metrics"]:
        for kind in g["kinds"]:
            hubness, kw = names[str(kind)]
            kz = Kiez(n_candidates=target.shape[0], algorithm="SklearnNN", algorithm_kwargs={"metric": str(metric)}, hubness=hubness,
                      hubness_kwargs=dict(kw))
            rank = kz.fit(source, target).gold_ranks(gold, reduced=True)
            clear = g[f"{metric}__{kind}__clear"]
            pos = RR.positions(g[f"{metric}__{kind}__ind"].astype(np.int64), gold)
            assert clear.sum() >= 0.9 * (gold >= 0).sum()
            np.testing.assert_array_equal(rank[clear], pos[clear], err_msg=f"{metric} {kind}")
            np.testing.assert_array_equal(rank == -1, gold < 0)
