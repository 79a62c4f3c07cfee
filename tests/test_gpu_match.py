"""One-to-one matching on the device (kz_match_lists, matching.one_to_one, Kiez.match): every result is compared for exact equality
of `match` and `col` with the sequential Gale-Shapley of tests/match_restate.py, and with the greedy assignment where the rows
ascend -- over one row, complete lists, more sources than targets and the reverse, lists that force displacements, identical lists
(the skip-ahead), more rows than one grid covers; float64 and float32 values, sorted rows and shuffled columns; ties, NaN,
infinities, signed zeros, negative values, repeated targets, padding; the facade under every device-native reduction.
`pytest -m gpu`."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import match_restate as MR
from tests.test_match import CHAIN_COL, CHAIN_DIST, CHAIN_IND, CHAIN_MATCH, assert_same, random_lists

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def run(ctx, dist, ind, n_index):
    """kz_match_lists on host lists -> ((match, col), rounds)."""
    from kiez_amd import _native as N
    match, col, rounds = N.match_lists(ctx, ctx.to_device(dist), ctx.to_device(ind), n_index)
    return (match.numpy(), col.numpy()), rounds


def shuffled(rng, dist, ind):
    """The same pairs with the columns of every row in random order: the source's ranking is the column, not the value."""
    perm = np.argsort(rng.random(ind.shape), axis=1)
    return np.take_along_axis(dist, perm, axis=1), np.take_along_axis(ind, perm, axis=1)


def check(ctx, dist, ind, n_index, ascending, what=""):
    """Device == Gale-Shapley (and == greedy on ascending rows), a valid matching, -> ((match, col), rounds)."""
    got, rounds = run(ctx, dist, ind, n_index)
    assert got[0].dtype == got[1].dtype == np.int64
    assert_same(got, MR.gale_shapley(dist, ind, n_index), f"against Gale-Shapley {what}")
    if ascending:
        assert_same(got, MR.greedy(dist, ind, n_index), f"against greedy {what}")
    assert 0 <= rounds <= ind.size + n_index
    return got, rounds


def complete_lists(rng, n_q, n_index, dtype):
    """Every row lists every target, values ascending."""
    ind = np.argsort(rng.random((n_q, n_index)), axis=1).astype(np.int64)
    return np.sort(rng.standard_normal((n_q, n_index)), axis=1).astype(dtype), ind


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_shapes(ctx, dtype, shuffle):
    rng = np.random.default_rng(7)
    prep = (lambda d, i: shuffled(rng, d, i)) if shuffle else (lambda d, i: (d, i))

    dist, ind = prep(np.array([[0.25]], dtype=dtype), np.zeros((1, 1), dtype=np.int64))
    got, rounds = check(ctx, dist, ind, 1, not shuffle, "1 x 1 x 1")
    assert got[0].tolist() == [0] and got[1].tolist() == [0] and rounds == 1

    dist, ind = prep(*complete_lists(rng, 64, 64, dtype))
    got, _ = check(ctx, dist, ind, 64, not shuffle, "64 x 64 x 64")
    assert sorted(got[0].tolist()) == list(range(64))            # every row matched: a permutation

    dist, ind = prep(*complete_lists(rng, 257, 65, dtype))
    got, _ = check(ctx, dist, ind, 65, not shuffle, "257 x 65 x 65")
    assert sorted(got[0][got[0] >= 0].tolist()) == list(range(65))   # exactly the 65 targets are taken

    dist, ind = prep(*random_lists(rng, 65, 257, 10, dtype=dtype))
    check(ctx, dist, ind, 257, not shuffle, "65 x 257 x 10")

    dist, ind = prep(*random_lists(rng, 1000, 1000, 10, dtype=dtype))
    got, rounds = check(ctx, dist, ind, 1000, not shuffle, "1000 x 1000 x 10")
    assert rounds > 1                                              # displacements and retries occur
    assert MR.blocking_pairs(dist, ind, 1000, got) == []
    m = got[0][got[0] >= 0]
    assert len(np.unique(m)) == len(m)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_displacement_chain(ctx, dtype):
    got, rounds = check(ctx, CHAIN_DIST.astype(dtype), CHAIN_IND, 2, False, "chain")
    np.testing.assert_array_equal(got[0], CHAIN_MATCH)
    np.testing.assert_array_equal(got[1], CHAIN_COL)
    assert rounds == 3      # all three propose; C takes X; A takes Y (B then steps over X, which holds a better pair)


@pytest.mark.parametrize("direction", [1, -1], ids=["increasing", "decreasing"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_identical_lists_take_one_round_per_target(ctx, dtype, direction):
    """Every row holds the same list; the values grow (shrink) with the source row.  Without the skip-ahead every loser would retry
    column by column: with it, the rows left over step to the first target not yet held, and each round assigns one target."""
    n = 300
    rng = np.random.default_rng(3)
    ind = np.tile(rng.permutation(n).astype(np.int64), (n, 1))
    rows = np.arange(n, dtype=np.float64)[:, None]
    dist = (np.arange(n, dtype=np.float64)[None, :] + direction * rows / 1024.0).astype(dtype)   # (exact in float32)
    got, rounds = check(ctx, dist, ind, n, True, "identical lists")
    assert rounds <= n + 1
    order = np.arange(n) if direction > 0 else np.arange(n)[::-1]
    np.testing.assert_array_equal(got[0][order], ind[0])          # the best row takes the first target, the next the second, ...
    dist_s, ind_s = shuffled(rng, dist, np.ascontiguousarray(ind))
    check(ctx, dist_s, ind_s, n, False, "identical pairs, shuffled columns")


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values(ctx, dtype, shuffle):
    rng = np.random.default_rng(11)
    prep = (lambda d, i: shuffled(rng, d, i)) if shuffle else (lambda d, i: (d, i))
    n_q, n_index, k = 70, 24, 8
    inf, nan = np.inf, np.nan

    # all values equal (the MP-normal 1.0 plateau): by source row
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype)
    check(ctx, *prep(np.ones_like(dist), ind), n_index, not shuffle, "all equal")

    # rows holding NaN, +-inf and +-0.0 (sorted rows: in key order, NaN with +inf at the end)
    special = np.array([-inf, -1.0, -0.0, 0.0, 0.0, 1.0, inf, nan], dtype=dtype)
    dist = np.tile(special, (n_q, 1))
    dist[1::3] = np.array([-inf, -inf, -0.0, -0.0, 0.0, inf, nan, inf], dtype=dtype)
    dist[2::3] = np.array([0.0, -0.0, 0.0, nan, nan, inf, inf, nan], dtype=dtype)
    check(ctx, *prep(dist, ind), n_index, not shuffle, "special values")

    # all-negative values (CSLS)
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype)
    dist = np.sort(-np.abs(dist) - 0.5, axis=1)
    check(ctx, *prep(dist, ind), n_index, not shuffle, "negative")

    # few distinct values: ties across rows
    check(ctx, *prep(*random_lists(rng, n_q, n_index, k, dtype=dtype, ties=True)), n_index, not shuffle, "ties")

    # a target listed twice in one row (k > n_index repeats ids; and one repeated on purpose in every row)
    dist, ind = random_lists(rng, n_q, 5, k, dtype=dtype)
    ind[:, 5] = ind[:, 1]
    check(ctx, *prep(dist, ind), 5, not shuffle, "repeated targets")

    # padding (-1, INT_MAX, n_index) at the row ends, in the middle, and rows of padding only
    dist, ind = random_lists(rng, n_q, n_index, k, dtype=dtype, pad=0.25)
    ind[:, -1] = 0x7fffffff
    ind[::2, -2] = -1
    ind[5] = -1
    ind[6] = n_index
    ind[7] = 0x7fffffff
    ind[8] = [n_index, -1, 0x7fffffff, -5, n_index + 1, 1 << 40, -(1 << 40), np.iinfo(np.int64).min]
    got, _ = check(ctx, *prep(dist, ind), n_index, not shuffle, "padding")
    assert (got[0][5:9] == -1).all() and (got[1][5:9] == -1).all()


def test_two_runs_agree(ctx):
    rng = np.random.default_rng(5)
    dist, ind = shuffled(rng, *random_lists(rng, 3000, 800, 12, ties=True))
    (a, rounds_a), (b, rounds_b) = run(ctx, dist, ind, 800), run(ctx, dist, ind, 800)
    assert_same(a, b, "second run")
    assert rounds_a == rounds_b


def test_more_rows_than_one_grid(ctx):
    """70 000 rows: the grid-stride loop of every kernel.  Compared with the greedy assignment (a sort of 700 000 triples)."""
    rng = np.random.default_rng(70_000)
    n = 70_000
    ind = rng.integers(0, n, (n, 10), dtype=np.int64)
    dist = np.sort(rng.standard_normal((n, 10)), axis=1)
    got, rounds = run(ctx, dist, ind, n)
    assert_same(got, MR.greedy(dist, ind, n), "70 000 x 70 000 x 10")
    assert rounds > 1


def test_limits_and_null_rounds(ctx):
    from kiez_amd import _native as N
    from kiez_amd import matching
    dist, ind = np.zeros((3, 4097)), np.zeros((3, 4097), dtype=np.int64)
    with pytest.raises(ValueError, match="4096"):
        run(ctx, dist, ind, 5)
    with pytest.raises(ValueError, match="4096"):
        matching.one_to_one(dist, ind, 5)
    with pytest.raises(ValueError, match="n_index"):
        run(ctx, dist[:, :4], ind[:, :4], 0)
    with pytest.raises(ValueError, match="n_index"):
        run(ctx, dist[:, :4], ind[:, :4], 1 << 31)
    # n_q == 0 returns at once
    got, rounds = run(ctx, np.zeros((0, 4)), np.zeros((0, 4), dtype=np.int64), 5)
    assert got[0].shape == (0,) and rounds == 0
    # h_rounds may be null
    rng = np.random.default_rng(9)
    dist, ind = random_lists(rng, 200, 50, 6)
    d_dev, i_dev = ctx.to_device(dist), ctx.to_device(ind)
    match, col = ctx.empty((200,), np.int64), ctx.empty((200,), np.int64)
    N._check(ctx.lib.kz_match_lists(ctx.handle, d_dev.ptr, N.KZ_F64, i_dev.ptr, 200, 6, 50, match.ptr, col.ptr,
                                    ctypes.POINTER(ctypes.c_int64)()), "kz_match_lists")
    assert_same((match.numpy(), col.numpy()), MR.greedy(dist, ind, 50), "null h_rounds")
    with pytest.raises(ValueError, match="dist_dtype"):
        N._check(ctx.lib.kz_match_lists(ctx.handle, d_dev.ptr, 7, i_dev.ptr, 200, 6, 50, match.ptr, col.ptr, None), "kz_match_lists")


def test_one_to_one(ctx):
    from kiez_amd import _native as N
    from kiez_amd import matching
    rng = np.random.default_rng(13)
    for dtype in DTYPES:
        dist, ind = random_lists(rng, 300, 120, 9, dtype=dtype, pad=0.1)
        dist[4, 2] = np.nan
        want_match, want_col = MR.gale_shapley(dist, ind, 120)
        want_dist = np.where(want_col >= 0, dist[np.arange(300), np.maximum(want_col, 0)], np.nan).astype(dtype)
        md, mi = matching.one_to_one(dist, ind, 120)
        assert md.dtype == dtype and mi.dtype == np.int64
        np.testing.assert_array_equal(mi, want_match)
        np.testing.assert_array_equal(md.view(np.uint8), want_dist.view(np.uint8))     # bit for bit, NaN where unmatched
        assert (want_match < 0).any() and np.isnan(md[want_match < 0]).all()
        np.testing.assert_array_equal(matching.one_to_one(dist, ind.astype(np.int32), 120, return_distance=False), want_match)
        md_dev, mi_dev = matching.one_to_one(ctx.to_device(dist), ctx.to_device(ind), 120)
        assert isinstance(md_dev, N.DeviceArray) and isinstance(mi_dev, N.DeviceArray)
        np.testing.assert_array_equal(mi_dev.numpy(), want_match)
        np.testing.assert_array_equal(md_dev.numpy().view(np.uint8), want_dist.view(np.uint8))


def _kiez(hubness, metric):
    from kiez_amd import Kiez
    name, kwargs = {"none": (None, None), "csls": ("CSLS", None), "nicdm": ("LocalScaling", {"method": "nicdm"}),
                    "mp_normal": ("MutualProximity", {"method": "normal"}), "mp_empiric": ("MutualProximity", {"method": "empiric"})}[hubness]
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=name, hubness_kwargs=kwargs)


@pytest.fixture(scope="module")
def embeddings():
    rng = np.random.default_rng(500)
    target = rng.standard_normal((400, 16))
    source = target[rng.integers(0, 400, 500)] + 0.4 * rng.standard_normal((500, 16))    # several sources near one target
    return source, target


@pytest.mark.parametrize("metric,dtype", [("euclidean", np.float64), ("cosine", np.float32)], ids=["euclidean_f64", "cosine_f32"])
@pytest.mark.parametrize("hubness", ["none", "csls", "nicdm", "mp_normal"])
def test_facade(embeddings, hubness, metric, dtype):
    from kiez_amd import _native as N
    from kiez_amd import evaluate
    source, target = (x.astype(dtype) for x in embeddings)
    k_inst = _kiez(hubness, metric).fit(source, target)
    before = k_inst.kneighbors(5)
    for whole in (False, True):
        dist, ind = k_inst.kneighbors_whole_index(10) if whole else k_inst.kneighbors(10)
        want_match, want_col = MR.greedy(dist, ind, 400)
        md, mi = k_inst.match(10, whole_index=whole)
        where = f"{hubness} {metric} whole_index={whole}"
        np.testing.assert_array_equal(mi, want_match, err_msg=where)
        assert md.dtype == dist.dtype and mi.dtype == np.int64
        want_dist = np.where(want_col >= 0, dist[np.arange(500), np.maximum(want_col, 0)], np.nan).astype(dist.dtype)
        np.testing.assert_array_equal(md.view(np.uint8), want_dist.view(np.uint8), err_msg=where)   # dist[i, col] bit for bit, else NaN
        assert (mi < 0).any() and np.isnan(md[mi < 0]).all()        # 500 sources, 400 targets
        taken = mi[mi >= 0]
        assert len(np.unique(taken)) == len(taken)                   # no target twice
        np.testing.assert_array_equal(k_inst.match(10, whole_index=whole, return_distance=False), mi)
        md_dev, mi_dev = k_inst.match_device(10, whole_index=whole)
        assert isinstance(md_dev, N.DeviceArray) and isinstance(mi_dev, N.DeviceArray)
        np.testing.assert_array_equal(mi_dev.numpy(), mi)
        np.testing.assert_array_equal(md_dev.numpy().view(np.uint8), md.view(np.uint8))
        gold = {i: int(t) for i, t in enumerate(np.random.default_rng(1).integers(0, 400, 450))}
        gold_arr = np.array([gold[i] for i in range(450)])
        assert evaluate.hits(mi[:, None], gold, k=[1])[1] == np.count_nonzero(mi[:450] == gold_arr) / 450
    after = k_inst.kneighbors(5)
    np.testing.assert_array_equal(after[1], before[1])
    np.testing.assert_array_equal(after[0], before[0])


def test_facade_passes_the_list_calls_rules_through(embeddings):
    source, target = embeddings
    k_inst = _kiez("mp_empiric", "euclidean").fit(source, target)
    with pytest.raises(NotImplementedError):
        k_inst.match(10, whole_index=True)
    dist, ind = k_inst.kneighbors(10)
    np.testing.assert_array_equal(k_inst.match(10)[1], MR.greedy(dist, ind, 400)[0])
    k_inst = _kiez("csls", "euclidean").fit(source, target)
    with pytest.warns(UserWarning, match="No k supplied"):
        mi = k_inst.match(return_distance=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dist, ind = k_inst.kneighbors()
    np.testing.assert_array_equal(mi, MR.greedy(dist, ind, 400)[0])
    with pytest.raises(ValueError, match="n_samples_fit = 400"):
        k_inst.match(401, whole_index=True)
    single = _kiez("csls", "euclidean").fit(source)
    with pytest.raises(NotImplementedError, match="two-sided"):
        single.match(10, whole_index=True)
