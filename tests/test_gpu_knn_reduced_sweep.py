"""knn_reduced_sweep -- kz_knn_reduced_sweep: the rank-one emit sweep of the fp16 images plus the exact w of its candidates --
against two references per case: (a) knn_reduced (the exact route) on the same handles, byte for byte (the project's anchor), and (b) a plain numpy
float64 w of all pairs from the same state vectors, top k by (w, row), compared as indices.

numpy is a reference only where the data lets it be one: on every row the relative gap between the k-th and the (k+1)-th numpy w is at
least 1e-9.  That is a condition on the data, asserted on the CPU for every case; the seeds are fixed so that it holds.  The state
vectors are passed at the ABI with t_a spread over 0.5 .. 2 x the mean distance, so that the rank-one term and the tile reject matter and
whole-index lists leave the seed lists on a share of the rows (asserted > 0 on the CPU).  The main cases use data of low intrinsic
dimension (`latent_case`): its distances vary by an order of magnitude, so a row's seeds say something about its neighbours; on
Gaussian data of high dimension every distance is the same within a few percent and a state spread that wide decides the lists alone."""
import numpy as np
import pytest

from tests.test_gpu_radius_sweep import make_case

pytestmark = pytest.mark.gpu
KINDS = {"csls": 1, "ls": 2, "nicdm": 3, "mp_normal": 4, "dual": 8}


def latent_case(n_q, n_i, d, seed):
    """Rows on a 4-dimensional subspace of R^d plus 5 % noise."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((4, d))
    rows = lambda n: (rng.standard_normal((n, 4)) @ basis + 0.05 * rng.standard_normal((n, d))).astype(np.float32)   # noqa: E731
    return rows(n_q), rows(n_i)


def numpy_distances(q, y, metric):
    """float64 distances as the search returns them: euclidean float32 rows come back rounded to float32 (the scikit-learn convention)."""
    q, y = q.astype(np.float64), y.astype(np.float64)
    if metric == "cosine":
        q, y = q / np.linalg.norm(q, axis=1, keepdims=True), y / np.linalg.norm(y, axis=1, keepdims=True)
        return 1.0 - q @ y.T
    v = np.maximum((q * q).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (q @ y.T), 0.0)
    return np.sqrt(v.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64) if metric == "euclidean" else v


def numpy_w(kind, d, a, b):
    a, b = a[:, None], b[None, :]
    with np.errstate(all="ignore"):
        return {"csls": lambda: 2.0 * d - a - b, "dual": lambda: (d - a) - b, "nicdm": lambda: d / np.sqrt(a * b),
                "ls": lambda: 1.0 - np.exp(-(d * d) / (a * b))}[kind]()


def check(kind, metric, d, k, k_seed, n_q=300, n_i=4097, dtype=np.float32, seed=0, benign=True, q_begin=0, spoil=None, spread=(0.5, 2.0), **kw):
    """One case: states (t_a = `spread` x the mean distance), seeds = the k_seed nearest rows by plain distance, both routes.
    kw: make_case's options (Gaussian data) -- none: latent_case.  spoil(q_a, t_a): edits the state in place."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    q, y = make_case(n_q, n_i, d, seed, **kw) if kw else latent_case(n_q, n_i, d, seed)
    dist = numpy_distances(q, y, metric)
    rng = np.random.default_rng(seed + 1)
    mean = dist.mean()
    q_a, t_a = rng.uniform(0.8, 1.2, n_q) * mean, rng.uniform(*spread, n_i) * mean
    if spoil:
        spoil(q_a, t_a)
    q_state, t_state = [q_a[q_begin:]], [t_a]
    if kind == "mp_normal":
        q_state, t_state = q_state + [np.full(n_q - q_begin, 0.3 * mean)], t_state + [np.full(n_i, 0.3 * mean)]
    seeds = np.argsort(dist, axis=1, kind="stable")[q_begin:, :k_seed].astype(np.int64)
    im, qm = N.DeviceMatrix(ctx, y.astype(dtype), metric), N.DeviceMatrix(ctx, q.astype(dtype), metric)
    dev = lambda vs: tuple(ctx.to_device(np.ascontiguousarray(v)) for v in vs)   # noqa: E731
    args = (ctx, qm, im, k, KINDS[kind], dev(q_state), dev(t_state), q_begin)
    stats = {}
    w_s, i_s = N.knn_reduced_sweep(*args[:-1], ctx.to_device(seeds), q_begin, stats=stats)
    w_e, i_e = N.knn_reduced(*args)
    print(f"{kind} {metric} d={d} k={k} k_seed={k_seed} {kw}: {stats}")
    np.testing.assert_array_equal(i_s.numpy(), i_e.numpy())
    assert w_s.numpy().tobytes() == w_e.numpy().tobytes()
    assert stats["n_rows"] == n_q - q_begin
    if not benign:
        assert stats["route_taken"] == 0
        return
    assert (stats["route_taken"], stats["overflowed"]) == (1, 0) and stats["max_err_ratio"] <= 1.0
    w = numpy_w(kind, dist, q_a, t_a)[q_begin:]
    order = np.argsort(w, axis=1, kind="stable")   # (stable: ties by row)
    ws = np.take_along_axis(w, order[:, :k + 1], 1)
    gap = ws[:, k] - ws[:, k - 1]
    tied = np.take_along_axis(dist[q_begin:], order[:, k - 1:k + 1], 1)   # (exact duplicates tie in w and go by row: no gap to ask for)
    assert ((gap >= 1e-9 * np.abs(ws[:, k])) | (tied[:, 0] == tied[:, 1])).all(), "precondition: a k-th / (k+1)-th gap below 1e-9 relative"
    outside = np.array([not set(order[r, :k]) <= set(seeds[r]) for r in range(len(seeds))]).mean()
    assert outside > 0 or spread[0] == spread[1], "precondition: no whole-index list leaves its seed list"
    np.testing.assert_array_equal(i_s.numpy(), order[:, :k])


@pytest.mark.parametrize("d", [17, 144, 224, 384])
def test_widths(d):
    check("csls", "euclidean", d, 10, 10)


@pytest.mark.parametrize("k,k_seed", [(1, 1), (1, 5), (10, 16), (64, 64), (64, 80)])
def test_neighbours_and_seeds(k, k_seed):
    check("csls", "cosine", 144, k, k_seed)


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cosine"])
@pytest.mark.parametrize("kind", ["csls", "ls", "nicdm", "dual"])
def test_kinds_and_metrics(kind, metric):
    check(kind, metric, 144, 10, 10)


@pytest.mark.parametrize("kw", [dict(q_begin=37), dict(dups=40, spread=(1.0, 1.0)), dict(scale=1e-3, spread=(0.98, 1.02)),
                                dict(offset=1.0, spread=(0.98, 1.02))], ids=str)
def test_edges(kw):
    """A row range; exact duplicate index rows with one state (ties in w, ordered by row); data far from unit scale."""
    check("csls", "euclidean", 96, 10, 12, **kw)


def _set(side, at, value):
    def spoil(q_a, t_a):
        (q_a if side == "q" else t_a)[at] = value
    return spoil


@pytest.mark.parametrize("kind,kw", [
    ("csls", dict(dtype=np.float64)), ("mp_normal", {}), ("csls", dict(k=129, k_seed=129)), ("csls", dict(n_i=127)),
    ("csls", dict(spoil=_set("t", 4000, np.nan))), ("nicdm", dict(spoil=_set("t", 77, -1.0))), ("ls", dict(spoil=_set("q", 5, 1e-9))),
], ids=["float64", "mp_normal", "k129", "127rows", "nan_state", "negative_state", "ls_tau_1"])
def test_must_take_the_exact_route(kind, kw):
    kw = dict(dict(k=10, k_seed=10), **kw)
    check(kind, "euclidean", 64, kw.pop("k"), kw.pop("k_seed"), benign=False, spread=(0.9, 1.1), dups=0, **kw)


def test_kiez_end_to_end():
    from kiez_amd import Kiez
    rng = np.random.default_rng(5)
    source, target = rng.standard_normal((300, 64)).astype(np.float32), rng.standard_normal((4097, 64)).astype(np.float32)
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness="CSLS").fit(source, target)
    dist_s, ind_s = kz.hubness.kneighbors_whole_index(10, route="sweep")
    assert kz.algorithm.reduced_stats_["route_taken"] == 1 and kz.algorithm.reduced_stats_["max_err_ratio"] <= 1.0
    dist_e, ind_e = kz.kneighbors_whole_index(10)
    np.testing.assert_array_equal(ind_s, ind_e)
    assert dist_s.tobytes() == dist_e.tobytes() and kz.algorithm.reduced_stats_ is None
    gold = ind_s[:, 3].copy()
    np.testing.assert_array_equal(kz.gold_ranks(gold, reduced=True), np.full(300, 3))
    with pytest.raises(ValueError):
        kz.hubness.kneighbors_whole_index(10, route="fast")
