"""metric='precomputed' on the device: kz_knn on the two views of a distance matrix against the numpy restatement
(tests/precomputed_restate.py) at the edges of the 64 x 64 transpose tile, of the 16-byte load path and of the selection chunks; more
than one value batch; a listed-row subset with holes (gold ranks); the anchor -- a matrix of the library's own distances gives the
embedding path's results bit for bit under every reduction; float32 matrices; every input kind; validation; refusals at the ABI.
`pytest -m gpu`.

Every comparison is exact (values' bits and indices): the feature performs no arithmetic on the values before the existing kernels
see them."""
import ctypes as C
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import precomputed_restate as PR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KZ_OK, KZ_ERR_INVALID, KZ_ERR_NONFINITE = 0, 1, 5


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _knn(ctx, query, index, k, q_begin=0, q_count=None):
    from kiez_amd import _native as N
    dist, ind, _ = N.knn(ctx, query, index, k, q_begin=q_begin, q_count=q_count)
    return dist.numpy(), ind.numpy()


def _check_both_directions(ctx, D, ks, where):
    """kz_knn rows -> columns and columns -> rows of D against the restatement, for every k of `ks` the index admits."""
    from kiez_amd import _native as N
    rows, cols = N.DeviceMatrix.precomputed(ctx, D)
    assert rows.shape == D.shape and cols.shape == D.shape[::-1] and rows.dtype == D.dtype == cols.dtype
    for s_to_t, query, index in ((True, rows, cols), (False, cols, rows)):
        for k in sorted({min(k, index.shape[0]) for k in ks}):
            want_d, want_i = PR.knn(D, k, s_to_t)
            got_d, got_i = _knn(ctx, query, index, k)
            msg = f"{where} {D.shape} {D.dtype} k={k} {'rows' if s_to_t else 'columns'} direction"
            np.testing.assert_array_equal(got_i, want_i, err_msg=msg)
            np.testing.assert_array_equal(got_d, want_d, err_msg=msg)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_searches_at_the_tile_and_vector_edges(ctx, dtype):
    """Extents {1, 63, 64, 65, 129} on both sides: the edges of the transpose tile and of the 16-byte loads (an odd n_cols makes the
    row starts alternate in alignment)."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(11)
    for n_rows in (1, 63, 64, 65, 129):
        for n_cols in (1, 63, 64, 65, 129):
            _check_both_directions(ctx, rng.random((n_rows, n_cols)).astype(dtype), (1, 10, 64), "edges")
    # kz_matrix_shape: (n, the other extent, dtype, KZ_PRECOMPUTED)
    rows, cols = N.DeviceMatrix.precomputed(ctx, rng.random((63, 129)).astype(dtype))
    for m, want in ((rows, (63, 129)), (cols, (129, 63))):
        n, d, dt, metric = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        assert ctx.lib.kz_matrix_shape(m.handle, C.byref(n), C.byref(d), C.byref(dt), C.byref(metric)) == KZ_OK
        assert (n.value, d.value, dt.value, metric.value) == want + (N.KZ_F32 if dtype == np.float32 else N.KZ_F64, N.KZ_PRECOMPUTED)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_searches_across_selection_chunks(ctx, dtype):
    """70 x 4 097: two selection chunks, the last of one entry.  300 x 20 500 and 20 500 x 70: six chunks -- the two-level selection
    in each direction (k = 10: the arg-min first level, k = 64: the radix one)."""
    rng = np.random.default_rng(12)
    for shape in ((70, 4097), (300, 20500), (20500, 70)):
        _check_both_directions(ctx, rng.random(shape).astype(dtype), (1, 10, 64), "chunks")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_row_ranges_and_ties(ctx, dtype):
    from kiez_amd import _native as N
    rng = np.random.default_rng(13)
    D = rng.random((201, 333)).astype(dtype)
    rows, cols = N.DeviceMatrix.precomputed(ctx, D)
    for s_to_t, query, index in ((True, rows, cols), (False, cols, rows)):
        want_d, want_i = PR.knn(D, 10, s_to_t)
        for q_begin, q_count in ((0, 1), (1, 63), (37, 101), (130, 71), (query.shape[0] - 1, 1)):
            got_d, got_i = _knn(ctx, query, index, 10, q_begin, q_count)
            np.testing.assert_array_equal(got_i, want_i[q_begin:q_begin + q_count])
            np.testing.assert_array_equal(got_d, want_d[q_begin:q_begin + q_count])
    # massive ties: ordered by index row exactly as the restatement (one chunk and two-level)
    for shape in ((129, 200), (70, 20500), (20500, 70)):
        _check_both_directions(ctx, rng.integers(0, 5, size=shape).astype(dtype), (1, 10, 64), "ties")


# ---- more than one value batch ---------------------------------------------------------------------------------------------------
# The batch is 256 MiB / (8 index.n) rows: 70 000 index rows give 479 rows per batch, 1 000 query rows three batches.
BIG_ROWS, BIG_COLS, BIG_BATCH = 1000, 70000, (256 << 20) // (8 * 70000)
EDGE_ROWS = [0, BIG_BATCH - 1, BIG_BATCH, BIG_BATCH + 1, 2 * BIG_BATCH - 1, 2 * BIG_BATCH, 2 * BIG_BATCH + 1, BIG_ROWS - 1]


@pytest.fixture(scope="module")
def big():
    """D [1 000, 70 000] float32, its transpose (contiguous) and the restatement's lists of the rows on both sides of each batch edge:
    computed once, shared, never changed."""
    assert BIG_BATCH == 479
    rng = np.random.default_rng(14)
    D = rng.random((BIG_ROWS, BIG_COLS), dtype=np.float32)
    want_d, want_i = PR.knn_rows(D[EDGE_ROWS], 10)
    return {"D": D, "Dt": np.ascontiguousarray(D.T), "want_d": want_d, "want_i": want_i}


@pytest.mark.parametrize("direction", ["rows", "columns"])
def test_more_than_one_value_batch(ctx, big, direction):
    """Rows direction on D; columns direction on its transpose [70 000, 1 000] -- the same lists.  A call split into two row ranges
    (other batch edges) gives the same arrays as the whole call."""
    from kiez_amd import _native as N
    if direction == "rows":
        query, index = N.DeviceMatrix.precomputed(ctx, big["D"])
    else:
        index, query = N.DeviceMatrix.precomputed(ctx, big["Dt"])
    assert query.shape[0] == BIG_ROWS and index.shape[0] == BIG_COLS
    got_d, got_i = _knn(ctx, query, index, 10)
    np.testing.assert_array_equal(got_i[EDGE_ROWS], big["want_i"])
    np.testing.assert_array_equal(got_d[EDGE_ROWS], big["want_d"])
    cut = 333
    a_d, a_i = _knn(ctx, query, index, 10, 0, cut)
    b_d, b_i = _knn(ctx, query, index, 10, cut, BIG_ROWS - cut)
    np.testing.assert_array_equal(np.concatenate([a_i, b_i]), got_i)
    np.testing.assert_array_equal(np.concatenate([a_d, b_d]), got_d)


def test_gold_ranks_of_a_listed_subset_with_holes(ctx, big):
    """gold ids for every third row plus the batch-edge rows, columns direction (s_to_t=False): the compacted list has holes, so the
    transpose kernel's lanes read columns that are no run.  Rank = position in the full sorted row; rows without gold: -1."""
    from kiez_amd.neighbors import SklearnNN
    Dt = big["Dt"]                                   # [70 000 source rows, 1 000 target rows]
    rng = np.random.default_rng(15)
    gold = np.full(BIG_ROWS, -1, dtype=np.int64)
    listed = sorted(set(range(0, BIG_ROWS, 3)) | set(EDGE_ROWS))
    gold[listed] = rng.integers(0, BIG_COLS, size=len(listed))
    nn = SklearnNN(n_candidates=10, metric="precomputed")
    nn.fit(Dt)
    got = nn.gold_ranks(gold, s_to_t=False)
    want = np.full(BIG_ROWS, -1, dtype=np.int64)
    for r in listed:
        row, g = big["D"][r], gold[r]                # (target row r against every source row: column r of Dt = row r of D)
        want[r] = int((row < row[g]).sum() + (row[:g] == row[g]).sum())
    np.testing.assert_array_equal(got, want)
    assert (got[np.setdiff1d(np.arange(BIG_ROWS), listed)] == -1).all()


# ---- the anchor ----------------------------------------------------------------------------------------------------------------
def _outcome(fn):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = fn()
        return ("ok",) + tuple(res if isinstance(res, tuple) else (res,))
    except Exception as exc:   # noqa: BLE001  (the error IS the outcome compared)
        return ("raised", type(exc), str(exc))


def _same_outcome(a, b, where):
    assert a[0] == b[0], f"{where}: {a[:3]} vs {b[:3]}"
    if a[0] == "raised":
        assert a[1:] == b[1:], where
        return
    assert len(a) == len(b), where
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and x.shape == y.shape, where
        np.testing.assert_array_equal(x, y, err_msg=where)


@pytest.fixture(scope="module")
def anchor():
    """float64 embeddings, sqeuclidean (the value is returned as it is: ordering value and returned distance coincide), and D = the
    library's own value of every pair (kz_pair_values)."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(16)
    source, target = rng.standard_normal((300, 16)), rng.standard_normal((257, 16))
    sm, tm = N.DeviceMatrix(ctx, source, "sqeuclidean"), N.DeviceMatrix(ctx, target, "sqeuclidean")
    ind = ctx.to_device(np.tile(np.arange(257, dtype=np.int64), (300, 1)))
    val = ctx.empty((300, 257), np.float64)
    N._check(ctx.lib.kz_pair_values(ctx.handle, sm.handle, 0, 300, tm.handle, ind.ptr, 257, val.ptr), "kz_pair_values")
    gold = rng.integers(0, 257, size=300).astype(np.int64)
    gold[::7] = -1
    return {"source": source, "target": target, "D": val.numpy(), "gold": gold}


def _reductions():
    from kiez_amd import InvertedSoftmax, Sinkhorn
    return [("none", None, {}), ("csls", "CSLS", {}), ("ls", "LocalScaling", {"method": "standard"}),
            ("nicdm", "LocalScaling", {"method": "nicdm"}), ("mp_normal", "MutualProximity", {"method": "normal"}),
            ("mp_empiric", "MutualProximity", {"method": "empiric"}), ("sinkhorn", Sinkhorn, {"temperature": 1.0, "n_iter": 3}),
            ("inverted_softmax", InvertedSoftmax, {"temperature": 1.0})]


@pytest.mark.parametrize("name", ["none", "csls", "ls", "nicdm", "mp_normal", "mp_empiric", "sinkhorn", "inverted_softmax"])
def test_anchor_own_distances_give_the_embedding_paths_results(anchor, name):
    from kiez_amd import Kiez
    _, hubness, kwargs = next(r for r in _reductions() if r[0] == name)
    kz_e = Kiez(n_candidates=10, algorithm_kwargs={"metric": "sqeuclidean"}, hubness=hubness, hubness_kwargs=dict(kwargs))
    kz_p = Kiez(n_candidates=10, algorithm_kwargs={"metric": "precomputed"}, hubness=hubness, hubness_kwargs=dict(kwargs))
    kz_e.fit(anchor["source"], anchor["target"])
    kz_p.fit(anchor["D"])
    assert kz_p.algorithm.source_equals_target is False
    assert kz_p.algorithm.source_index.view == "rows" and kz_p.algorithm.target_index.view == "columns"
    gold = anchor["gold"]
    calls = [("kneighbors(5)", lambda kz: kz.kneighbors(5)),
             ("kneighbors_whole_index(10)", lambda kz: kz.kneighbors_whole_index(10)),
             ("gold_ranks", lambda kz: kz.gold_ranks(gold)),
             ("gold_ranks reduced", lambda kz: kz.gold_ranks(gold, reduced=True)),
             ("match(5)", lambda kz: kz.match(5)),
             ("match(10, whole_index)", lambda kz: kz.match(10, whole_index=True))]
    n_ok = 0
    for what, call in calls:
        e, p = _outcome(lambda: call(kz_e)), _outcome(lambda: call(kz_p))
        _same_outcome(p, e, f"{name}: {what}")
        n_ok += e[0] == "ok"
    assert n_ok == (3 if name == "mp_empiric" else 6)          # (MP empiric has no value outside its lists: whole-index calls raise)
    if name in ("sinkhorn", "inverted_softmax"):
        np.testing.assert_array_equal(kz_p.hubness.source_potential_, kz_e.hubness.source_potential_)
        np.testing.assert_array_equal(kz_p.hubness.target_potential_, kz_e.hubness.target_potential_)
        assert kz_p.hubness.n_iter_ == kz_e.hubness.n_iter_


def test_reverse_direction_and_adhoc_query(anchor):
    """`query=target_` resolves to the columns view (HubnessReduction.fit's reverse search); any other array is refused."""
    from kiez_amd.neighbors import SklearnNN
    nn_e = SklearnNN(n_candidates=10, metric="sqeuclidean")
    nn_p = SklearnNN(n_candidates=10, metric="precomputed")
    nn_e.fit(anchor["source"], anchor["target"])
    nn_p.fit(anchor["D"])
    assert nn_p.target_ is not nn_p.source_ and nn_p.target_.shape == (257, 300)
    assert nn_p.kneighbors_device_both(10) is None
    for query_e, query_p, s_to_t in ((None, None, True), (None, None, False), (anchor["target"], nn_p.target_, False)):
        de, ie = nn_e.kneighbors(k=10, query=query_e, s_to_t=s_to_t)
        dp, ip = nn_p.kneighbors(k=10, query=query_p, s_to_t=s_to_t)
        np.testing.assert_array_equal(ip, ie)
        np.testing.assert_array_equal(dp, de)
    with pytest.raises(NotImplementedError, match="fitted side"):
        nn_p.kneighbors(k=3, query=anchor["D"][:5].copy())


# ---- float32 ---------------------------------------------------------------------------------------------------------------------
def test_float32_matrix(ctx):
    from kiez_amd import Kiez
    from kiez_amd.hubness_reduction import CSLS, HubnessReduction
    from kiez_amd.neighbors import SklearnNN
    rng = np.random.default_rng(17)
    D = rng.random((150, 131), dtype=np.float32)
    K, k = 10, 5
    nn = SklearnNN(n_candidates=K, metric="precomputed")
    nn.fit(D)
    for s_to_t in (True, False):
        dist, ind = nn.kneighbors(k=K, s_to_t=s_to_t)
        want_d, want_i = PR.knn(D, K, s_to_t)
        assert dist.dtype == np.float32 and ind.dtype == np.int64
        np.testing.assert_array_equal(ind, want_i)
        np.testing.assert_array_equal(dist, want_d.astype(np.float32))
    # CSLS through the facade == the existing transform path fed the restatement's lists (float64 on the widened values, cast at the end)
    kz = Kiez(n_candidates=K, algorithm_kwargs={"metric": "precomputed"}, hubness="CSLS").fit(D)
    got_d, got_i = kz.kneighbors(k)
    fwd_d, fwd_i = PR.knn(D, K, True)
    rev_d, rev_i = PR.knn(D, K, False)
    hub = CSLS(nn_algo=SklearnNN(n_candidates=K, metric="precomputed"))
    hub._fit(ctx.to_device(rev_d), ctx.to_device(rev_i), None, None)
    hd, hi = hub.transform(ctx.to_device(fwd_d), ctx.to_device(fwd_i), None)
    od, oi = HubnessReduction._sort(hd, hi, k, ctx=ctx)
    assert got_d.dtype == np.float32
    np.testing.assert_array_equal(got_i, oi.numpy())
    np.testing.assert_array_equal(got_d, od.numpy().astype(np.float32))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def test_numpy_and_device_array_inputs_and_destroy_order(ctx):
    from kiez_amd import _native as N
    from kiez_amd.neighbors import SklearnNN
    rng = np.random.default_rng(18)
    D = rng.random((97, 150))
    want = PR.knn(D, 7, True) + PR.knn(D, 7, False)
    dev = ctx.to_device(D)
    for data in (D, dev, np.asfortranarray(D)):       # (copied; borrowed in place; a non-contiguous array, made contiguous)
        nn = SklearnNN(n_candidates=7, metric="precomputed")
        nn.fit(data)
        assert nn.source_index.dtype == np.float64 and nn.source_ is data
        got = nn.kneighbors(k=7) + nn.kneighbors(k=7, s_to_t=False)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    # an integer matrix is cast to float64, as embeddings are
    Di = rng.integers(0, 50, size=(20, 30))
    nn = SklearnNN(n_candidates=4, metric="precomputed")
    nn.fit(Di)
    assert nn.source_index.dtype == np.float64
    np.testing.assert_array_equal(nn.kneighbors(k=4)[1], PR.knn(Di, 4)[1])
    # the two views share one storage: destroying them in either order is clean, and the survivor's pair still answers until then
    for first in (0, 1):
        for borrow in (False, True):
            views = list(N.DeviceMatrix.precomputed(ctx, D) if not borrow else
                         N.DeviceMatrix.precomputed(ctx, None, device_ptr=dev.ptr.value, shape=dev.shape, dtype=dev.dtype, borrow=True,
                                                    keepalive=dev))
            got_d, got_i = _knn(ctx, views[0], views[1], 7)
            np.testing.assert_array_equal(got_i, want[1])
            np.testing.assert_array_equal(got_d, want[0])
            assert ctx.lib.kz_matrix_destroy(views[first].handle) == KZ_OK
            views[first].handle = None
            assert ctx.lib.kz_matrix_destroy(views[1 - first].handle) == KZ_OK
            views[1 - first].handle = None
    ctx.sync()
    np.testing.assert_array_equal(dev.numpy(), D)     # (a borrowed buffer is the caller's: still there, unchanged)


TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd import Kiez
from kiez_amd.neighbors import SklearnNN
from tests import precomputed_restate as PR
rng = np.random.default_rng(19)
D = rng.random((90, 141), dtype=np.float32)
wide = rng.random((90, 282), dtype=np.float32)
wide[:, ::2] = D
t_contig = torch.from_numpy(D).cuda()
t_strided = torch.from_numpy(wide).cuda()[:, ::2]              # (non-contiguous: made contiguous by the backend)
assert not t_strided.is_contiguous()
for t in (t_contig, t_strided, torch.from_numpy(D)):           # (a CPU tensor goes through its numpy view)
    nn = SklearnNN(n_candidates=6, metric="precomputed")
    nn.fit(t)
    for s_to_t in (True, False):
        dist, ind = nn.kneighbors(k=6, s_to_t=s_to_t)
        assert isinstance(dist, torch.Tensor) and dist.dtype == torch.float32 and ind.dtype == torch.int64
        assert dist.is_cuda == t.is_cuda
        want_d, want_i = PR.knn(D, 6, s_to_t)
        assert np.array_equal(ind.cpu().numpy(), want_i) and np.array_equal(dist.cpu().numpy(), want_d.astype(np.float32))
    kz = Kiez(n_candidates=6, algorithm_kwargs={"metric": "precomputed"}, hubness="CSLS").fit(t)
    kz_np = Kiez(n_candidates=6, algorithm_kwargs={"metric": "precomputed"}, hubness="CSLS").fit(D)
    dist, ind = kz.kneighbors(3)
    dist_np, ind_np = kz_np.kneighbors(3)
    assert isinstance(dist, torch.Tensor) and dist.dtype == torch.float32
    assert np.array_equal(ind.cpu().numpy(), ind_np) and np.array_equal(dist.cpu().numpy(), dist_np)
print("TORCH_OK")
"""


def test_torch_tensor_inputs():
    """A CUDA tensor (borrowed, tensors out), a non-contiguous one and a CPU tensor (in a child process: torch must load its HIP
    runtime first)."""
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- validation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_validation(ctx, dtype):
    """One bad value in the LAST element of a 65 x 129 matrix.  Host values: ValueError at fit.  A borrowed device matrix: ValueError
    at the first search (of any kind).  -0.0 is accepted."""
    from kiez_amd import _native as N
    from kiez_amd.neighbors import SklearnNN
    rng = np.random.default_rng(20)
    base = rng.random((65, 129)).astype(dtype)
    for bad, match in ((np.nan, "NaN or infinity"), (np.inf, "NaN or infinity"), (-np.inf, "NaN or infinity"),
                       (-1.0, "Negative values in data passed to precomputed distance matrix")):
        D = base.copy()
        D[-1, -1] = bad
        with pytest.raises(ValueError, match=match):
            SklearnNN(n_candidates=3, metric="precomputed").fit(D)
        dev = ctx.to_device(D)
        nn = SklearnNN(n_candidates=3, metric="precomputed")
        nn.fit(dev)                                  # (borrowed: nothing is waited for)
        with pytest.raises(ValueError, match=match):
            nn.kneighbors(k=3)
        with pytest.raises(ValueError, match=match):
            nn.kneighbors(k=3, s_to_t=False)
        with pytest.raises(ValueError, match=match):
            nn.gold_ranks(np.zeros(65, dtype=np.int64))
        with pytest.raises(ValueError, match=match):
            N.softmin_rows(ctx, nn.source_index, nn.target_index, 1.0)
    D = base.copy()
    D[-1, -1] = -0.0
    D[0, 0] = -0.0
    for data in (D, ctx.to_device(D)):
        nn = SklearnNN(n_candidates=3, metric="precomputed")
        nn.fit(data)
        dist, ind = nn.kneighbors(k=3)
        np.testing.assert_array_equal(ind, PR.knn(D, 3)[1])
        assert ind[0, 0] == 0 and ind[-1, 0] == 128


# ---- refusals at the ABI ----------------------------------------------------------------------------------------------------------
def test_refusals_at_the_abi(ctx):
    from kiez_amd import _native as N
    lib = ctx.lib
    rng = np.random.default_rng(21)
    D = rng.random((40, 40))
    rows_a, cols_a = N.DeviceMatrix.precomputed(ctx, D)
    rows_b, cols_b = N.DeviceMatrix.precomputed(ctx, D)
    emb = N.DeviceMatrix(ctx, rng.random((40, 40)), "sqeuclidean")
    dist, ind = ctx.empty((40, 5), np.float64), ctx.empty((40, 5), np.int64)
    sentinel = np.full((40, 5), -7.0)
    dist.fill_from_host(sentinel)

    def knn(q, i, exclude_self=0):
        return lib.kz_knn(ctx.handle, q.handle, 0, 40, i.handle, 5, exclude_self, dist.ptr, ind.ptr, None)

    def message():
        return lib.kz_last_error().decode()
    assert knn(rows_a, cols_a) == KZ_OK
    dist.fill_from_host(sentinel)
    assert knn(rows_a, cols_b) == KZ_ERR_INVALID and "different precomputed matrices" in message()
    assert knn(cols_b, rows_a) == KZ_ERR_INVALID
    assert knn(rows_a, rows_a) == KZ_ERR_INVALID and "same view" in message()
    assert knn(cols_a, cols_a) == KZ_ERR_INVALID
    assert knn(rows_a, emb) == KZ_ERR_INVALID and "embedding matrix" in message()
    assert knn(emb, cols_a) == KZ_ERR_INVALID and "embedding matrix" in message()
    assert knn(rows_a, cols_a, exclude_self=1) == KZ_ERR_INVALID and "exclude_self" in message()
    gold, rank = ctx.to_device(np.zeros(40, dtype=np.int64)), ctx.empty((40,), np.int64)
    assert lib.kz_gold_ranks(ctx.handle, rows_a.handle, 0, 40, rows_a.handle, gold.ptr, rank.ptr) == KZ_ERR_INVALID
    assert lib.kz_gold_ranks(ctx.handle, rows_a.handle, 0, 40, emb.handle, gold.ptr, rank.ptr) == KZ_ERR_INVALID
    out = ctx.empty((40,), np.float64)
    assert lib.kz_softmin_rows(ctx.handle, cols_a.handle, 0, 40, rows_b.handle, 1.0, None, 0.0, out.ptr) == KZ_ERR_INVALID
    d2, i2 = ctx.empty((40, 5), np.float64), ctx.empty((40, 5), np.int64)
    assert lib.kz_knn_dual(ctx.handle, rows_a.handle, cols_a.handle, 5, dist.ptr, ind.ptr, d2.ptr, i2.ptr, None, None) == KZ_ERR_INVALID
    assert "precomputed" in message()
    cand = ctx.to_device(np.zeros((40, 5), dtype=np.int64))
    assert lib.kz_pair_values(ctx.handle, rows_a.handle, 0, 40, cols_a.handle, cand.ptr, 5, dist.ptr) == KZ_ERR_INVALID
    assert "precomputed" in message()
    t2c = ctx.empty((40,), np.float64)
    assert lib.kz_dsl_fit(ctx.handle, cand.ptr, 40, 5, rows_a.handle, cols_a.handle, 0, t2c.ptr) == KZ_ERR_INVALID
    assert "precomputed" in message()
    gmin = ctx.to_device(np.array([np.inf]))
    assert lib.kz_dsl_transform(ctx.handle, cand.ptr, 40, 5, rows_a.handle, 0, cols_a.handle, t2c.ptr, dist.ptr,
                                gmin.ptr) == KZ_ERR_INVALID
    assert lib.kz_matrix_set_minkowski_p(rows_a.handle, 3.0) == KZ_ERR_INVALID and "precomputed" in message()
    V = np.ones(40)
    assert lib.kz_matrix_set_seuclidean_v(cols_a.handle, V.ctypes.data_as(C.c_void_p), 40) == KZ_ERR_INVALID
    assert "precomputed" in message()
    ctx.sync()
    np.testing.assert_array_equal(dist.numpy(), sentinel)          # (no refusal wrote anything)
    # kz_matrix_create keeps refusing the id
    h = C.c_void_p()
    assert lib.kz_matrix_create(ctx.handle, D.ctypes.data_as(C.c_void_p), 0, 40, 40, N.KZ_F64, N.KZ_PRECOMPUTED,
                                C.byref(h)) == KZ_ERR_INVALID
    assert "unknown metric" in message() and not h.value
    # the constructor's own argument checks
    r, c = C.c_void_p(), C.c_void_p()
    for n_rows, n_cols, dtype, where in ((0, 40, N.KZ_F64, 0), (40, 0, N.KZ_F64, 0), (40, 40, 2, 0), (40, 40, N.KZ_F64, 3),
                                         ((1 << 31) - 256, 1, N.KZ_F64, 0)):
        assert lib.kz_matrix_create_precomputed(ctx.handle, D.ctypes.data_as(C.c_void_p), where, n_rows, n_cols, dtype, C.byref(r),
                                                C.byref(c)) == KZ_ERR_INVALID
        assert not r.value and not c.value
