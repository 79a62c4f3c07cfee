"""scipy's seven boolean metrics on the MI355X (bit-packed rows, kz_bool_dist_kernel): the C ABI against scikit-learn's brute-force
search (distances bit for bit, indices equal except inside runs of equal distances), all-false rows under dice and sokalsneath, the
Kiez pipeline against the reference's goldens (tools/gen_golden_boolean.py), non-float inputs, torch tensors, ad-hoc queries and
two ShardedKiez ranks."""
import os
import socket
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import boolean_restate as BR
from tests.golden_util import GOLDEN, HUB, knife_edge_rows

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
METRICS = BR.BOOLEAN_METRICS
MIN_COMPARABLE = 45     # rows (of 90) of a golden case whose candidate set must be the reference's: see the pipeline test
# (n_q, n_i, d, k): d crosses the image's word (32) and row-padding (128) edges and the kernel's 16-word LDS stage (512);
# n_q and n_i are no multiples of the 64 x 64 tile
SHAPES = ((100, 700, 5, 7), (65, 333, 31, 10), (70, 1301, 32, 10), (257, 1301, 33, 10), (33, 900, 127, 5), (130, 5000, 128, 50),
          (63, 1000, 129, 9), (31, 300, 513, 3), (40, 2500, 2049, 200))


def _data(rng, n, d, dtype, density=0.5):
    """Rows whose true features carry arbitrary nonzero values (truth is x != 0), false ones +0.0 or -0.0."""
    on = rng.random((n, d)) < density
    v = np.where(on, rng.uniform(0.5, 3.0, (n, d)) * rng.choice([-1.0, 1.0], (n, d)), rng.choice([0.0, -0.0], (n, d)))
    return v.astype(dtype)


def _sklearn(metric, y, q, k):
    from sklearn.neighbors import NearestNeighbors
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (DataConversionWarning: the rows are cast to bool)
        return NearestNeighbors(n_neighbors=k, algorithm="brute", metric=metric).fit(y).kneighbors(q)


def _check(metric, dd, ii, sd, si, q, y):
    """Distances: scikit-learn's bits (NaN where scikit-learn has NaN).  Indices: equal except inside runs of equal distances -- a
    run that reaches the k-th place may hold other rows of that distance than scikit-learn's (its order among ties is unstable):
    every row the device returned has the distance it was returned with (restated), no row twice, and below the last run the
    rows of every distance are scikit-learn's."""
    np.testing.assert_array_equal(dd, sd)
    for r in range(len(dd)):
        assert len(set(ii[r])) == len(ii[r]), (metric, r)
        got = BR.ranking_values(metric, q[r:r + 1], y[ii[r]])[0]
        np.testing.assert_array_equal(got, dd[r], err_msg=f"{metric} row {r}")
        key_d, key_s = np.nan_to_num(dd[r], nan=np.inf), np.nan_to_num(sd[r], nan=np.inf)
        for v in np.unique(key_d[key_d < key_d[-1]]):
            assert set(ii[r][key_d == v]) == set(si[r][key_s == v]), (metric, r, v)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_against_scikit_learn(metric, dtype):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(23)
    for n_q, n_i, d, k in SHAPES:
        density = 0.5 if d > 5 else 0.4
        q, y = _data(rng, n_q, d, dtype, density), _data(rng, n_i, d, dtype, density)
        qm, im = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
        dd, ii, st = N.knn(ctx, qm, im, k)
        sd, si = _sklearn(metric, y, q, k)
        _check(metric, dd.numpy(), ii.numpy(), sd, si, q, y)
        assert st["n_fallback_rows"] == n_q, st   # (the exact route: no MFMA tier, no range re-search, no speculative rows)


@pytest.mark.parametrize("metric", METRICS)
def test_self_query_with_duplicates(metric):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(5)
    y = _data(rng, 600, 70, np.float32)
    y[17] = y[400]
    y[31] = y[32] = y[33]
    m = N.DeviceMatrix(ctx, y, metric)
    dd, ii, _ = N.knn(ctx, m, m, 6, exclude_self=True)
    rd, ri = BR.knn(metric, y, y, 6, exclude_self=True)
    _check(metric, dd.numpy(), ii.numpy(), rd, ri, y, y)
    np.testing.assert_array_equal(ii.numpy(), ri)       # (the device order IS (value, index row))
    assert not (ii.numpy() == np.arange(600)[:, None]).any()


@pytest.mark.parametrize("metric", ["dice", "sokalsneath"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_all_false_rows_are_nan_and_last(metric, dtype):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(2)
    y, q = _data(rng, 500, 45, dtype, 0.3), _data(rng, 40, 45, dtype, 0.3)
    y[[3, 77, 300]] = 0.0          # all-false index rows: NaN against an all-false query only
    y[77, ::2] = -0.0
    q[[0, 9]] = 0.0                # all-false query rows
    qm, im = N.DeviceMatrix(ctx, q, metric), N.DeviceMatrix(ctx, y, metric)
    dd, ii, _ = N.knn(ctx, qm, im, 500)
    dd, ii = dd.numpy(), ii.numpy()
    sd, si = _sklearn(metric, y, q, 500)
    _check(metric, dd, ii, sd, si, q, y)
    rd, ri = BR.knn(metric, q, y, 500)
    np.testing.assert_array_equal(dd, rd)
    np.testing.assert_array_equal(ii, ri)
    empty = np.zeros(40, dtype=bool)
    empty[[0, 9]] = True
    assert np.isfinite(dd[~empty]).all()
    assert np.isnan(dd[empty, -3:]).all() and np.isfinite(dd[empty, :-3]).all()
    assert (ii[empty, -3:] == np.array([3, 77, 300])).all()          # (NaN last, by row)
    # ... and through the facade
    from kiez_amd.neighbors import SklearnNN
    nn = SklearnNN(n_candidates=500, metric=metric)
    nn.fit(q, y)
    fd, fi = nn.kneighbors(k=500)
    np.testing.assert_array_equal(fd, rd)
    np.testing.assert_array_equal(fi, ri)


@pytest.mark.parametrize("metric", ["russellrao", "dice", "jaccard"])
def test_query_is_the_index(metric):
    """A matrix searched against itself without self removal (the reverse pass of a single-source hubness fit): scikit-learn takes
    X is Y through pdist + squareform, whose diagonal is 0 whatever the metric says of a row and itself (russellrao: (n - nx) / n,
    dice of an all-false row: NaN).  The device returns that 0 (kz_bool.h: kz_bool_self_zero); a copy of the rows is another matrix
    and has the metric's own values, as scikit-learn's cdist route."""
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(19)
    y = _data(rng, 700, 90, np.float64, 0.4)
    y[[5, 130]] = 0.0
    m = N.DeviceMatrix(ctx, y, metric)
    dd, ii, _ = N.knn(ctx, m, m, 7)
    sd, si = _sklearn(metric, y, y, 7)                     # (the fitted array itself: X is Y)
    np.testing.assert_array_equal(dd.numpy(), sd)
    assert (dd.numpy()[:, 0] == 0).all() and (ii.numpy()[:, 0] == np.arange(700))[np.setdiff1d(np.arange(700), [5, 130])].all()
    m2 = N.DeviceMatrix(ctx, y.copy(), metric)
    d2, i2, _ = N.knn(ctx, m2, m, 7)
    sd2, si2 = _sklearn(metric, y, y.copy(), 7)            # (another array: cdist)
    _check(metric, d2.numpy(), i2.numpy(), sd2, si2, y, y)
    if metric == "russellrao":
        assert (d2.numpy()[:, 0] > 0).all()


def _runs_equal(rd, ri, d, i, rtol):
    """Indices equal except inside runs of (to rtol) equal reference distances; the run that reaches the k-th place may hold other
    rows of that distance than the reference's."""
    if np.array_equal(ri, i):
        return True
    rd, d = np.nan_to_num(rd, nan=np.inf), np.nan_to_num(d, nan=np.inf)
    for r in np.flatnonzero((ri != i).any(axis=1)):
        last = np.isclose(rd[r], rd[r][-1], rtol=rtol, atol=0) | (rd[r] == rd[r][-1])
        for p in np.flatnonzero((ri[r] != i[r]) & ~last):
            tied = np.isclose(rd[r], rd[r][p], rtol=rtol, atol=0) | (rd[r] == rd[r][p])
            if set(ri[r][tied]) != set(i[r][tied]):
                return False
    return True


def _golden_cases():
    return sorted(p.stem for p in GOLDEN.glob("boolean_*.npz"))


@pytest.mark.parametrize("case", _golden_cases())
def test_kiez_pipeline_against_the_reference(case):
    """Values are ratios of small integers: where a tie runs across the K-th candidate, scikit-learn's unstable order and the device's
    (value, index row) order keep different candidate sets -- both right.  Without hubness reduction the distances are compared
    bit for bit and the indices outside runs of equal distances.  CSLS / LocalScaling / MP normal read the candidates' distances
    only: the rows whose candidate set is the reference's are compared, and at least MIN_COMPARABLE of the 90 rows must be such
    rows.  MP empiric counts through the reverse LISTS, ties in nearly every one of them: shape and finiteness only (its exact check
    is test_two_ranks_equal_one)."""
    from kiez_amd import Kiez
    z = np.load(GOLDEN / f"{case}.npz")
    g = {k: z[k] for k in z.files}
    metric, K = str(g["metric"]), int(g["K"])
    ks = [None if k < 0 else int(k) for k in g["ks"]]
    akw = {"metric": metric}
    tags = sorted({k.split("__")[0] for k in g if "__" in k})
    assert len(tags) == (1 if case == "boolean_dice_empty_rows" else 7)
    for tag in tags:
        hname, kw = HUB[tag]
        if f"{tag}__raises" in g:
            with pytest.raises(ValueError, match="only supports"):
                Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs=akw, hubness=hname, hubness_kwargs=dict(kw))
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs=akw, hubness=hname, hubness_kwargs=dict(kw))
            kz.fit(g["source"], g.get("target"))
            if g["source"].dtype == np.bool_:
                assert kz.algorithm.target_index.dtype == np.float32     # (bool rows go up as float32)
            for k in ks:
                d, i = kz.kneighbors(k)
                kt = "None" if k is None else str(k)
                rd, ri = g[f"{tag}__k{kt}__dist"], g[f"{tag}__k{kt}__ind"]
                assert d.dtype == np.float64 and d.shape == rd.shape
                if tag == "none":
                    np.testing.assert_array_equal(d, rd)          # (the k smallest values are the same whatever the tie order)
                    assert _runs_equal(rd, ri, d, i, 0.0), (case, k)
                    continue
                if tag == "mp_empiric":
                    assert np.isfinite(d).all()
                    continue
                _, ci = kz.algorithm.kneighbors(k=K)
                same = np.array([set(a) == set(b) for a, b in zip(ci, g[f"{tag}__ind_s2t"])])
                print(case, tag, k, "comparable rows:", int(same.sum()), "of", len(same))
                assert same.sum() >= MIN_COMPARABLE, (case, tag, same.sum())
                np.testing.assert_allclose(d[same], rd[same], rtol=1e-12, atol=1e-15)
                assert _runs_equal(rd[same], ri[same], d[same], i[same], 1e-12), (case, tag, k)


def test_non_float_inputs():
    """bool and int64 rows give the float32 rows' results, and the fitted index is float32."""
    from kiez_amd.neighbors import SklearnNN
    rng = np.random.default_rng(11)
    s, t = rng.random((300, 77)) < 0.4, rng.random((260, 77)) < 0.4
    for metric in ("jaccard", "yule"):
        res = []
        for conv in (lambda a: a.astype(np.float32), lambda a: a, lambda a: a.astype(np.int64) * 7):
            nn = SklearnNN(n_candidates=9, metric=metric)
            nn.fit(conv(s), conv(t))
            assert nn.source_index.dtype == np.float32 and nn.target_index.dtype == np.float32
            res.append(nn.kneighbors(k=9) + nn.kneighbors(k=4, query=conv(s[:50])))     # (fitted and ad-hoc query)
        for other in res[1:]:
            for a, b in zip(res[0], other):
                np.testing.assert_array_equal(a, b)
        rd, ri = BR.knn(metric, s, t, 9)
        np.testing.assert_array_equal(res[0][0], rd)
        np.testing.assert_array_equal(res[0][1], ri)


TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd.neighbors import SklearnNN
from tests import test_gpu_boolean_metrics as T
for metric in T.METRICS:
    rng = np.random.default_rng(8)
    y = T._data(rng, 900, 137, np.float32)
    q = T._data(rng, 70, 137, np.float32)
    nn = SklearnNN(n_candidates=9, metric=metric)
    nn.fit(torch.from_numpy(y).cuda())
    dt, it = nn.kneighbors(k=9, query=torch.from_numpy(q).cuda())
    assert isinstance(dt, torch.Tensor) and dt.is_cuda and dt.dtype == torch.float64 and it.dtype == torch.int64
    sd, si = T._sklearn(metric, y, q, 9)
    T._check(metric, dt.cpu().numpy(), it.cpu().numpy(), sd, si, q, y)
    nn2 = SklearnNN(n_candidates=9, metric=metric)
    nn2.fit(y)
    d2, i2 = nn2.kneighbors(k=9, query=q)        # (an ad-hoc numpy query)
    assert d2.dtype == np.float64
    T._check(metric, d2, i2, sd, si, q, y)
    nn3 = SklearnNN(n_candidates=9, metric=metric)
    nn3.fit(torch.from_numpy(y != 0).cuda())     # (a bool tensor: float32 on the device)
    d3, i3 = nn3.kneighbors(k=9, query=torch.from_numpy(q != 0).cuda())
    assert nn3.source_index.dtype == np.float32
    assert np.array_equal(d3.cpu().numpy(), dt.cpu().numpy()) and np.array_equal(i3.cpu().numpy(), it.cpu().numpy())
print("TORCH_OK")
"""


def test_torch_tensors_and_adhoc_query():
    """Torch device tensors in, tensors out (in a child process: torch must load its HIP runtime first)."""
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


SCRIPT = r"""
import os, sys, warnings
sys.path.insert(0, %r)
os.environ["KIEZ_AMD_WITH_TORCH"] = "1"
import numpy as np
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
from kiez_amd import Kiez
from kiez_amd.distributed import HipEngine, ShardedKiez, row_slice
from tests.staged_comm import StagedComm
warnings.simplefilter("ignore")
eng = HipEngine(0)
eng.ctx.set_option("dual_force", 1)
rng = np.random.RandomState(3)
src = (rng.rand(1501, 150) < 0.4).astype(np.float32)
tgt = (rng.rand(1203, 150) < 0.4).astype(np.float32)
b, c = row_slice(len(src), rank, world)
K, k = 8, 5
for metric in ("jaccard", "russellrao", "yule"):
    akw = {"metric": metric}
    for hub, kw in ((None, {}), ("CSLS", {}), ("MutualProximity", {"method": "empiric"}), ("LocalScaling", {"method": "nicdm"})):
        sk = ShardedKiez(n_candidates=K, algorithm_kwargs=akw, hubness=hub, hubness_kwargs=kw, engine=eng, comm=StagedComm())
        sk.fit(src[b:b + c], tgt if rank == 0 else None)
        d, i = sk.kneighbors(k)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        one = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs=akw, hubness=hub, hubness_kwargs=kw)
        one.fit(src, tgt)
        od, oi = one.kneighbors(k)
        od, oi = od[b:b + c], oi[b:b + c]
        assert np.array_equal(d, od, equal_nan=True), (metric, hub)
        assert np.array_equal(i, oi), (metric, hub)
        print(rank, metric, hub, "ok", flush=True)
dist.barrier()
dist.destroy_process_group()
print("RANKS_OK", rank)
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one():
    world, port = 2, _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen([sys.executable, "-c", SCRIPT % str(ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rank, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"RANKS_OK {rank}" in out, f"rank {rank}:\n{out[-2000:]}\n{err[-4000:]}"
