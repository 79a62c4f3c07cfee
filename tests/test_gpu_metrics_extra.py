"""braycurtis, seuclidean, correlation and hamming on the MI355X: the C ABI against scikit-learn's brute-force search (distances bit for
bit, indices equal except inside runs of equal distances), the Kiez pipeline against the reference's goldens
(tools/gen_golden_metrics.py), torch tensors, ad-hoc queries, constant rows under correlation, and two ShardedKiez ranks."""
import os
import socket
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import metric_restate as MR
from tests.golden_util import GOLDEN, HUB, knife_edge_rows

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
METRICS = MR.EXTRA_METRICS


def _data(rng, n, d, dtype, metric):
    if metric == "hamming":
        return rng.integers(0, 3, (n, d)).astype(dtype)
    return rng.standard_normal((n, d)).astype(dtype)


def _V(rng, d, metric):
    return rng.uniform(0.5, 2.0, d) if metric == "seuclidean" else None


def _sklearn(metric, y, q, k, V):
    from sklearn.neighbors import NearestNeighbors
    kw = {"metric_params": {"V": V}} if V is not None else {}
    return NearestNeighbors(n_neighbors=k, algorithm="brute", metric=metric, **kw).fit(y).kneighbors(q)


def _check(metric, dd, ii, sd, si, q, y, V):
    """Distances: scikit-learn's bits (NaN where scikit-learn has NaN).  Indices: equal except inside runs of equal distances -- a
    run that reaches the k-th place may hold other rows of that distance than scikit-learn's (its order among ties is unstable):
    every row the device returned has the distance it was returned with (restated), no row twice, and below the last run the
    rows of every distance are scikit-learn's."""
    np.testing.assert_array_equal(dd, sd)
    for r in range(len(dd)):
        assert len(set(ii[r])) == len(ii[r]), (metric, r)
        got = MR.output_distance(metric, MR.ranking_values(metric, q[r:r + 1], y[ii[r]], V), q.dtype)[0]
        np.testing.assert_array_equal(got, dd[r], err_msg=f"{metric} row {r}")
        key_d, key_s = np.nan_to_num(dd[r], nan=np.inf), np.nan_to_num(sd[r], nan=np.inf)
        for v in np.unique(key_d[key_d < key_d[-1]]):
            assert set(ii[r][key_d == v]) == set(si[r][key_s == v]), (metric, r, v)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_against_scikit_learn(metric, dtype):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(17)
    for n_q, n_i, d, k in ((257, 1301, 33, 10), (64, 5000, 300, 50), (100, 700, 5, 7), (31, 300, 513, 3), (40, 2500, 20, 200)):
        q, y = _data(rng, n_q, d, dtype, metric), _data(rng, n_i, d, dtype, metric)
        V = _V(rng, d, metric)
        qm, im = N.DeviceMatrix(ctx, q, metric, V=V), N.DeviceMatrix(ctx, y, metric, V=V)
        dd, ii, st = N.knn(ctx, qm, im, k)
        sd, si = _sklearn(metric, y, q, k, V)
        _check(metric, dd.numpy(), ii.numpy(), sd, si, q, y, V)
        assert st["n_fallback_rows"] == n_q, st   # (the exact route: no MFMA tier, no range re-search, no speculative rows)


@pytest.mark.parametrize("metric", METRICS)
def test_self_query_with_duplicates(metric):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(5)
    y = _data(rng, 600, 24, np.float32, metric)
    y[17] = y[400]
    y[31] = y[32] = y[33]
    V = _V(rng, 24, metric)
    m = N.DeviceMatrix(ctx, y, metric, V=V)
    dd, ii, _ = N.knn(ctx, m, m, 6, exclude_self=True)
    rd, ri = MR.knn(metric, y, y, 6, V=V, exclude_self=True)
    _check(metric, dd.numpy(), ii.numpy(), rd, ri, y, y, V)
    assert not (ii.numpy() == np.arange(600)[:, None]).any()


def _runs_equal(rd, ri, d, i, rtol):
    """Indices equal except inside runs of (to rtol) equal reference distances; the run that reaches the k-th place may hold other
    rows of that distance than the reference's."""
    if np.array_equal(ri, i):
        return True
    rd, d = np.nan_to_num(rd, nan=np.inf), np.nan_to_num(d, nan=np.inf)
    for r in np.flatnonzero((ri != i).any(axis=1)):
        last = np.isclose(rd[r], rd[r][-1], rtol=rtol, atol=0) | (rd[r] == rd[r][-1])
        for p in np.flatnonzero((ri[r] != i[r]) & ~last):
            tied = np.isclose(rd[r], rd[r][p], rtol=rtol, atol=0)
            if set(ri[r][tied]) != set(i[r][tied]):
                return False
    return True


def _golden_cases():
    return sorted(p.stem for p in GOLDEN.glob("metrics_*.npz"))


@pytest.mark.parametrize("case", _golden_cases())
def test_kiez_pipeline_against_the_reference(case):
    from kiez_amd import Kiez
    z = np.load(GOLDEN / f"{case}.npz")
    g = {k: z[k] for k in z.files}
    metric, K = str(g["metric"]), int(g["K"])
    ks = [None if k < 0 else int(k) for k in g["ks"]]
    akw = {"metric": metric}
    if "V" in g:
        akw["metric_params"] = {"V": g["V"]}
    tree = str(g["algorithm"]) != "brute"    # (scikit-learn's ball tree: float64 values where the device rounds to float32)
    tags = sorted({k.split("__")[0] for k in g if "__" in k})
    assert len(tags) == 7
    if case == "metrics_correlation_constant_row":
        tags = ["none"]   # (the hubness kinds on NaN distances: INTEGRATION.md "Deviations")
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
            for k in ks:
                d, i = kz.kneighbors(k)
                kt = "None" if k is None else str(k)
                rd, ri = g[f"{tag}__k{kt}__dist"], g[f"{tag}__k{kt}__ind"]
                keep = np.ones(len(i), dtype=bool)
                if tag == "mp_empiric":
                    keep &= ~knife_edge_rows(g["mp_empiric__ind_s2t"])
                if metric == "hamming" and tag != "none":
                    # (hamming values are multiples of 1 / d: where a tie runs across the K-th candidate, scikit-learn's unstable
                    #  order and the device's smallest-row order keep different candidate sets -- both right; the rescaled scores of
                    #  such rows are not comparable)
                    #  CSLS / LocalScaling / MP normal read the candidates' distances only: the rows whose candidate set is the
                    #  reference's are compared.  MP empiric counts through the reverse LISTS, and with ties in nearly every one of
                    #  them no row is comparable: that kind is checked on hamming against one GPU in test_two_ranks_equal_one)
                    if tag == "mp_empiric":
                        assert d.shape == rd.shape and np.isfinite(d).all()
                        continue
                    _, ci = kz.algorithm.kneighbors(k=K)
                    same = np.array([set(a) == set(b) for a, b in zip(ci, g[f"{tag}__ind_s2t"])])
                    assert same.sum() >= 5, (case, tag, same.sum())
                    keep &= same
                rtol = 1e-5 if tree else 1e-12
                np.testing.assert_allclose(d[keep], rd[keep], rtol=rtol, atol=1e-6 if tree else 1e-15)
                assert _runs_equal(rd[keep], ri[keep], d[keep], i[keep], rtol), (case, tag, k)


TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import torch                       # first: its HIP runtime is the one the process uses
import numpy as np
from kiez_amd.neighbors import SklearnNN
from tests import test_gpu_metrics_extra as T
for metric in T.METRICS:
    rng = np.random.default_rng(8)
    y = T._data(rng, 900, 37, np.float32, metric)
    q = T._data(rng, 70, 37, np.float32, metric)
    V = T._V(rng, 37, metric)
    kw = {"metric_params": {"V": V}} if V is not None else {}
    nn = SklearnNN(n_candidates=9, metric=metric, **kw)
    nn.fit(torch.from_numpy(y).cuda())
    dt, it = nn.kneighbors(k=9, query=torch.from_numpy(q).cuda())
    assert isinstance(dt, torch.Tensor) and dt.is_cuda and dt.dtype == torch.float64 and it.dtype == torch.int64
    sd, si = T._sklearn(metric, y, q, 9, V)
    T._check(metric, dt.cpu().numpy(), it.cpu().numpy(), sd, si, q, y, V)
    nn2 = SklearnNN(n_candidates=9, metric=metric, **kw)
    nn2.fit(y)
    d2, i2 = nn2.kneighbors(k=9, query=q)        # (an ad-hoc numpy query: uploaded with the index's V)
    assert d2.dtype == np.float64
    T._check(metric, d2, i2, sd, si, q, y, V)
print("TORCH_OK")
"""


def test_torch_tensors_and_adhoc_query():
    """Torch device tensors in, tensors out (in a child process: torch must load its HIP runtime first)."""
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_correlation_constant_rows(dtype):
    from kiez_amd import _native as N
    ctx = N.Context.get()
    rng = np.random.default_rng(2)
    y = rng.standard_normal((500, 31)).astype(dtype)
    q = rng.standard_normal((40, 31)).astype(dtype)
    y[[3, 77, 300]] = np.array([0.5, -2.0, 0.0], dtype=dtype)[:, None]   # constant index rows: NaN, after every finite value
    q[[0, 9]] = 1.25                                                       # constant query rows: all NaN
    qm, im = N.DeviceMatrix(ctx, q, "correlation"), N.DeviceMatrix(ctx, y, "correlation")
    dd, ii, _ = N.knn(ctx, qm, im, 500)
    dd, ii = dd.numpy(), ii.numpy()
    sd, si = _sklearn("correlation", y, q, 500, None)
    live = np.ones(40, dtype=bool)
    live[[0, 9]] = False
    _check("correlation", dd[live], ii[live], sd[live], si[live], q[live], y, None)
    assert np.isnan(dd[live, -3:]).all() and np.isfinite(dd[live, :-3]).all()
    assert set(ii[live, -3:].ravel()) == {3, 77, 300}
    assert np.isnan(dd[~live]).all() and (np.sort(ii[~live], axis=1) == np.arange(500)).all()


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
src = rng.randn(1501, 21).astype(np.float32)
tgt = rng.randn(1203, 21).astype(np.float32)
src[10] = 0.5                                         # (correlation: a constant row on one shard)
V = rng.uniform(0.5, 2.0, 21)
b, c = row_slice(len(src), rank, world)
K, k = 8, 5
for metric in ("braycurtis", "seuclidean", "correlation", "hamming"):
    s_in, t_in = (np.round(src), np.round(tgt)) if metric == "hamming" else (src, tgt)
    akw = {"metric": metric, "metric_params": {"V": V}} if metric == "seuclidean" else {"metric": metric}
    for hub, kw in ((None, {}), ("CSLS", {}), ("MutualProximity", {"method": "empiric"}), ("LocalScaling", {"method": "nicdm"})):
        sk = ShardedKiez(n_candidates=K, algorithm_kwargs=akw, hubness=hub, hubness_kwargs=kw, engine=eng, comm=StagedComm())
        sk.fit(s_in[b:b + c], t_in if rank == 0 else None)
        d, i = sk.kneighbors(k)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        one = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs=akw, hubness=hub, hubness_kwargs=kw)
        one.fit(s_in, t_in)
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
