"""Embeddings of 497 to 1024 features (32 .. 64 slices of 16) on the fp16 first pass: the one-wave-per-SIMD builds of the fp16
kernel (kz_knn_h_inst.h "WIDE ROWS"), the shared sweep (kz_knn_dual) at those widths, the ladder below the new pass (speculative
rescue, float32 operands, exact kernels -- there is no split-bf16 tier beyond 24 slices), long k, and the drop-in API.  The fp16 pass
only decides how fast a row is answered: every result must equal the float32-operand run (precision = 1) bit for bit and the
oracle.  Reference path: kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101; both directions of a fit:
kiez/hubness_reduction/base.py:33-50."""
import os
import socket
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests.golden_util import HUB

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import fuzz_wide  # noqa: E402

TIER_F32, TIER_FP16 = 0, 2   # kz_knn_stats.first_pass


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("precision", 0), ("eps_scale", 1.0), ("spec_rows", 64), ("dual_force", 0), ("dual_stride", 1)):
        c.set_option(name, value)


def _gmm(rows, d, seed, spread=0.35):
    centres = np.random.RandomState(6).standard_normal((64, d)).astype(np.float32)
    rng = np.random.RandomState(seed)
    x = centres[rng.randint(0, 64, rows)] + np.float32(spread) * rng.standard_normal((rows, d)).astype(np.float32)
    return (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(np.float32)


def _both_precisions(ctx, q, y, k, metric, exclude_self=False):
    from kiez_amd import _native as N
    out = {}
    for prec in (1, 0):
        ctx.set_option("precision", prec)
        qm = N.DeviceMatrix(ctx, q, metric)
        ym = qm if y is q else N.DeviceMatrix(ctx, y, metric)
        dd, ii, st = N.knn(ctx, qm, ym, k, exclude_self=exclude_self)
        out[prec] = (dd.numpy(), ii.numpy(), st)
    ctx.set_option("precision", 0)
    return out


@pytest.mark.parametrize("d", [497, 512, 768, 1024])
def test_wide_rows_take_the_fp16_pass(ctx, d):
    from kiez_amd import _native as N
    rng = np.random.RandomState(d)
    q, y = rng.rand(300, d).astype(np.float32), rng.rand(1000, d).astype(np.float32)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    _, _, st = N.knn(ctx, qm, ym, 10)
    assert st["first_pass"] == TIER_FP16, st
    ctx.set_option("precision", 2)   # (no split-bf16 tier beyond 24 slices: float32 operands, as before)
    _, _, st2 = N.knn(ctx, qm, ym, 10)
    assert st2["first_pass"] == TIER_F32, st2


# (d, metric, dtype, k, single, n_q, n_i): every width, metric, dtype and k of the issue, ragged row counts
PARITY = [
    (497, "euclidean", np.float32, 10, False, 331, 1777),
    (512, "cosine", np.float64, 50, False, 260, 2049),
    (640, "sqeuclidean", np.float32, 1, True, 900, 900),
    (768, "euclidean", np.float64, 1, False, 129, 1501),
    (768, "cosine", np.float32, 10, True, 1100, 1100),
    (1000, "sqeuclidean", np.float64, 10, False, 250, 1300),
    (1000, "euclidean", np.float32, 50, True, 700, 700),
    (1024, "cosine", np.float32, 1, False, 200, 1999),
    (1024, "euclidean", np.float32, 10, False, 385, 2500),
    (497, "sqeuclidean", np.float64, 50, True, 600, 600),
]


@pytest.mark.parametrize("d,metric,dtype,k,single,n_q,n_i", PARITY)
def test_parity_with_float32_operands_and_the_oracle(ctx, d, metric, dtype, k, single, n_q, n_i):
    from oracle import kiez_oracle as O
    rng = np.random.RandomState(d + k)
    q = rng.standard_normal((n_q, d)).astype(dtype) if metric == "cosine" else rng.rand(n_q, d).astype(dtype)
    y = q if single else (rng.standard_normal((n_i, d)).astype(dtype) if metric == "cosine" else rng.rand(n_i, d).astype(dtype))
    res = _both_precisions(ctx, q, y, k, metric, exclude_self=single)
    assert res[0][2]["first_pass"] == TIER_FP16 and res[1][2]["first_pass"] == TIER_F32
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0], res[1][0])
    q64, y64 = (q.astype(np.float64), y.astype(np.float64)) if metric == "cosine" else (q, y)
    _, oi = O.knn_exact(q64, y64, k, metric, exclude_self=single)
    np.testing.assert_array_equal(res[0][1], oi)


def _uncertified(ctx, qm, ym, k, lo, hi):
    """An `eps_scale` at which the fp16 pass leaves between lo and hi rows uncertified (speculation off while looking): bisection,
    as in test_gpu_spec_rescue.py."""
    from kiez_amd import _native as N
    ctx.set_option("spec_rows", 0)
    scale, lo_s, hi_s = 1.0, None, None
    for _ in range(60):
        ctx.set_option("eps_scale", scale)
        _, _, st = N.knn(ctx, qm, ym, k)
        assert st["first_pass"] == TIER_FP16
        n = st["n_first_pass_fail"]
        if lo <= n <= hi:
            return scale, n
        if n < lo:
            lo_s = scale
            scale = scale * 2 if hi_s is None else 0.5 * (scale + hi_s)
        else:
            hi_s = scale
            scale = scale / 2 if lo_s is None else 0.5 * (scale + lo_s)
    raise AssertionError(f"no eps_scale leaves {lo} .. {hi} rows uncertified")


def test_a_handful_of_uncertified_rows_take_the_speculative_rescue(ctx):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(3000, 768, 1), _gmm(5000, 768, 2)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    scale, n_fail = _uncertified(ctx, qm, ym, 10, 1, 16)
    ctx.set_option("spec_rows", 64)
    d_on, i_on, st = N.knn(ctx, qm, ym, 10)
    assert st["n_first_pass_fail"] == n_fail and st["n_spec_rows"] == n_fail, st
    ctx.set_option("precision", 1)
    d_ref, i_ref, _ = N.knn(ctx, qm, ym, 10)
    np.testing.assert_array_equal(i_on.numpy(), i_ref.numpy())
    np.testing.assert_array_equal(d_on.numpy(), d_ref.numpy())
    np.testing.assert_array_equal(i_on.numpy(), O.knn_exact(q, y, 10, "euclidean")[1])


@pytest.mark.parametrize("scale", [30.0, 1e30])
def test_uncertified_rows_go_to_float32_operands_and_the_exact_kernels(ctx, scale):
    """Many rows uncertified (eps_scale 30), then every row (1e30: nothing approximate can certify anything): the rows go down
    the ladder -- longer lists on the same image, float32 operands, the exact kernels -- and the answer keeps its bits."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(1500, 768, 3), _gmm(4000, 768, 4)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    ctx.set_option("spec_rows", 0)
    ctx.set_option("eps_scale", scale)
    dd, ii, st = N.knn(ctx, qm, ym, 10)
    assert st["first_pass"] == TIER_FP16 and st["n_first_pass_fail"] > 0 and st["n_escalated_rows"] > 0, st
    if scale > 1e10:
        assert st["n_first_pass_fail"] == len(q) and st["n_fallback_rows"] > 0, st
    ctx.set_option("eps_scale", 1.0)
    ctx.set_option("precision", 1)
    d_ref, i_ref, _ = N.knn(ctx, qm, ym, 10)
    np.testing.assert_array_equal(ii.numpy(), i_ref.numpy())
    np.testing.assert_array_equal(dd.numpy(), d_ref.numpy())
    np.testing.assert_array_equal(ii.numpy(), O.knn_exact(q, y, 10, "euclidean")[1])


@pytest.mark.parametrize("k", [200, 540])
def test_long_k(ctx, k):
    from oracle import kiez_oracle as O
    rng = np.random.RandomState(k)
    q, y = rng.rand(300, 768).astype(np.float32), rng.rand(12500, 768).astype(np.float32)
    res = _both_precisions(ctx, q, y, k, "euclidean")
    assert res[0][2]["first_pass"] == TIER_FP16
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], O.knn_exact(q, y, k, "euclidean")[1])


def test_shared_sweep_forced_and_chosen(ctx):
    """A two-source CSLS fit at d = 768 through the shared sweep: forced on a small shape, and chosen by the cost model on one
    where it pays (40k x 40k); both equal two ordinary searches (dual_stride = 0) bit for bit."""
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    warnings.simplefilter("ignore")
    rng = np.random.RandomState(11)
    for n, force in ((3000, 1), (40000, 0)):
        s, t = rng.rand(n, 768).astype(np.float32), rng.rand(n + 77, 768).astype(np.float32)
        out = {}
        for stride in (1, 0):
            ctx.set_option("dual_force", force if stride else 0)
            ctx.set_option("dual_stride", stride)
            kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
            kz.fit(s, t)
            out[stride] = kz.kneighbors(5) + (kz.algorithm.last_stats["dual"],)
        assert out[1][2] == 1 and out[0][2] == 0, (n, out[1][2], out[0][2])
        np.testing.assert_array_equal(out[1][1], out[0][1])
        np.testing.assert_array_equal(out[1][0], out[0][0])
        if n <= 3000:
            od, oi = O.kiez_pipeline(s, t, 10, 5, "euclidean", 2, "CSLS", {})
            np.testing.assert_array_equal(out[1][1], oi)
            np.testing.assert_allclose(out[1][0], od, rtol=1e-5, atol=1e-6)
    ctx.set_option("dual_stride", 1)


@pytest.mark.parametrize("tag", ["csls", "mp_empiric", "mp_normal", "ls", "nicdm", "dsl"])
def test_kiez_pipeline_against_the_oracle(ctx, tag):
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    warnings.simplefilter("ignore")
    hub, kw = HUB[tag]
    rng = np.random.RandomState(5)
    s, t = rng.rand(1400, 768).astype(np.float32), rng.rand(1700, 768).astype(np.float32)
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub, hubness_kwargs=kw)
    kz.fit(s, t)
    dd, ii = kz.kneighbors(5)
    od, oi = O.kiez_pipeline(s, t, 10, 5, "euclidean", 2, hub, kw)
    np.testing.assert_array_equal(ii, oi)
    np.testing.assert_allclose(dd, od, rtol=1e-5, atol=1e-6)


def test_fuzz_slice(ctx):
    """A fixed-seed slice of tools/fuzz_wide.py: random shapes at 32 .. 64 slices, the shared sweep against two searches, both
    against the oracle."""
    bad, n_dual = fuzz_wide.run(seed=20261015, n_cases=6, max_rows=3000)
    assert not bad, bad
    assert n_dual >= 3, n_dual


SCRIPT = r"""
import sys, os, warnings
sys.path.insert(0, %r)
import numpy as np
import torch
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
from kiez_amd import Kiez
from kiez_amd.distributed import HipEngine, ShardedKiez, row_slice
from oracle import kiez_oracle as O
from tests.staged_comm import StagedComm
warnings.simplefilter("ignore")
eng = HipEngine(0)
rng = np.random.RandomState(9)
src = rng.rand(2301, 768).astype(np.float32)
tgt = rng.rand(2203, 768).astype(np.float32)
b, c = row_slice(len(src), rank, world)
K, k = 10, 5
for hub, kw in ((None, {}), ("CSLS", {}), ("MutualProximity", {"method": "empiric"}), ("LocalScaling", {"method": "nicdm"})):
    sk = ShardedKiez(n_candidates=K, algorithm_kwargs={"metric": "euclidean"}, hubness=hub, hubness_kwargs=kw, engine=eng, comm=StagedComm())
    sk.fit(src[b:b + c], tgt if rank == 0 else None)
    d, i = sk.kneighbors(k)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    one = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub, hubness_kwargs=kw)
    one.fit(src, tgt)
    od, oi = one.kneighbors(k)
    assert np.array_equal(d, od[b:b + c]), hub
    assert np.array_equal(i, oi[b:b + c]), hub
    if rank == 0:
        # CUDA torch inputs: same bits as the numpy inputs, the result on the device
        tk = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub, hubness_kwargs=kw)
        tk.fit(torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda"))
        td, ti = tk.kneighbors(k)
        assert isinstance(td, torch.Tensor) and td.device.type == "cuda", type(td)
        assert np.array_equal(td.cpu().numpy(), od) and np.array_equal(ti.cpu().numpy(), oi), hub
        xd, xi = O.kiez_pipeline(src, tgt, K, k, "euclidean", 2, hub, kw)
        assert np.array_equal(oi, xi), hub
        assert np.allclose(od, xd, rtol=1e-5, atol=1e-6), hub
    print(rank, hub, "ok", flush=True)
dist.barrier()
dist.destroy_process_group()
print("RANKS_OK", rank)
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_sharded_ranks_and_torch_inputs():
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
