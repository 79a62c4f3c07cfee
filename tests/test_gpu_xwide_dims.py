"""Embeddings of 1025 to 2048 features (65 .. 128 slices of 16) on the fp16 first pass: the parity-split builds of the fp16 kernel
(kz_knn_hx16.h: 64 queries per workgroup, two waves per query group, the K dimension split between them by slice parity, two
workgroups per work item), the shared sweep (kz_knn_dual) at those widths, the ladder below the pass (speculative rescue, longer
lists on the same image, float32 operands, exact kernels), long k and the drop-in API.  The fp16 pass only decides how fast a row
is answered: every result must equal the float32-operand run (precision = 1) bit for bit and the oracle.  Reference path:
kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101; both directions of a fit: kiez/hubness_reduction/base.py:33-50.
Modelled on tests/test_gpu_wide_dims.py (d = 497 .. 1024), whose helpers it uses."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.golden_util import HUB
from tests.test_gpu_wide_dims import ROOT, SCRIPT, TIER_F32, TIER_FP16, _both_precisions, _free_port, _gmm, _uncertified, fuzz_wide

pytestmark = pytest.mark.gpu
D = 1536   # 96 slices: the width of the tests that are not about the width


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("precision", 0), ("eps_scale", 1.0), ("spec_rows", 64), ("dual_force", 0), ("dual_stride", 1)):
        c.set_option(name, value)


def _three_way(ctx, q, y, k, metric, single=False):
    """fp16 pass against float32 operands bit for bit, both on the route they should take, indices against the oracle."""
    from oracle import kiez_oracle as O
    res = _both_precisions(ctx, q, y, k, metric, exclude_self=single)
    assert res[0][2]["first_pass"] == TIER_FP16 and res[1][2]["first_pass"] == TIER_F32, (res[0][2], res[1][2])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][0], res[1][0])
    q64, y64 = (q.astype(np.float64), y.astype(np.float64)) if metric == "cosine" else (q, y)
    np.testing.assert_array_equal(res[0][1], O.knn_exact(q64, y64, k, metric, exclude_self=single)[1])
    return res


@pytest.mark.parametrize("d", [1025, 1280, 1281, 1536, 1792, 2048])
def test_xwide_rows_take_the_fp16_pass(ctx, d):
    from kiez_amd import _native as N
    rng = np.random.RandomState(d)
    q, y = rng.rand(300, d).astype(np.float32), rng.rand(1000, d).astype(np.float32)
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    _, _, st = N.knn(ctx, qm, ym, 10)
    assert st["first_pass"] == TIER_FP16, st
    ctx.set_option("precision", 2)   # (no split-bf16 tier beyond 24 slices: float32 operands)
    _, _, st2 = N.knn(ctx, qm, ym, 10)
    assert st2["first_pass"] == TIER_F32, st2


def test_beyond_2048_stays_on_float32_operands(ctx):
    from kiez_amd import _native as N
    rng = np.random.RandomState(2049)
    q, y = rng.rand(300, 2049).astype(np.float32), rng.rand(1000, 2049).astype(np.float32)
    _, _, st = N.knn(ctx, N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean"), 10)
    assert st["first_pass"] == TIER_F32, st


# (d, metric, dtype, k, single, n_q, n_i): every metric, dtype and k, ragged row counts, each padded slice count (80 / 96 / 112 / 128)
# at its first and last width
PARITY = [
    (1025, "euclidean", np.float32, 10, False, 331, 1777),
    (1280, "cosine", np.float64, 50, False, 260, 2049),
    (1281, "sqeuclidean", np.float32, 1, True, 900, 900),
    (1536, "euclidean", np.float64, 1, False, 129, 1501),
    (1536, "cosine", np.float32, 10, True, 1100, 1100),
    (1537, "sqeuclidean", np.float64, 10, False, 250, 1300),
    (1792, "euclidean", np.float32, 50, True, 700, 700),
    (1793, "cosine", np.float32, 1, False, 200, 1999),
    (2048, "euclidean", np.float32, 10, False, 385, 2500),
    (2048, "sqeuclidean", np.float64, 50, True, 600, 600),
]


@pytest.mark.parametrize("d,metric,dtype,k,single,n_q,n_i", PARITY)
def test_parity_with_float32_operands_and_the_oracle(ctx, d, metric, dtype, k, single, n_q, n_i):
    rng = np.random.RandomState(d + k)
    q = rng.standard_normal((n_q, d)).astype(dtype) if metric == "cosine" else rng.rand(n_q, d).astype(dtype)
    y = q if single else (rng.standard_normal((n_i, d)).astype(dtype) if metric == "cosine" else rng.rand(n_i, d).astype(dtype))
    _three_way(ctx, q, y, k, metric, single)


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 127, 128, 129, 200])
def test_query_counts_around_the_64_query_workgroup(ctx, n_q):
    rng = np.random.RandomState(n_q)
    _three_way(ctx, rng.rand(n_q, D).astype(np.float32), rng.rand(2000, D).astype(np.float32), 10, "euclidean")


def test_a_handful_of_uncertified_rows_take_the_speculative_rescue(ctx):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(3000, D, 1), _gmm(5000, D, 2)
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
    """Many rows uncertified (eps_scale 30), then every row (1e30): the rows go down the ladder -- longer lists on the same image,
    float32 operands, the exact kernels -- and the answer keeps its bits."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    q, y = _gmm(1500, D, 3), _gmm(4000, D, 4)
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
    rng = np.random.RandomState(k)
    _three_way(ctx, rng.rand(300, D).astype(np.float32), rng.rand(12500, D).astype(np.float32), k, "euclidean")


def test_shared_sweep_forced_and_chosen(ctx):
    """A two-source CSLS fit at d = 1536 through the shared sweep: forced on a small shape, and chosen by the cost model on one
    where it pays (30k x 30k); both equal two ordinary searches (dual_stride = 0) bit for bit."""
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    warnings.simplefilter("ignore")
    rng = np.random.RandomState(11)
    for n, force in ((3000, 1), (30000, 0)):
        s, t = rng.rand(n, D).astype(np.float32), rng.rand(n + 77, D).astype(np.float32)
        out = {}
        for stride in (1, 0):
            ctx.set_option("dual_force", force if stride else 0)
            ctx.set_option("dual_stride", stride)
            kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS")
            kz.fit(s, t)
            out[stride] = kz.kneighbors(5) + (kz.algorithm.last_stats["dual"], kz.algorithm.last_stats["first_pass"])
        assert out[1][2] == 1 and out[0][2] == 0, (n, out[1][2], out[0][2])
        assert out[0][3] == TIER_FP16, (n, out[0][3])
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
    s, t = rng.rand(1400, D).astype(np.float32), rng.rand(1700, D).astype(np.float32)
    kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub, hubness_kwargs=kw)
    kz.fit(s, t)
    dd, ii = kz.kneighbors(5)
    assert kz.algorithm.last_stats["first_pass"] == TIER_FP16, kz.algorithm.last_stats
    od, oi = O.kiez_pipeline(s, t, 10, 5, "euclidean", 2, hub, kw)
    np.testing.assert_array_equal(ii, oi)
    np.testing.assert_allclose(dd, od, rtol=1e-5, atol=1e-6)


FUZZ_SEED = 20261016


def test_fuzz_slice(ctx):
    """A fixed-seed slice of tools/fuzz_wide.py at 65 .. 128 slices, k <= 50: no bad case (a case off the fp16 pass is a bad one),
    and at least half of the cases through the shared sweep -- the share tests/test_gpu_wide_dims.py asks of its slice.  (The
    sweep may decline a forced case for reasons other than the width: too few sample rows for the list length.)"""
    bad, n_dual = fuzz_wide.run(seed=FUZZ_SEED, n_cases=6, max_rows=3000, d_lo=1025, d_hi=2048, k_max=50)
    assert not bad, bad
    assert n_dual >= 3, n_dual


def test_two_sharded_ranks_and_torch_inputs():
    """The two-rank script of tests/test_gpu_wide_dims.py at d = 1536."""
    script = SCRIPT.replace(", 768)", f", {D})")
    assert script.count(f", {D})") == 2
    world, port = 2, _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen([sys.executable, "-c", script % str(ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
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
