"""Every entry of the sweep-kernel table (kiez_amd/csrc/kz_knn_kernels.h) is reached through the public calls and gives the exact
result: one case per (family, list length K', slice count) the library is built for, on a shape so small -- 300 query rows against
300 index rows, three index tiles -- that no short-list or long-k route replaces the list length.  `list_len` and `first_pass` of
the call's statistics say which entry ran: nothing may fall through to a lower tier, and a slice count without a build must run on
float32 operands.  Reference: the float64 brute force of tests/cpu_engine.py (sklearn's ArgKmin order, kiez/neighbors/exact/
sklearn_nearest_neighbors.py:96-101); indices must be equal, distances within the tolerance of tests/test_gpu_wide_dims.py.

The dual-pass entries run through kz_knn_dual, forced (`dual_force`) on 2100 x 1100 rows with every second tile in the sample
(`dual_stride` = 2): the shared sweep needs 1024 index rows and 8 K' sample rows, which 300 rows do not give.  Its main sweep keeps
lists of kz_pick_list_len(k) there (the short-list route of the shared sweep needs 128 tiles per range), so k = 5, 20, 40, 100 reach
the dual builds of K' = 16, 32, 64, 128 at every slice count.

Dual entries that cannot be reached through the public API at this shape: none.  (Non-dual families: none either.)"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIER_F32, TIER_BF, TIER_FP16 = 0, 1, 2   # kz_knn_stats.first_pass
KS = {5: 16, 20: 32, 40: 64, 100: 128}   # k -> K' (kz_pick_list_len)
NARROW = [16 * s for s in range(2, 25)]            # 2 .. 24 slices
WIDE = [512, 640, 768, 896, 1024]                  # 32 .. 64 slices (padded to a multiple of 8)
XWIDE = [1280, 1536, 1792, 2048]                   # 80 .. 128 slices (padded to a multiple of 16)
Q64 = [16 * s for s in range(4, 14)]               # 4 .. 13 slices: the 64-query kernel
NO_BUILD = [16 * s for s in range(25, 32)] + [2049, 2064]   # 25 .. 31 slices, and beyond 2048 features
N_ROWS = 300
DUAL_ROWS = (2100, 1100)


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("precision", 0), ("h_q64", 2), ("dual_force", 0), ("dual_stride", 1)):
        c.set_option(name, value)


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed):
    return np.random.RandomState(seed * 100003 + d).standard_normal((n, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(n_q, seed_q, n_i, seed_i, d, k):
    """(distances, indices) of the float64 brute force, computed once per case and shared."""
    from tests.cpu_engine import OracleEngine, _Mat
    qm, im = _Mat(torch.from_numpy(_rows(n_q, d, seed_q)), "euclidean"), _Mat(torch.from_numpy(_rows(n_i, d, seed_i)), "euclidean")
    dist, ind = OracleEngine().knn(qm, 0, n_q, im, k, False)
    return dist.numpy(), ind.numpy()


def _assert_exact(dist, ind, ref, what):
    np.testing.assert_array_equal(ind, ref[1], err_msg=what)
    np.testing.assert_allclose(dist, ref[0], rtol=1e-5, atol=1e-6, err_msg=what)


def _search(ctx, d, k, tier):
    from kiez_amd import _native as N
    qm, ym = N.DeviceMatrix(ctx, _rows(N_ROWS, d, 1), "euclidean"), N.DeviceMatrix(ctx, _rows(N_ROWS, d, 2), "euclidean")
    dist, ind, st = N.knn(ctx, qm, ym, k)
    what = f"d = {d}, k = {k}"
    assert st["list_len"] == KS[k] and st["first_pass"] == tier, (what, st)
    _assert_exact(dist.numpy(), ind.numpy(), _reference(N_ROWS, 1, N_ROWS, 2, d, k), what)


@pytest.mark.parametrize("k", sorted(KS))
@pytest.mark.parametrize("dims", [NARROW, WIDE, XWIDE], ids=["narrow", "wide", "parity-split"])
def test_fp16_entries(ctx, dims, k):
    for d in dims:
        _search(ctx, d, k, TIER_FP16)


@pytest.mark.parametrize("k", sorted(KS))
def test_split_bf16_entries(ctx, k):
    ctx.set_option("precision", 2)
    for d in NARROW:
        _search(ctx, d, k, TIER_BF)


@pytest.mark.parametrize("k", sorted(KS))
def test_float32_entries(ctx, k):
    ctx.set_option("precision", 1)
    _search(ctx, 200, k, TIER_F32)


def test_64_query_entries(ctx):
    ctx.set_option("h_q64", 1)
    for d in Q64:
        _search(ctx, d, 5, TIER_FP16)


@pytest.mark.parametrize("k", sorted(KS))
@pytest.mark.parametrize("precision", [0, 2])
def test_slice_counts_without_a_build_run_on_float32_operands(ctx, precision, k):
    ctx.set_option("precision", precision)
    for d in NO_BUILD:
        _search(ctx, d, k, TIER_F32)


def _shared_sweep(ctx, d, k):
    from kiez_amd import _native as N
    na, nb = DUAL_ROWS
    am, bm = N.DeviceMatrix(ctx, _rows(na, d, 1), "euclidean"), N.DeviceMatrix(ctx, _rows(nb, d, 2), "euclidean")
    (d_ab, i_ab, s_ab), (d_ba, i_ba, s_ba) = N.knn_dual(ctx, am, bm, k)
    what = f"shared sweep, d = {d}, k = {k}"
    assert s_ab["dual"] == 1 and s_ab["list_len"] == KS[k] and s_ab["first_pass"] == TIER_FP16, (what, s_ab)
    _assert_exact(d_ab.numpy(), i_ab.numpy(), _reference(na, 1, nb, 2, d, k), what + ", a -> b")
    _assert_exact(d_ba.numpy(), i_ba.numpy(), _reference(nb, 2, na, 1, d, k), what + ", b -> a")


@pytest.mark.parametrize("k", sorted(KS))
@pytest.mark.parametrize("dims", [NARROW, WIDE, XWIDE], ids=["narrow", "wide", "parity-split"])
def test_dual_entries(ctx, dims, k):
    ctx.set_option("dual_force", 1)
    ctx.set_option("dual_stride", 2)
    for d in dims:
        _shared_sweep(ctx, d, k)


def test_dual_64_query_entries(ctx):
    ctx.set_option("dual_force", 1)
    ctx.set_option("dual_stride", 2)
    ctx.set_option("h_q64", 1)
    for d in Q64:
        _shared_sweep(ctx, d, 5)
