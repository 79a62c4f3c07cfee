"""The two buffer kinds of `kiez_amd._native`: every wrapper that `distributed.HipEngine` shares with the single-GPU classes is called
twice on the same bytes -- once with torch CUDA tensors and the engine's allocator, once with `DeviceArray` copies and the default
allocator -- and must return the buffer kind of its allocator, with equal dtype, shape and BYTES (one library, one kernel, one stream:
there is nothing to tolerate).  One small shape (source 67 x 8, target 53 x 8, float32, K = 7; row counts that are no multiple of 64):
the kernels are tested elsewhere, this tests the binding.  `kz_comm_*`: tests/test_gpu_kz_comm.py.

A child process, because torch must be imported before the library is loaded.  `pytest -m gpu`."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

SCRIPT = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["KIEZ_AMD_WITH_TORCH"] = "1"
import numpy as np
import torch
from kiez_amd import _native as N
from kiez_amd.distributed import HipEngine

eng = HipEngine(0)
ctx = eng.ctx
rng = np.random.RandomState(31)
n_s, n_t, K = 67, 53, 7
S = eng.matrix(eng.to_engine(rng.rand(n_s, 8).astype(np.float32)), "euclidean")
T = eng.matrix(eng.to_engine(rng.rand(n_t, 8).astype(np.float32)), "euclidean")
fd, fi = eng.knn(S, 0, n_s, T, K, False)      # forward lists [67, 7]
rd, ri = eng.knn(T, 0, n_t, S, K, False)      # reverse lists [53, 7]
assert isinstance(fd, torch.Tensor) and fd.is_cuda and fd.dtype == torch.float64 and tuple(fi.shape) == (n_s, K)
n_checked = 0


def dev(t):
    # a DeviceArray copy of a tensor's bytes (None stays None)
    return None if t is None else ctx.to_device(t.cpu().numpy())


def same(what, got_t, got_d):
    # tensor-side result against DeviceArray-side result: buffer kinds, dtype, shape, bytes
    global n_checked
    got_t = got_t if isinstance(got_t, tuple) else (got_t,)
    got_d = got_d if isinstance(got_d, tuple) else (got_d,)
    assert len(got_t) == len(got_d), what
    for j, (a, b) in enumerate(zip(got_t, got_d)):
        if a is None or b is None:
            assert a is None and b is None, (what, j)
            continue
        assert isinstance(a, torch.Tensor) and a.is_cuda, (what, j, type(a))
        assert isinstance(b, N.DeviceArray), (what, j, type(b))
        ha, hb = a.cpu().numpy(), b.numpy()
        assert ha.dtype == hb.dtype and ha.shape == hb.shape, (what, j, ha.dtype, hb.dtype, ha.shape, hb.shape)
        assert ha.tobytes() == hb.tobytes(), (what, j, "bytes differ")
        n_checked += 1


def both(fn, *args, **kw):
    # fn on tensors with the engine's allocator, and on DeviceArray copies with the default one
    got_t = fn(ctx, *args, alloc=eng.empty, **kw)
    got_d = fn(ctx, *[dev(a) if isinstance(a, torch.Tensor) else a for a in args], **kw)
    same(fn.__name__, got_t, got_d)
    return got_t


(d1, i1, st1), (d2, i2, st2) = N.knn(ctx, S, T, K, False, 0, n_s, alloc=eng.empty), N.knn(ctx, S, T, K)
same("knn", (d1, i1), (d2, i2))
assert torch.equal(d1, fd) and torch.equal(i1, fi) and st1["list_len"] == st2["list_len"]
(ab_t, ba_t), (ab_d, ba_d) = N.knn_dual(ctx, S, T, K, alloc=eng.empty), N.knn_dual(ctx, S, T, K)
same("knn_dual", ab_t[:2] + ba_t[:2], ab_d[:2] + ba_d[:2])
assert isinstance(ab_t[2], dict) and ab_t[2].keys() == ba_d[2].keys()

both(N.row_stats, fd, mean=True)                                   # (the outputs not asked for: None on both sides)
r_mean, _, r_last = both(N.row_stats, rd, mean=True, std=True, last=True)
mu, sd = both(N.row_nanstats, rd)
both(N.select_topk, fd, fi, 5)
w = both(N.csls, fd, fi, r_mean)
both(N.local_scaling, fd, fi, r_last, False)
both(N.local_scaling, fd, fi, r_mean, True)
both(N.mp_normal, fd, fi, mu, sd)
both(N.mp_empiric, fd, fi, rd, ri)
t2c = both(N.dsl_fit, ri, S, T, 0)
assert tuple(t2c.shape) == (n_t,)
gmin_t = torch.full((1,), float("inf"), dtype=torch.float64, device=eng.device)
gmin_d = ctx.to_device(np.array([np.inf]))
out_t = N.dsl_transform(ctx, fi, S, 0, T, t2c, gmin_t, alloc=eng.empty)
out_d = N.dsl_transform(ctx, dev(fi), S, 0, T, dev(t2c), gmin_d)
same("dsl_transform", (out_t, gmin_t), (out_d, gmin_d))
mn = float(gmin_t.cpu()[0])
assert np.isfinite(mn)
fin_t, fin_d = N.dsl_finalize(ctx, out_t, mn, False), N.dsl_finalize(ctx, out_d, mn, False)
assert fin_t is out_t and fin_d is out_d                           # (in place)
same("dsl_finalize", fin_t, fin_d)
both(N.pair_values, S, 0, n_s, T, fi)
# two segments per row, each ascending by (key, id): the forward lists and a shifted copy with other ids
key = torch.cat([fd, fd + 0.25], dim=1).contiguous()
ids = torch.cat([fi, fi + 1000], dim=1).contiguous()
both(N.merge_topk, key, ids, None, 2, K, K)
both(N.merge_topk, key, ids, (key * 3.0).contiguous(), 2, K, K)
both(N.merge_topk, key, None, None, 2, K, K)

lo_hi = N.minmax_i64_2d(ctx, fi, 5)
assert lo_hi == N.minmax_i64_2d(ctx, dev(fi), 5) and 0 <= lo_hi[0] <= lo_hi[1] < n_t
n_bins = max(n_s, lo_hi[1] + 1)
kocc = both(N.k_occurrence, fi, 5, n_bins)
assert int(kocc.sum()) == 5 * n_s
st_t, st_d = N.kocc_stats(ctx, kocc, 10.0, True), N.kocc_stats(ctx, dev(kocc), 10.0, True)
assert len(st_t) == 10 and np.array(st_t).tobytes() == np.array(st_d).tobytes() and st_t[0] == 5 * n_s
for mode in (0, 1):
    (sel_t, cnt_t), (sel_d, cnt_d) = N.kocc_select(ctx, kocc, mode, 2.0, alloc=eng.empty), N.kocc_select(ctx, dev(kocc), mode, 2.0)
    assert cnt_t == cnt_d and 0 < cnt_t < n_bins, (mode, cnt_t, cnt_d)
    assert isinstance(sel_t, torch.Tensor) and isinstance(sel_d, N.DeviceArray) and tuple(sel_t.shape) == sel_d.shape == (n_bins,)
    # (the library defines the first `count` entries only)
    assert sel_t.cpu().numpy()[:cnt_t].tobytes() == sel_d.numpy()[:cnt_d].tobytes(), mode
gold = fi[torch.arange(n_s), torch.arange(n_s) %% K].clone()
gold[::5] = torch.iinfo(torch.int64).min                          # no gold id: the row is not counted
gold[1::5] = 10 ** 6                                               # a gold id outside the list: counted in the last entry
hist = both(N.hit_positions, fi, gold.contiguous())
assert int(hist.sum()) == n_s - len(range(0, n_s, 5)) and int(hist[K]) == len(range(1, n_s, 5))

# mixed: DeviceArray inputs, the tensor allocator
mixed = N.csls(ctx, dev(fd), dev(fi), dev(r_mean), alloc=eng.empty)
assert isinstance(mixed, torch.Tensor) and mixed.is_cuda and torch.equal(mixed, w)
# a buffer that is no contiguous device buffer never reaches the library
calls = []
real_call = N._call
N._call = lambda owner, name, *a: (calls.append(name), real_call(owner, name, *a))[1]
try:
    for bad, named in (((fd[:, ::2], fi[:, ::2].contiguous(), r_mean), "dist"), ((fd, fi, r_mean.cpu()), "r_train"), ((fd, fi.cpu(), r_mean), "ind")):
        try:
            N.csls(ctx, *bad, alloc=eng.empty)
        except TypeError as e:
            assert str(e) == named + " must be a DeviceArray or a contiguous CUDA tensor", e
        else:
            raise AssertionError("no TypeError for a bad " + named)
    assert calls == [], calls
    N.csls(ctx, fd, fi, r_mean, alloc=eng.empty)
    assert calls == ["kz_csls"], calls                               # (the probe sees the calls it is there to see)
finally:
    N._call = real_call
eng.sync()
assert n_checked >= 30, n_checked
print("NATIVE_BUFFERS_OK", n_checked)
"""


def test_every_shared_wrapper_gives_the_same_bytes_for_tensors_and_device_arrays():
    r = subprocess.run([sys.executable, "-c", SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "NATIVE_BUFFERS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
