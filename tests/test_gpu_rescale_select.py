"""kz_rescale_select -- the fused rescale + `_sort` selection + output cast of kiez_amd/csrc/kz_hubness.hip -- on crafted candidate
lists, against the sequence it replaces run through `_native`: kz_csls / kz_local_scaling / kz_mp_normal -> kz_select_topk ->
kz_cast_f64_f32 (pinned to the reference by the goldens and by tests/test_gpu_hubness_kernels.py).  Equality is on BYTES: the fused
kernel evaluates the same device functions in the same order, so there is no tolerance, and a NaN must carry the same payload.

Rows 1 / 63 / 64 / 65 / 130: a partial, a full and several workgroups of 64 rows.  K 2 .. 128: the branches of numpy's pairwise tree
(< 8, a multiple of 8, a remainder, 128) up to the last fused size; K = 129: the sequence inside the call.  The values are
quantised to a handful of levels, so rows are full of ties and the swap history of the selection decides the order; one row ends in
NaN, the state holds sd = 0 (MP normal gives NaN) and radius 0 (LS gives NaN), and -0.0 appears among the distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
KS = (2, 7, 8, 9, 16, 17, 127, 128, 129)
N_T = 97


@pytest.fixture(scope="module")
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _bytes_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.count_nonzero(got.view(np.uint8) != want.view(np.uint8))} bytes differ"


def _case(n, K, seed):
    """(dist, ind, t_a, t_b): quantised distances (ties everywhere), -0.0 entries, a row ending in NaN; state vectors with a zero
    (radius 0 / sd = 0) that the ids reach."""
    rng = np.random.default_rng(seed)
    dist = np.sort(rng.integers(0, 6, size=(n, K)).astype(np.float64) * 0.25, axis=1)
    dist[dist == 0.0] = np.where(rng.random(np.count_nonzero(dist == 0.0)) < 0.5, -0.0, 0.0)
    if n > 2:
        dist[n // 2, K - 1] = np.nan              # a list that ends in NaN (correlation against a constant row)
    ind = np.stack([rng.choice(N_T, K, replace=False) if K <= N_T else rng.integers(0, N_T, K) for _ in range(n)]).astype(np.int64)
    ind[0, 0], ind[n - 1, K - 1] = 0, N_T - 1     # both ends of the gathered vectors
    t_a = rng.integers(1, 5, size=N_T).astype(np.float64) * 0.5
    t_b = rng.integers(1, 4, size=N_T).astype(np.float64) * 0.25
    t_a[3] = 0.0                                  # radius 0: LS divides by 0
    t_b[5] = 0.0                                  # sd = 0: MP normal divides by 0
    ind[0, 1 % K] = 3 if K > 1 else ind[0, 0]
    ind[n - 1, 0] = 5
    return np.ascontiguousarray(dist), np.ascontiguousarray(ind), t_a, t_b


def _sequence(N, ctx, kind, d, i, ta, tb, k, out_dtype):
    """The present tail: rescale kernel -> kz_select_topk -> kz_cast_f64_f32."""
    if kind == N.HUB_NONE:
        w = d
    elif kind == N.HUB_CSLS:
        w = N.csls(ctx, d, i, ta)
    elif kind in (N.HUB_LS, N.HUB_NICDM):
        w = N.local_scaling(ctx, d, i, ta, kind == N.HUB_NICDM)
    else:
        w = N.mp_normal(ctx, d, i, ta, tb)
    od, oi = N.select_topk(ctx, w, i, k)
    if out_dtype == np.float32:
        od = N.cast_f32(ctx, od)
    return od.numpy(), oi.numpy()


@pytest.mark.parametrize("K", KS)
def test_fused_tail_equals_the_kernel_sequence_on_bytes(ctx, K):
    from kiez_amd import _native as N
    assert N.RESCALE_SELECT_FUSED_MAX_K == 128
    saw_nan = False
    for n in ROWS:
        dist, ind, t_a, t_b = _case(n, K, 1000 * K + n)
        d, i, ta, tb = (ctx.to_device(a) for a in (dist, ind, t_a, t_b))
        for kind in (N.HUB_NONE, N.HUB_CSLS, N.HUB_LS, N.HUB_NICDM, N.HUB_MP_NORMAL):
            for k in sorted({1, max(K // 2, 1), K}):
                for out_dtype in (np.float64, np.float32):
                    want_d, want_i = _sequence(N, ctx, kind, d, i, ta, tb, k, out_dtype)
                    got_d, got_i = N.rescale_select(ctx, d, i, k, kind, ta if kind else None, tb if kind == N.HUB_MP_NORMAL else None, out_dtype)
                    what = f"n={n} K={K} k={k} kind={kind} {np.dtype(out_dtype).name}"
                    _bytes_equal(got_i.numpy(), want_i, what + " ids")
                    _bytes_equal(got_d.numpy(), want_d, what + " distances")
                    saw_nan |= bool(np.isnan(want_d).any())
    assert saw_nan, "the crafted lists were meant to produce NaN (radius 0, sd = 0, a row ending in NaN)"


def test_refusals_write_nothing(ctx):
    """k outside [1, K], a null state for a kind that reads it, an unknown kind: ValueError before anything is written."""
    from kiez_amd import _native as N
    dist, ind, t_a, t_b = _case(65, 9, 7)
    d, i, ta, tb = (ctx.to_device(a) for a in (dist, ind, t_a, t_b))
    made = []

    def alloc(shape, dtype):
        a = ctx.to_device(np.full(shape, 7, dtype=dtype))   # (a sentinel the call must leave in place)
        made.append(a)
        return a

    bad = [dict(k=0, kind=N.HUB_CSLS, t_a=ta), dict(k=10, kind=N.HUB_CSLS, t_a=ta), dict(k=-3, kind=N.HUB_NONE),
           dict(k=3, kind=N.HUB_CSLS), dict(k=3, kind=N.HUB_LS), dict(k=3, kind=N.HUB_NICDM), dict(k=3, kind=N.HUB_MP_NORMAL, t_a=ta),
           dict(k=3, kind=N.HUB_MP_NORMAL, t_b=tb), dict(k=3, kind=N.HUB_MP_EMPIRIC, t_a=ta, t_b=tb), dict(k=3, kind=6, t_a=ta, t_b=tb),
           dict(k=3, kind=-1, t_a=ta, t_b=tb), dict(k=3, kind=N.RANK_DUAL, t_a=ta, t_b=tb)]
    for kw in bad:
        with pytest.raises(ValueError, match="kz_rescale_select"):
            N.rescale_select(ctx, d, i, alloc=alloc, **kw)
    with pytest.raises(ValueError, match="out_dtype"):
        N.rescale_select(ctx, d, i, 3, N.HUB_NONE, out_dtype=np.float16, alloc=alloc)
    ctx.sync()
    assert len(made) == 2 * len(bad)
    for a in made:
        assert (a.numpy() == 7).all(), "a refused call wrote into its outputs"
    # ... and the same call with legal arguments does write
    od, oi = N.rescale_select(ctx, d, i, 3, N.HUB_CSLS, ta, alloc=alloc)
    assert not (od.numpy() == 7).all() and oi.shape == (65, 3)
