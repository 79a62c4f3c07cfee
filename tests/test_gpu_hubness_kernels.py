"""The rescaling and sort kernels of kiez_amd/csrc/kz_hubness.hip through the C ABI, each on the same float64 / int64 arrays as
its reference: every comparison covers the whole output, no row or element is set aside.

Bit for bit (the kernels use +, -, x, / and sqrt only, all correctly rounded in float64, and the unit is built with
-ffp-contract=off): kz_row_stats, kz_row_nanstats, kz_csls, kz_local_scaling(nicdm = 1), kz_dsl_finalize, kz_cast_f64_f32,
kz_split_self, kz_select_topk (narrow kernel at every K around the 64 KiB LDS line), kz_mp_empiric (wide kernel at every launch
branch), the minimum kz_dsl_transform reports.

Against a high-precision reference with a derived bound: kz_local_scaling(nicdm = 0) and kz_mp_normal (mpmath, 40 digits; exp /
erf / erfc differ between device and host in their last bits), kz_dsl_fit and kz_dsl_transform (fractions.Fraction; the bound
follows the kernel's operation count, tests/hubness_restate.py).

U_EXP = 3 and U_ERF = 16 are the ulp bounds taken for the device library's float64 exp and erf / erfc: the ROCm tree carries no
accuracy table for its device library's math functions (its share/doc holds licences and the runtime API reference only), so these are the
OpenCL full-profile figures (OpenCL C specification, "Relative error as ULPs": exp <= 3 ulp, erf / erfc <= 16 ulp), which the
device library is built to.  They are not fitted to what the kernels return.

Row counts are no multiples of the 256-row block, the four-wave workgroup or the 64-row select tile."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

from tests import hubness_restate as R

pytestmark = pytest.mark.gpu

U_EXP = 3
U_ERF = 16
LS_BOUND = (U_EXP + 2) * 2.0 ** -53          # exp <= 1: one ulp of it <= 2^-53; the subtraction's and the reference's rounding
MP_BOUND = (2 * U_ERF + 6) * 2.0 ** -53      # p1, p2 in [0, 1]: the product's error <= the sum of the two

N_ROWS = (1, 5, 63, 65, 257)
K_STATS = [1, 2, 7, 8, 9, 16, 17, 127, 128, 129, 136, 137, 255, 256, 257, 272, 273, 1000, 1024, 1025, 4095, 4096]
K_RESCALE = [1, 5, 8, 50, 128, 129, 300, 1025, 4096]


@pytest.fixture(scope="module")
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def assert_bits(got, want, what=""):
    """NaN at the same positions, identical bit patterns everywhere else (so +0 and -0 differ)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got, want, err_msg=what)                # (NaN == NaN here)
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        nan = np.isnan(want)
        np.testing.assert_array_equal(got.view(u)[~nan], want.view(u)[~nan], err_msg=what + " (bit patterns)")


def _dev(ctx, *arrays):
    """Uploaded copies, to be HELD by the caller until the result is read back: a device array is freed with its Python object,
    and the pointer taken from a temporary names memory the next upload may reuse."""
    return [ctx.to_device(a) for a in arrays]


def _rows(rng, n, K):
    """n rows of K positive doubles, the rows cycling through the scales 1e-3 / 1 / 1e3."""
    scale = np.array([1e-3, 1.0, 1e3])[np.arange(n) % 3][:, None]
    return np.ascontiguousarray(rng.random((n, K)) * scale)


def _distinct_ids(rng, n, K, n_t):
    """n rows of K distinct ids below n_t (what a kNN search returns) that reach both ends of the gathered array."""
    ind = np.stack([rng.choice(n_t, K, replace=False) for _ in range(n)]).astype(np.int64)
    if 0 not in ind[0]:
        ind[0, 0] = 0
    if n_t - 1 not in ind[n - 1] and n * K >= 2:
        ind[n - 1, K - 1] = n_t - 1
    return ind


def _ids(rng, n, K, n_t):
    """Random ids in [0, n_t) that reach both ends of the gathered array."""
    ind = rng.integers(0, n_t, size=(n, K)).astype(np.int64)
    ind[0, 0] = 0
    if n * K >= 2:
        ind[n - 1, K - 1] = n_t - 1
    return ind


# ---- kz_row_stats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_STATS)
def test_row_stats_bit_for_bit(ctx, K):
    """ndarray.mean / np.nanstd / column K - 1 for every branch of numpy's summation tree and every combination of outputs."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(K)
    a = _rows(rng, max(N_ROWS), K)
    for n in N_ROWS:
        d = ctx.to_device(a[:n])
        want = {"mean": a[:n].mean(axis=1), "std": np.nanstd(a[:n], axis=1), "last": a[:n, K - 1].copy()}
        combos = [(m, s, l_) for m in (0, 1) for s in (0, 1) for l_ in (0, 1)] if n in (5, 257) else [(1, 1, 1)]
        for m, s, l_ in combos:
            got = N.row_stats(ctx, d, mean=bool(m), std=bool(s), last=bool(l_))
            for g, on, name in zip(got, (m, s, l_), ("mean", "std", "last")):
                assert (g is not None) == bool(on)
                if on:
                    assert_bits(g.numpy(), want[name], f"{name} K={K} n={n} outputs={m}{s}{l_}")
        gm, gs = N.row_nanstats(ctx, d)
        assert_bits(gm.numpy(), np.nanmean(a[:n], axis=1), f"nanmean K={K} n={n}")
        assert_bits(gs.numpy(), want["std"], f"nanstd K={K} n={n}")
    # the host restatement of the tree, which test_hubness_restate.py pins to numpy, on the same rows
    assert_bits(R.rows(R.mean, a[:5]), a[:5].mean(axis=1))
    assert_bits(R.rows(R.nanstd, a[:5]), np.nanstd(a[:5], axis=1))


# ---- kz_csls, kz_local_scaling(nicdm) ---------------------------------------------------------------------------------------
def _rescale_case(rng, kind, n, K, n_t):
    if kind == "offset":                                   # distances around 1e3 with spread 1e-3: the mean swallows the low bits
        dist = 1e3 + 1e-3 * rng.standard_normal((n, K))
    else:
        dist = _rows(rng, n, K)
    r = rng.random(n_t) * np.array([1e-3, 1.0, 1e3])[np.arange(n_t) % 3] + 1e-9      # arbitrary positive doubles
    ind = _ids(rng, n, K, n_t)
    if kind == "zero":                                     # a zero radius (division by 0: inf) and a zero list on it (0 / 0: NaN)
        r[0] = 0.0
        r[n_t // 2] = 0.0
        dist[n // 2] = 0.0
        ind[n // 2, 0] = n_t // 2
    return np.ascontiguousarray(dist), r, ind


def _csls(ctx, dist, ind, r):
    from kiez_amd import _native as N
    out = ctx.empty(dist.shape, np.float64)
    d, i, rt = _dev(ctx, dist, ind, r)
    N._check(ctx.lib.kz_csls(ctx.handle, d.ptr, i.ptr, dist.shape[0], dist.shape[1], rt.ptr, out.ptr), "kz_csls")
    return out.numpy()


def _ls(ctx, dist, ind, r, nicdm):
    from kiez_amd import _native as N
    out = ctx.empty(dist.shape, np.float64)
    d, i, rt = _dev(ctx, dist, ind, r)
    N._check(ctx.lib.kz_local_scaling(ctx.handle, d.ptr, i.ptr, dist.shape[0], dist.shape[1], rt.ptr, int(nicdm), out.ptr),
             "kz_local_scaling")
    return out.numpy()


@pytest.mark.parametrize("K", K_RESCALE)
def test_csls_and_nicdm_bit_for_bit(ctx, K):
    rng = np.random.default_rng(100 + K)
    n_t = 37
    for kind in ("unit", "offset", "zero"):
        for n in (N_ROWS if kind == "unit" else (65,)):
            dist, r, ind = _rescale_case(rng, kind, n, K, n_t)
            assert ind.min() == 0 and (n * K < 2 or ind.max() == n_t - 1)
            want = 2 * dist - dist.mean(axis=1)[:, None] - r[ind]                           # csls.py:90-93
            assert_bits(_csls(ctx, dist, ind, r), want, f"csls {kind} K={K} n={n}")
            with np.errstate(divide="ignore", invalid="ignore"):
                want = dist / np.sqrt(dist.mean(axis=1)[:, None] * r[ind])                  # local_scaling.py:143-147
            if kind == "zero":
                assert np.isinf(want).any() and np.isnan(want[n // 2, 0])
            assert_bits(_ls(ctx, dist, ind, r, 1), want, f"nicdm {kind} K={K} n={n}")


# ---- kz_dsl_finalize, kz_cast_f64_f32, kz_split_self ------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 257])
def test_dsl_finalize_bit_for_bit(ctx, count):
    from kiez_amd import _native as N
    rng = np.random.default_rng(count)
    for min_value in (-0.75, 0.0, 0.5):
        for squared in (0, 1):
            out = rng.random(count) * 3.0 + min_value
            out[0] = min_value                                       # the minimum itself: 0 after the shift
            shift = -min_value if min_value < 0 else 0.0             # dis_sim.py:171-173
            want = out + shift if squared else np.sqrt(out + shift)
            assert want[0] == (0.0 if min_value <= 0 else min_value if squared else np.sqrt(min_value))
            d = ctx.to_device(out)
            N._check(ctx.lib.kz_dsl_finalize(ctx.handle, d.ptr, count, float(min_value), squared), "kz_dsl_finalize")
            assert_bits(d.numpy(), want, f"finalize count={count} min={min_value} squared={squared}")
    # a minimum of 0 or above shifts nothing: what lies below 0 becomes NaN under the root, as numpy has it
    out = np.linspace(-1.0, 1.0, count)
    d = ctx.to_device(out)
    N._check(ctx.lib.kz_dsl_finalize(ctx.handle, d.ptr, count, 0.0, 0), "kz_dsl_finalize")
    with np.errstate(invalid="ignore"):
        assert_bits(d.numpy(), np.sqrt(out + 0.0))


def test_cast_f64_f32_is_astype(ctx):
    from kiez_amd import _native as N
    rng = np.random.default_rng(5)
    one = np.float32(1.0)
    eps = float(np.spacing(one))                                                   # 2^-23
    f32max = float(np.finfo(np.float32).max)
    tiny = float(np.finfo(np.float32).tiny)                                        # 2^-126
    sub = float(np.finfo(np.float32).smallest_subnormal)                           # 2^-149
    special = [0.0, -0.0, np.nan, np.inf, -np.inf,
               1.0 + eps / 2, 1.0 + 3 * eps / 2, -(1.0 + eps / 2), 1.0 + eps / 2 + 2.0 ** -52, 1.0 + eps / 2 - 2.0 ** -53,   # half-way: to even
               f32max, f32max * (1 + 2.0 ** -25), f32max + 2.0 ** 102, f32max + 2.0 ** 103, -f32max - 2.0 ** 103, 1e39, -1e300,     # overflow
               tiny, tiny / 2, tiny * (1 - 2.0 ** -24), sub, sub / 2, sub * 0.5000001, sub * 1.5, sub * 2.5, -sub * 1.5, sub / 4, 1e-310]
    a = np.concatenate([np.array(special), rng.standard_normal(257) * 10.0 ** rng.integers(-50, 50, 257), rng.random(64)])
    with np.errstate(over="ignore", under="ignore"):
        want = a.astype(np.float32)
    assert np.isinf(want[12:17]).sum() >= 3 and want[5] == one and want[6] == np.float32(1.0 + 2 * eps) and want[21] == 0.0
    for count in (1, 255, len(a)):
        (d_a,) = _dev(ctx, a[:count])
        got = N.cast_f32(ctx, d_a).numpy()
        assert_bits(got, want[:count], f"cast count={count}")
    assert np.signbit(got[1]) and not np.signbit(got[0])


def _split_self_restated(dist, ind, row0):
    """The row minus the entry whose id is the row itself (its first occurrence), or minus the first entry when it is absent."""
    n, K1 = dist.shape
    fd, fi = np.empty((n, K1 - 1)), np.empty((n, K1 - 1), dtype=np.int64)
    for r in range(n):
        hit = np.flatnonzero(ind[r] == row0 + r)
        s = int(hit[0]) if len(hit) else 0
        fd[r], fi[r] = np.delete(dist[r], s), np.delete(ind[r], s)
    return (dist[:, :K1 - 1].copy(), ind[:, :K1 - 1].copy()), (fd, fi)


@pytest.mark.parametrize("K1", [2, 11, 129])
@pytest.mark.parametrize("row0", [0, 1000])
def test_split_self_is_its_restatement(ctx, K1, row0):
    from kiez_amd import _native as N
    rng = np.random.default_rng(K1 + row0)
    for n in N_ROWS:
        dist = np.sort(rng.random((n, K1)), axis=1)
        ind = np.stack([rng.choice(5000, K1, replace=False) + 10000 for _ in range(n)]).astype(np.int64)    # never a row's own id
        for r in range(n):
            if r % 3 == 0:                       # self at rank 0
                dist[r, 0] = 0.0
                ind[r, 0] = row0 + r
            elif r % 3 == 1:                     # self at a later rank, behind exact duplicates of it
                s = min(K1 - 1, 1 + r % 4)
                dist[r, :s + 1] = 0.0
                ind[r, s] = row0 + r
            # else: self absent, the first entry is dropped
            if row0 and r % 5 == 4:
                ind[r, K1 - 1] = r               # the LOCAL row number is not the row's id when row0 != 0
        d_dist, d_ind = _dev(ctx, dist, ind)
        (rd, ri), (fd, fi) = N.split_self(ctx, d_dist, d_ind, row0)
        (wrd, wri), (wfd, wfi) = _split_self_restated(dist, ind, row0)
        for got, want, name in ((rd, wrd, "reverse distances"), (ri, wri, "reverse ids"), (fd, wfd, "forward distances"), (fi, wfi, "forward ids")):
            assert_bits(got.numpy(), want, f"{name} K1={K1} n={n} row0={row0}")
        assert (wfi[0::3] != (row0 + np.arange(n)[0::3])[:, None]).all()       # (the restatement did strip the rows that hold themselves)


# ---- kz_select_topk, the narrow kernel --------------------------------------------------------------------------------------
def _select_reference(dist, ind, k):
    """HubnessReduction._sort (base.py:81-86): np.argpartition(kth = arange(k)) for k >= 2 (NaN last); for k = 1 the first minimum
    (numpy's SIMD arg-select differs there; the scalar rule is what the kernel implements)."""
    n = dist.shape[0]
    if k >= 2:
        o = np.argpartition(dist, kth=np.arange(k), axis=1)[:, :k]
        return np.take_along_axis(dist, o, axis=1), np.take_along_axis(ind, o, axis=1)
    first = np.array([0 if np.isnan(r).all() else np.nanargmin(r) for r in dist])
    return dist[np.arange(n), first][:, None], ind[np.arange(n), first][:, None]


@pytest.mark.parametrize("K", [2, 64, 112, 113, 127, 128])
def test_narrow_select_topk_is_the_reference_selection_sort(ctx, K):
    """K = 113 .. 128 need more than 64 KiB of LDS (584 bytes per candidate) and an explicit allowance for it."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(K)
    for n in (1, 63, 64, 65, 130):
        dist = np.round(rng.random((n, K)) * 20) / 20        # multiples of 1/20: every row is full of ties
        dist[::7, K // 2] = np.nan
        dist[::5, K - 1] = np.nan
        dist[2::11, 0] = np.nan
        if n > 3:
            dist[3] = np.nan
        ind = np.argsort(rng.random((n, K)), axis=1).astype(np.int64) + 7 * np.arange(n)[:, None]
        dd, di = ctx.to_device(dist), ctx.to_device(ind)
        for k in sorted({1, 2, K - 1, K}):
            od, oi = N.select_topk(ctx, dd, di, k)
            rd, ri = _select_reference(dist, ind, k)
            assert_bits(oi.numpy(), ri, f"ids K={K} n={n} k={k}")
            assert_bits(od.numpy(), rd, f"values K={K} n={n} k={k}")


# ---- kz_mp_empiric, every launch branch of the wide kernel ------------------------------------------------------------------
@pytest.mark.parametrize("n,K,n_t,Kt", [(9, 129, 300, 129), (7, 128, 300, 129), (6, 129, 200, 5), (5, 819, 900, 64), (5, 820, 900, 64),
                                        (5, 1024, 1100, 1024), (3, 1025, 1100, 100), (2, 3276, 3400, 40), (2, 3277, 3400, 40),
                                        (2, 4096, 4200, 200)])
def test_mp_empiric_wide_branches(ctx, n, K, n_t, Kt):
    """20 bytes of LDS per candidate and wave: four waves up to K = 1024 (beyond 64 KiB from K = 820), one wave above (beyond
    64 KiB from K = 3277); K <= 128 with longer reverse lists takes this kernel too.  Distances are multiples of 1 / 16, so the
    strict comparisons meet equality; about half of the reverse-list ids are somebody's candidate, the rest are ids no list
    holds, negative ids and ids beyond 2^32 whose low bits are a candidate's."""
    from kiez_amd import _native as N
    rng = np.random.default_rng(K * 7 + Kt)
    ind = np.stack([rng.choice(n_t, K, replace=False) for _ in range(n)]).astype(np.int64)       # distinct per row, below n_t
    dist = np.sort(np.round(rng.random((n, K)) * 16) / 16, axis=1)
    ind_t2s = np.stack([rng.choice(2 * n_t, Kt, replace=False) for _ in range(n_t)]).astype(np.int64)
    ind_t2s[::5, 0] = -1 - ind_t2s[::5, 0]
    ind_t2s[::7, Kt - 1] = (1 << 32) + (ind_t2s[::7, Kt - 1] % n_t)
    ind_t2s[1::7, Kt // 2] = (1 << 40) + 5
    dist_t2s = np.sort(np.round(rng.random((n_t, Kt)) * 16) / 16, axis=1)
    matched = np.isin(ind_t2s[ind[0]], ind[0]).mean()
    assert 0.1 < matched < 0.9, matched
    out = ctx.empty((n, K), np.float64)
    d, i, dt, it = _dev(ctx, dist, ind, dist_t2s, ind_t2s)
    N._check(ctx.lib.kz_mp_empiric(ctx.handle, d.ptr, i.ptr, n, K, dt.ptr, it.ptr, n_t, Kt, out.ptr), "kz_mp_empiric")
    assert_bits(out.numpy(), R.mp_empiric_rows(dist, ind, dist_t2s, ind_t2s), f"K={K} Kt={Kt}")


# ---- kz_local_scaling(standard), kz_mp_normal: mpmath ------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def _abs_err(got, ref_mpf):
    """|got - ref| as floats, elementwise, in mpmath arithmetic (got converts exactly); NaN must meet NaN."""
    mp = _mp()
    err = np.zeros(got.shape)
    for idx in np.ndindex(got.shape):
        r = ref_mpf[idx]
        if r is None:
            assert np.isnan(got[idx]), (idx, got[idx])
        else:
            assert np.isfinite(got[idx]), (idx, got[idx], float(r))
            err[idx] = float(abs(mp.mpf(float(got[idx])) - r))
    return err


def _ls_reference(inner):
    """1 - exp(inner) at 40 digits from the float64 inner (None where inner is NaN: 0 / 0 radius)."""
    mp = _mp()
    ref = np.empty(inner.shape, dtype=object)
    for idx in np.ndindex(inner.shape):
        x = float(inner[idx])
        ref[idx] = None if x != x else mp.mpf(1) if x == -np.inf else 1 - mp.exp(mp.mpf(x))
    return ref


@pytest.mark.parametrize("K,n", [(1, 257), (5, 257), (50, 65), (129, 5), (300, 5)])
def test_local_scaling_standard_against_mpmath(ctx, K, n):
    """out = 1 - exp(inner), inner = -1 (d d) / (r_s r_t[ind]) (local_scaling.py:135-140).  inner is made of multiplications and one
    division, which test_csls_and_nicdm_bit_for_bit shows the device rounds as numpy does, so both sides hand exp the same
    float64; |device - (1 - exp(inner))| <= (U_EXP + 2) 2^-53, and numpy's own exp stays inside the same bound.
    Rows where exp underflows (out = 1), where 1 - exp cancels (inner ~ -1e-18 .. -1e-9), a zero radius (inner = -inf) and 0 / 0.
    Note (no threshold): numpy's own exp reaches 0.16 of the bound on these rows; the device's figure is printed (-s) and has not been recorded yet."""
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(300 + K)
    n_t = 37
    dist = np.sort(_rows(rng, n, K), axis=1)
    dist_t2s = np.sort(_rows(rng, n_t, 3), axis=1)
    dist[1::9] *= 1e4                                      # exp underflows
    dist[2::9] *= 1e-12                                    # 1 - exp cancels
    dist[3::9] *= 1e-6
    dist[4] = 0.0                                          # a zero radius on the query side: 0 / 0
    dist_t2s[0, -1] = 0.0                                  # a zero radius
    ind = _ids(rng, n, K, n_t)
    r_t = dist_t2s[:, -1].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = -1 * dist ** 2 / (dist[:, -1].reshape(-1, 1) * r_t[ind])
        host = O.ls_transform(dist, ind, dist_t2s, "standard")
    assert (inner < -800).any() and ((inner > -1e-9) & (inner < 0)).any() and np.isneginf(inner).any() and np.isnan(inner).any()
    ref = _ls_reference(inner)
    got = _ls(ctx, dist, ind, r_t, 0)
    e_dev, e_host = _abs_err(got, ref), _abs_err(host, ref)
    print(f"LS standard K={K}: device max err {e_dev.max() / LS_BOUND:.3f} of the bound, numpy {e_host.max() / LS_BOUND:.3f}")
    assert e_host.max() <= LS_BOUND, e_host.max() / LS_BOUND
    assert e_dev.max() <= LS_BOUND, (e_dev.max() / LS_BOUND, np.unravel_index(e_dev.argmax(), e_dev.shape))
    assert np.isnan(got[4]).all() and (got[inner < -800] == 1.0).all()


def _ndtr_mp(z):
    mp = _mp()
    if z != z:
        return None
    if z == np.inf:
        return mp.mpf(1)
    if z == -np.inf:
        return mp.mpf(0)
    return mp.erfc(-mp.mpf(float(z)) / mp.sqrt(2)) / 2


def _mp_normal_reference(dist, ind, mu, sd, mu_t, sd_t):
    """1 - p1 p2, p = ndtr(-(d - mu) / sd) at 40 digits from the float64 quotients (None where a quotient is NaN)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z1 = -((dist - mu[:, None]) / sd[:, None])
        z2 = -((dist - mu_t[ind]) / sd_t[ind])
    ref = np.empty(dist.shape, dtype=object)
    for idx in np.ndindex(dist.shape):
        p1, p2 = _ndtr_mp(z1[idx]), _ndtr_mp(z2[idx])
        ref[idx] = None if p1 is None or p2 is None else 1 - p1 * p2
    return ref


def _mp_normal(ctx, dist, ind, mu_t, sd_t):
    from kiez_amd import _native as N
    out = ctx.empty(dist.shape, np.float64)
    d, i, mt, st = _dev(ctx, dist, ind, mu_t, sd_t)
    N._check(ctx.lib.kz_mp_normal(ctx.handle, d.ptr, i.ptr, dist.shape[0], dist.shape[1], mt.ptr, st.ptr, out.ptr), "kz_mp_normal")
    return out.numpy()


@pytest.mark.parametrize("K,n", [(1, 257), (5, 257), (50, 65), (129, 5), (300, 5)])
def test_mp_normal_against_mpmath(ctx, K, n):
    """mu / sd of a list and of the reverse lists are the bit-checked row statistics (test_row_stats_bit_for_bit), the quotients
    -(d - mu) / sd one subtraction and one division, so erf / erfc get the same float64 on both sides;
    |device - (1 - p1 p2)| <= (2 U_ERF + 6) 2^-53, and scipy's ndtr stays inside the same bound.  Constant lists (sd = 0) on either
    side reproduce numpy's pattern: +-inf -> p = 0 / 1, 0 / 0 -> NaN.  (K = 1: every list is constant.)
    Note (no threshold): scipy's ndtr reaches 0.05 of the bound on these rows; the device's figure is printed (-s) and has not been recorded yet."""
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(400 + K)
    n_t, Kt = 37, 9
    dist = np.sort(_rows(rng, n, K), axis=1)
    dist_t2s = np.sort(_rows(rng, n_t, Kt), axis=1)
    dist[2] = 0.5                                      # sd = 0 on the query side: (d - mu) / 0 = 0 / 0
    dist_t2s[0] = 0.25                                     # sd_t = 0: +-inf, or 0 / 0 where d == 0.25
    dist_t2s[n_t - 1] = 2.0
    dist[4, 0] = 0.25
    dist[3] = 1e3 + 1e-3 * np.sort(rng.standard_normal(K))
    ind = _ids(rng, n, K, n_t)
    mu_t, sd_t = np.nanmean(dist_t2s, axis=1), np.nanstd(dist_t2s, axis=1)
    assert sd_t[0] == 0.0 and sd_t[n_t - 1] == 0.0
    d_t2s, d_dist = _dev(ctx, dist_t2s, dist)
    gm, gs = N.row_nanstats(ctx, d_t2s)
    assert_bits(gm.numpy(), mu_t), assert_bits(gs.numpy(), sd_t)
    gm, gs = N.row_nanstats(ctx, d_dist)
    mu, sd = np.nanmean(dist, axis=1), np.nanstd(dist, axis=1)
    assert_bits(gm.numpy(), mu), assert_bits(gs.numpy(), sd)
    ref = _mp_normal_reference(dist, ind, mu, sd, mu_t, sd_t)
    host = O.mp_normal_transform(dist, ind, dist_t2s)
    got = _mp_normal(ctx, dist, ind, mu_t, sd_t)
    e_dev, e_host = _abs_err(got, ref), _abs_err(host, ref)
    print(f"MP normal K={K}: device max err {e_dev.max() / MP_BOUND:.3f} of the bound, scipy {e_host.max() / MP_BOUND:.3f}")
    assert e_host.max() <= MP_BOUND, e_host.max() / MP_BOUND
    assert e_dev.max() <= MP_BOUND, (e_dev.max() / MP_BOUND, np.unravel_index(e_dev.argmax(), e_dev.shape))
    assert np.isnan(got[2]).all()
    beyond = (ind == 0) & (dist > 0.25) & ~np.isnan(got)              # -(d - 0.25) / 0 = -inf: p2 = 0
    assert (got[beyond] == 1.0).all() and (K == 1 or beyond.any())


# ---- NaN-bearing lists under MutualProximity normal -------------------------------------------------------------------------
def _nan_tailed(rng, K, all_nan_row):
    """Rows whose last 1 .. 5 entries are NaN, a row without NaN and (all_nan_row) a row of NaN only; without it every row keeps
    two finite entries at least."""
    a = np.sort(_rows(rng, 7, K), axis=1)
    for r in range(5):
        a[r, K - (r + 1 if all_nan_row else min(r + 1, K - 2)):] = np.nan
    if all_nan_row:
        a[5] = np.nan
    return a


@pytest.mark.parametrize("K", [5, 50, 129, 300])
def test_mp_normal_fit_state_skips_nan(ctx, K):
    """mutual_proximity.py:102-103: np.nanmean / np.nanstd.  A candidate list ends in NaN when n_candidates reaches rows whose
    distance is undefined (correlation against a constant row, dice / sokalsneath between all-false rows)."""
    from kiez_amd import _native as N
    a = _nan_tailed(np.random.default_rng(K), K, True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want_m, want_s = np.nanmean(a, axis=1), np.nanstd(a, axis=1)
    assert np.isfinite(want_m[[0, 1, 2, 3, 6]]).all() and np.isnan(want_m[5]) and np.isnan(want_s[5])
    d = ctx.to_device(a)
    # kz_row_stats: the std is np.nanstd, the mean stays ndarray.mean (CSLS and NICDM propagate a NaN)
    m, s, _ = N.row_stats(ctx, d, mean=True, std=True)
    assert_bits(s.numpy(), want_s, "row_stats std")
    assert_bits(m.numpy(), a.mean(axis=1), "row_stats mean")
    assert np.isnan(m.numpy()[:6]).all() and np.isfinite(m.numpy()[6])
    gm, gs = N.row_nanstats(ctx, d)
    assert_bits(gm.numpy(), want_m, "nanmean")
    assert_bits(gs.numpy(), want_s, "nanstd")


@pytest.mark.parametrize("K", [5, 50, 129, 300])
def test_mp_normal_keeps_the_finite_entries_of_a_nan_tailed_list(ctx, K):
    """mutual_proximity.py:177-178: NaN in, NaN out at the same positions; every other entry is finite and within the bound of
    test_mp_normal_against_mpmath of the reference fed with nanmean / nanstd."""
    from oracle import kiez_oracle as O
    rng = np.random.default_rng(500 + K)
    dist = _nan_tailed(rng, K, True)
    dist_t2s = _nan_tailed(rng, K, False)
    n_t = dist_t2s.shape[0]
    ind = _ids(rng, dist.shape[0], K, n_t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mu, sd = np.nanmean(dist, axis=1), np.nanstd(dist, axis=1)
        mu_t, sd_t = np.nanmean(dist_t2s, axis=1), np.nanstd(dist_t2s, axis=1)
        host = O.mp_normal_transform(dist, ind, dist_t2s)
    assert np.isfinite(mu_t).all() and (sd_t > 0).all()
    ref = _mp_normal_reference(dist, ind, mu, sd, mu_t, sd_t)
    got = _mp_normal(ctx, dist, ind, mu_t, sd_t)
    # NaN in, NaN out, finite elsewhere -- in every list that keeps two finite entries at least (one alone has sd = 0: 0 / 0)
    few = np.isfinite(dist).sum(axis=1) < 2
    np.testing.assert_array_equal(np.isnan(host)[~few], np.isnan(dist)[~few])
    assert np.isnan(host[few]).all() and few.sum() == (3 if K == 5 else 1)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(host))
    assert np.isfinite(got[6]).all() and np.isfinite(got[0, :K - 1]).all() and np.isnan(got[5]).all()
    e_dev, e_host = _abs_err(got, ref), _abs_err(host, ref)
    print(f"MP normal, NaN tails, K={K}: device max err {e_dev.max() / MP_BOUND:.3f} of the bound, scipy {e_host.max() / MP_BOUND:.3f}")
    assert e_host.max() <= MP_BOUND
    assert e_dev.max() <= MP_BOUND, e_dev.max() / MP_BOUND


def _sort_topk_nan_last(hub, ind, k):
    """O.sort_topk with NaN ranked last, the order np.argpartition gives it (the oracle's np.argmin would pick a NaN first);
    MutualProximity values lie in [0, 1], so +inf stands for nothing else."""
    from oracle import kiez_oracle as O
    d, i = O.sort_topk(np.where(np.isnan(hub), np.inf, hub), ind, k)
    return np.where(np.isinf(d), np.nan, d), i


def _nan_problem(metric):
    rng = np.random.default_rng(17)
    if metric == "dice":                                   # 40 x 30 boolean rows, three all-false rows on each side
        src, tgt = rng.random((40, 30)) < 0.4, rng.random((40, 30)) < 0.4
        bad_s, bad_t = [4, 17, 33], [0, 21, 39]
        src[bad_s] = False
        tgt[bad_t] = False
        from tests.boolean_restate import knn
        return src, tgt, bad_s, bad_t, lambda x, y, k: knn("dice", x, y, k)
    src, tgt = rng.standard_normal((40, 30)), rng.standard_normal((40, 30))
    bad_t = [3, 28]                                        # two constant target rows: correlation with them is 0 / 0
    tgt[3] = 1.5
    tgt[28] = -2.0
    from tests.metric_restate import knn
    return src, tgt, [], bad_t, lambda x, y, k: knn("correlation", x, y, k)


@pytest.mark.parametrize("metric", ["dice", "correlation"])
def test_mp_normal_through_the_api_on_lists_that_end_in_nan(metric):
    """n_candidates = n_target: every list reaches the rows its distance to is undefined.  The expected result is the candidate
    lists of the host restatement of the metric through the oracle's MutualProximity normal and final sort.
    correlation: every list ends in two NaN and keeps 38 finite entries, which a mean that does not skip NaN turns into a row of
    NaN.  dice: the lists that end in NaN are those of the all-false rows, whose finite entries are all 1 (sd = 0: NaN by 0 / 0
    with either mean); the case pins the NaN pattern and the rows without NaN."""
    from kiez_amd import Kiez
    from oracle import kiez_oracle as O
    from tests.test_gpu_boolean_metrics import _runs_equal
    src, tgt, bad_s, bad_t, knn = _nan_problem(metric)
    K = tgt.shape[0]
    dist, ind = knn(src, tgt, K)
    dist_t2s, _ = knn(tgt, src, src.shape[0])
    # the premise, on the host: NaN-tailed lists for exactly the rows that must have them
    tails = np.isnan(dist).sum(axis=1)
    if metric == "dice":
        assert (tails[bad_s] == len(bad_t)).all() and (np.delete(tails, bad_s) == 0).all()
        assert (np.isnan(dist_t2s).sum(axis=1)[bad_t] == len(bad_s)).all()
    else:
        assert (tails == len(bad_t)).all() and np.isnan(dist_t2s[bad_t]).all() and np.isfinite(np.delete(dist_t2s, bad_t, axis=0)).all()
    assert all(np.isnan(r[K - t:]).all() for r, t in zip(dist, tails))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hub = O.mp_normal_transform(dist, ind, dist_t2s)
        kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness="MutualProximity",
                  hubness_kwargs={"method": "normal"})
        kz.fit(src, tgt)
        for k in (10, K):
            d, i = kz.kneighbors(k)
            wd, wi = _sort_topk_nan_last(hub, ind, k)
            np.testing.assert_array_equal(np.isnan(d), np.isnan(wd), err_msg=f"{metric} k={k}: NaN where the reference is finite")
            np.testing.assert_allclose(d, wd, rtol=0, atol=MP_BOUND, equal_nan=True)
            assert _runs_equal(wd, wi, d, i, rtol=1e-12), f"{metric} k={k}"


# ---- kz_dsl_fit, kz_dsl_transform -------------------------------------------------------------------------------------------
DSL_SHAPES = [(1, 1, 37), (63, 5, 37), (64, 20, 5), (65, 5, 5), (130, 1, 37), (300, 20, 5), (300, 5, 37), (64, 1, 5)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("centre,spread", [(0.0, 1.0), (100.0, 0.01)])
@pytest.mark.parametrize("case", range(len(DSL_SHAPES)))
def test_dissimlocal_against_exact_arithmetic(ctx, case, centre, spread, dtype):
    """kz_dsl_fit: t2c[j] = sum_k (t_jk - (sum_m s[ind[j, m], k]) / Kt)^2; kz_dsl_transform: out[i, m] = |q_i - t_c|^2 -
    |q_i - mean_m t_c|^2 - t2c[c] with t2c as given.  Reference: the same in fractions.Fraction.  Bound, per element, with
    u = 2^-53 and gamma_n = n u / (1 - n u) (tests/hubness_restate.py: _sq_bound, dsl_transform_bound):
      a centroid coordinate is off by at most e_k = gamma_Kt mean_m |s_mk|, which enters its difference: 2 |x_k - c_k| e_k + e_k^2
      per coordinate; a sum of squares (ceil(d / 64) terms per lane, a six-step butterfly, the difference twice, the product once)
      by gamma_{ceil(d / 64) + 9} of its value; each of the two subtractions by u of its result.
    The oracle's float64 evaluation must lie inside the same bound.  Data at unit scale and centred at 100 with spread 0.01,
    where the differences cancel five digits; begin offsets nonzero in every other case; the reported minimum is the minimum of
    the kernel's own output and is left alone when it was initialised below it.
    Note (no threshold): the oracle's float64 evaluation reaches 0.41 (fit) and 0.26 (transform) of the bound on these cases; the
    device's figures are printed (-s) and have not been recorded yet."""
    import torch
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    from tests.cpu_engine import OracleEngine, _Mat
    d, K, n = DSL_SHAPES[case]
    begin = 0 if case % 2 == 0 else 3
    rng = np.random.default_rng(case * 10 + (dtype == np.float32))
    n_s = max(K, 11)
    src = (centre + spread * rng.standard_normal((n_s, d))).astype(dtype)
    tgt = (centre + spread * rng.standard_normal((begin + max(n, K + 2), d))).astype(dtype)
    sm, tm = N.DeviceMatrix(ctx, src, "sqeuclidean"), N.DeviceMatrix(ctx, tgt, "sqeuclidean")
    # fit: n reverse-list rows for the target rows begin .. begin + n
    ind_t2s = _distinct_ids(rng, n, K, n_s)
    t2c = ctx.empty((n,), np.float64)
    (d_ind_t2s,) = _dev(ctx, ind_t2s)
    N._check(ctx.lib.kz_dsl_fit(ctx.handle, d_ind_t2s.ptr, n, K, sm.handle, tm.handle, begin, t2c.ptr), "kz_dsl_fit")
    got = t2c.numpy()
    exact = R.dsl_fit_exact(ind_t2s, src, tgt[begin:begin + n])
    bound = R.dsl_fit_bound(ind_t2s, src, tgt[begin:begin + n])
    host = O.dsl_fit(ind_t2s, src.astype(np.float64), tgt[begin:begin + n].astype(np.float64))
    worst = 0.0
    for j in range(n):
        assert abs(Fraction(float(host[j])) - exact[j]) <= bound[j], ("oracle", j, float(host[j]), float(exact[j]), float(bound[j]))
        err = abs(Fraction(float(got[j])) - exact[j])
        worst = max(worst, float(err / bound[j]) if bound[j] else 0.0)
        assert err <= bound[j], ("kz_dsl_fit", j, float(got[j]), float(exact[j]), float(bound[j]))
    # transform: n query rows begin .. begin + n of a query matrix (the source side), candidates in the target matrix
    n_t = tgt.shape[0]
    Kc = K
    qry = (centre + spread * rng.standard_normal((begin + n, d))).astype(dtype)
    qm = N.DeviceMatrix(ctx, qry, "sqeuclidean")
    ind = _distinct_ids(rng, n, Kc, n_t)
    t2c_all = np.abs(rng.standard_normal(n_t)) * spread * spread * d                 # taken as given: arbitrary doubles of t2c's scale
    out = ctx.empty((n, Kc), np.float64)
    gmin = ctx.to_device(np.array([np.inf]))
    d_ind, d_t2c = _dev(ctx, ind, t2c_all)
    args = (d_ind.ptr, n, Kc, qm.handle, begin, tm.handle, d_t2c.ptr)
    N._check(ctx.lib.kz_dsl_transform(ctx.handle, *args, out.ptr, gmin.ptr), "kz_dsl_transform")
    got = out.numpy()
    assert_bits(gmin.numpy(), np.array([got.min()]), "the reported minimum")
    low = ctx.to_device(np.array([got.min() - 1.0]))
    N._check(ctx.lib.kz_dsl_transform(ctx.handle, *args, out.ptr, low.ptr), "kz_dsl_transform")
    assert_bits(low.numpy(), np.array([got.min() - 1.0]), "a minimum below the output's")
    assert_bits(out.numpy(), got)
    exact = R.dsl_transform_exact(ind, qry[begin:], tgt, t2c_all)
    bound = R.dsl_transform_bound(ind, qry[begin:], tgt, t2c_all)
    host, _ = OracleEngine().dsl_transform(torch.from_numpy(ind), _Mat(torch.from_numpy(qry), "sqeuclidean"), begin,
                                           _Mat(torch.from_numpy(tgt), "sqeuclidean"), torch.from_numpy(t2c_all))
    host = host.numpy()
    worst_t = 0.0
    for i in range(n):
        for m in range(Kc):
            assert abs(Fraction(float(host[i, m])) - exact[i][m]) <= bound[i][m], ("oracle", i, m, float(host[i, m]), float(exact[i][m]))
            err = abs(Fraction(float(got[i, m])) - exact[i][m])
            worst_t = max(worst_t, float(err / bound[i][m]))
            assert err <= bound[i][m], ("kz_dsl_transform", i, m, float(got[i, m]), float(exact[i][m]), float(bound[i][m]))
    print(f"DSL d={d} K={K} n={n} {np.dtype(dtype).name} centre={centre}: fit max err {worst:.3f} of the bound, transform {worst_t:.3f}")
