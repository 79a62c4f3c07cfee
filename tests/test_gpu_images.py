"""The per-matrix kernels of kiez_amd/csrc/kz_pack.hip, one by one, against tests/image_restate.py: kz_norms_kernel,
kz_pack_f32_kernel, kz_pack_bf_kernel, kz_colsum_kernel + kz_center_finish_kernel, kz_pack_h_kernel (own, permuted, dealt and
row-list images), kz_norm64_kernel and kz_corr_rows_kernel.  The buffers come through the test hook kz_selftest_image as they lie in
HBM; no search runs except where a test says so.

Why directly: a wrong operand only makes fewer rows certify (the float64 re-rank still returns the oracle's answer), and a residual
or a maximum that is too SMALL makes the bound of DESIGN.md section 4 certify rows it must not -- neither shows in a parity test.

Tolerances.  A float64 sum of m non-negative terms accumulated by fma chains and a butterfly, in any order, is within
(m - 1) 2^-53 (1 + o(1)) relative of the exact sum; the kernels add at most d_pad products plus the tree's levels, hence
(d + 8) 2^-53 for the norms and (d_pad + 8) 2^-53 for the fp16 row sums.  A correctly rounded sqrt of such a sum is within half that
plus 2^-53.  The column mean: float32 rounding of the result (2^-24 |mean|) plus the float64 summation error of n terms and of
the up to 260 partial sums ((n + 260) 2^-53 mean|op|).  Everything else is bit for bit.

Mutations of kz_pack.hip tried by hand against this module (each fails the tests named):
  residual taken before the clamp            test_fp16_image_regimes[clamp-float32 / -float64], test_products_stay_inside_the_bound[clamp]
  d_max over one wave's rows only            51 cases: test_fp16_image_and_row_statistics (34: every shape but 1 x 17), the regime, bound,
                                             inheritance, misaligned, dealt and row-list tests (whatever builds an image of > 16 rows)
  lo plane from float32(x) instead of x      43 cases: test_float32_and_bf16_images, every float64 case and every cosine case (40),
                                             test_rows_four_bytes_off_a_16_byte_boundary[cosine-*]
  single-trip grid loop in kz_pack_h_kernel  test_fp16_image_and_row_statistics[65541x20-*], test_dealt_image_past_one_grid_trip
  mu padding left unwritten                  48 cases: test_fp16_image_and_row_statistics (35: every width that is no multiple of 16, "mu
                                             padding"), test_scale_exponent_is_clamped, the misaligned, regime and bound tests
(The padding checks rely on _poison: a buffer fresh from the allocator may happen to be zero.)
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import image_restate as R
from tests import value_regimes as V

pytestmark = pytest.mark.gpu

(SQN, BIAS, STATS, F32, BF, NORM64, CORR, MU, SCALE, H, H_BIAS, ROWQ, DMAX, DEALT_PERM, DEALT_H, DEALT_BIAS, ROWS_H,
 ROWS_BIAS) = range(18)
U = 2.0 ** -53
DTYPES = (np.float32, np.float64)
METRICS = ("euclidean", "cosine")


def _native():
    from kiez_amd import _native as N
    return N, N.Context.get()


def _read(m, what, dtype, partner=None, arg=0, rows=None):
    """One buffer of matrix m through the hook: size query, then the bytes."""
    N, ctx = _native()
    rows_p = None
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        rows_p = rows.ctypes.data_as(C.POINTER(C.c_int))
    head = (ctx.handle, m.handle, partner.handle if partner is not None else None, what, arg, rows_p)
    nb = C.c_size_t(0)
    N._check(ctx.lib.kz_selftest_image(*head, None, 0, C.byref(nb)), "kz_selftest_image")
    out = np.empty(nb.value, dtype=np.uint8)
    if nb.value:
        N._check(ctx.lib.kz_selftest_image(*head, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(nb)), "kz_selftest_image")
        assert nb.value == out.nbytes
    return out.view(dtype)


def _poison(*sizes):
    """Leave released device buffers of these sizes, filled with 0xFF, in the context's pool: the next allocations of the same sizes
    get them, so a padding element the kernels do not write shows (a fresh allocation may happen to be zero)."""
    N, ctx = _native()
    held = [ctx.to_device(np.full((max(int(s), 16) + 255) // 256 * 256, 0xFF, dtype=np.uint8)) for s in sizes]
    del held


def _rows(n, d, dtype, seed=0):
    """randn rows with a zero row, a duplicate of row 0 and a row whose only non-zero element is in the last column."""
    x = np.random.RandomState(7919 * d + n + seed).randn(n, d).astype(dtype)
    if n >= 5:
        x[n // 2] = 0.0
        x[1] = 0.0
        x[1, d - 1] = 3.0
        x[n - 1] = x[0]
    return x


def _matrix(x, metric):
    N, ctx = _native()
    npad = R.n_pad(len(x))
    _poison(npad * 4, npad * 4, len(x) * 8)
    return N.DeviceMatrix(ctx, x, metric)


def _misaligned(x, metric):
    """Borrowed float32 device rows whose base is 4 bytes off a 16-byte boundary: a flat buffer of n d + 1 floats, viewed from element 1."""
    N, ctx = _native()
    n, d = x.shape
    flat = np.zeros(n * d + 1, dtype=np.float32)
    flat[1:] = x.ravel()
    dev = ctx.to_device(flat)
    assert dev.ptr.value % 16 == 0
    return N.DeviceMatrix(ctx, None, metric, device_ptr=dev.ptr.value + 4, shape=(n, d), dtype=np.float32, borrow=True, keepalive=dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} elements differ, first at flat index {bad[:5]}"


def _sq_sums(x):
    """Exact squared row norms, correctly rounded (float32 squares are exact in float64; float64 ones are split)."""
    x64 = np.asarray(x, dtype=np.float64)
    return R.fsum_rows(x64 * x64 if x.dtype == np.float32 else R.exact_squares(x64))


def _stats(m):
    raw = _read(m, STATS, np.uint8)
    assert raw.nbytes == 40
    return raw[:16].view(np.float64), int(raw[32:36].view(np.int32)[0])


# ---- the checks, shared by the aligned and the misaligned cases -----------------------------------------------------------------
def check_creation(m, x, metric):
    n, d = x.shape
    npad = R.n_pad(n)
    sqn = _read(m, SQN, np.float64)
    bias = _read(m, BIAS, np.float32)
    st, flag = _stats(m)
    assert sqn.shape == (n,) and bias.shape == (npad,) and flag == 0
    exact = _sq_sums(x)
    x64 = np.abs(np.asarray(x, dtype=np.float64))
    if metric == "cosine":
        want = np.sqrt(exact)
        want[exact == 0.0] = 1.0
        assert (sqn[exact == 0.0] == 1.0).all()
        assert (np.abs(sqn - want) <= (d + 8) * U * want).all(), float((np.abs(sqn - want) / want).max())
        _assert_bits(bias[:n], np.zeros(n, dtype=np.float32), "cosine bias")
        assert st[0] == 1.0
        _assert_bits(st[1:2], np.array([(x64.max(axis=1) / sqn).max()]), "max |operand| (cosine)")
    else:
        assert (np.abs(sqn - exact) <= (d + 8) * U * exact).all(), float((np.abs(sqn - exact) / np.maximum(exact, 1e-300)).max())
        _assert_bits(bias[:n], (-0.5 * sqn).astype(np.float32), "bias")
        _assert_bits(st[0:1], np.sqrt(sqn.max(keepdims=True)), "max row norm")
        _assert_bits(st[1:2], np.array([x64.max()]), "max |x|")
    _assert_bits(bias[n:], np.full(npad - n, -np.inf, dtype=np.float32), "bias of the padding rows")
    return sqn


def check_lower_images(m, x, metric, sqn):
    n, d = x.shape
    npad, dpad = R.n_pad(n), R.kg(d) * 4
    op = R.operands(x, metric, sqn)
    row, k = R.grid(n, d)
    _poison(npad * dpad * 4, npad * dpad * 4)
    want = np.zeros(npad * dpad, dtype=np.float32)
    want[R.f32_offset(row, k, d)] = op.astype(np.float32)
    _assert_bits(_read(m, F32, np.float32), want, "float32 image")
    got = _read(m, BF, np.uint16)
    hi, lo = R.bf_split(op)
    want = np.zeros(2 * npad * dpad, dtype=np.uint16)
    want[R.bf_offset(row, k, d, 0)] = hi
    want[R.bf_offset(row, k, d, 1)] = lo
    _assert_bits(got, want, "split-bf16 image")
    # the bound the bf16 tier's certification relies on, on the device's own bytes
    err = np.abs((op - R.bf16_to_f64(got[R.bf_offset(row, k, d, 0)])) - R.bf16_to_f64(got[R.bf_offset(row, k, d, 1)]))
    assert (err <= R.SPLIT_BOUND * np.abs(op)).all()
    n64 = _read(m, NORM64, np.float64)
    if metric == "cosine" and x.dtype == np.float32 and d % 4 == 0 and d <= 256:
        _assert_bits(n64, (x.astype(np.float64) / sqn[:, None]).ravel(), "norm64")
    else:
        assert n64.size == 0


def check_centre(src, x_src, metric, sqn_src, mu, scale):
    """mu / scale of an image against the matrix the centre was taken from."""
    n, d = x_src.shape
    nsr = R.h_nsr(R.kg(d))
    assert mu.shape == (16 * nsr,) and scale.shape == (2,)
    op = R.operands(x_src, metric, sqn_src)
    mean = R.fsum_rows(op.T) / n
    mean_abs = R.fsum_rows(np.abs(op.T)) / n
    tol = 2.0 ** -24 * np.abs(mean) + (n + 260) * U * mean_abs
    err = np.abs(mu[:d].astype(np.float64) - mean)
    assert (err <= tol).all(), (int(np.argmax(err - tol)), float(err.max()))
    _assert_bits(mu[d:], np.zeros(16 * nsr - d, dtype=np.float32), "mu padding")
    amax = _stats(src)[0][1]
    S = R.scale_of(amax)
    assert scale[0] == S and scale[1] == 1.0 / (S * S)
    if 0.0 < amax:
        e = math.frexp(amax)[1]
        assert S == math.ldexp(1.0, max(-100, min(100, 13 - e)))
    return S


def check_h_image(m, x, metric, sqn, mu, S, packed, bias, rowq=None, dmax=None, perm=None):
    """An fp16 image (own, dealt or row-list: image row r holds matrix row perm[r]) against the restated pipeline on the device's mu and S."""
    n, d = x.shape
    nsr = R.h_nsr(R.kg(d))
    dp = 16 * nsr
    perm = np.arange(n) if perm is None else np.asarray(perm)
    n_img = len(perm)
    npad = R.n_pad(n_img)
    op = R.operands(x, metric, sqn)
    v, h = R.h_pipeline(op, mu[:d], S)
    c2, nh, nr = R.h_row_stats(v, h, S)
    row, k = R.grid(n_img, d)
    want = np.zeros(npad * dp, dtype=np.float16)
    want[R.h_offset(row, k, nsr)] = h[perm]
    assert packed.shape == want.shape
    _assert_bits(packed, want, "fp16 image")
    if rowq is not None:
        rowq = rowq.reshape(n, 3)
        rel = (dp + 8) * U
        assert (np.abs(rowq[:, 0] - c2) <= rel * c2).all(), "|x_c|^2"
        assert (np.abs(rowq[:, 1] - nh) <= (rel + U) * nh).all(), "|x_h|"
        assert (np.abs(rowq[:, 2] - nr) <= (rel + U) * nr).all(), ("|x_c - x_h|", float(np.abs(rowq[:, 2] - nr).max()))
        _assert_bits(bias[:n], (((-0.5 * rowq[:, 0]) * S) * S).astype(np.float32), "image bias")
        _assert_bits(dmax, np.array([rowq[:, 1].max(), rowq[:, 2].max(), rowq[:, 0].max()]), "d_max")
    _assert_bits(bias[n_img:], np.full(npad - n_img, -np.inf, dtype=np.float32), "image bias of the padding rows")
    return v, h


def _own_image(m, x, metric, sqn, partner=None, check_centre_of=None):
    """Build and check m's own fp16 image (centre shared with `partner`); returns (mu, S, v, h, rowq, dmax, packed, bias)."""
    n, d = x.shape
    nsr = R.h_nsr(R.kg(d))
    npad = R.n_pad(n)
    _poison(16 * nsr * 4, npad * nsr * 32 + 32 * 4096, npad * 4, n * 24)
    mu = _read(m, MU, np.float32, partner)
    scale = _read(m, SCALE, np.float64, partner)
    if check_centre_of is not None:
        check_centre(*check_centre_of, mu, scale)
    S = float(scale[0])
    packed, bias = _read(m, H, np.float16, partner), _read(m, H_BIAS, np.float32, partner)
    rowq, dmax = _read(m, ROWQ, np.float64, partner), _read(m, DMAX, np.float64, partner)
    v, h = check_h_image(m, x, metric, sqn, mu, S, packed, bias, rowq, dmax)
    return mu, S, v, h, rowq.reshape(n, 3), dmax, packed, bias


# ---- shapes --------------------------------------------------------------------------------------------------------------------
# rows 1, 127, 129, 1000, 3073 (kz_colsum_kernel's four-row body), 65541 (past every grid-stride trip; d = 20 only); widths with the
# scalar row path (float32: 6, float64: 3 and 2), the 16-byte path (4, 20), an odd tail, several slices, all-padding slices (513, 1040)
SHAPES = [(1, 17), (127, 1), (129, 2), (129, 3), (129, 4), (127, 6), (1000, 17), (1000, 20), (3073, 33), (129, 260), (127, 300),
          (129, 384), (127, 513), (129, 1040), (3073, 260), (65541, 20)]
CASES = [pytest.param(n, d, dtype, metric, id=f"{n}x{d}-{np.dtype(dtype).name}-{metric}")
         for i, (n, d) in enumerate(SHAPES) for j, dtype in enumerate(DTYPES) for metric in METRICS
         # (the two largest shapes: each dtype with one metric)
         if n * d < 500_000 or (metric == METRICS[(i + j) % 2])]
H_CASES = [c for c in CASES if R.h_slices_ok(R.kg(c.values[1]))]


@pytest.mark.parametrize("n,d,dtype,metric", CASES)
def test_creation(n, d, dtype, metric):
    x = _rows(n, d, dtype)
    check_creation(_matrix(x, metric), x, metric)


@pytest.mark.parametrize("n,d,dtype,metric", CASES)
def test_float32_and_bf16_images(n, d, dtype, metric):
    x = _rows(n, d, dtype)
    m = _matrix(x, metric)
    check_lower_images(m, x, metric, _read(m, SQN, np.float64))


@pytest.mark.parametrize("n,d,dtype,metric", H_CASES)
def test_fp16_image_and_row_statistics(n, d, dtype, metric):
    x = _rows(n, d, dtype)
    m = _matrix(x, metric)
    sqn = _read(m, SQN, np.float64)
    mu = _own_image(m, x, metric, sqn, check_centre_of=(m, x, metric, sqn))[0]
    # the same bits from a second build of a fresh matrix (fixed summation order)
    m2 = _matrix(x, metric)
    _assert_bits(_read(m2, MU, np.float32), mu, "mu of a second build")


@pytest.mark.parametrize("n,d", [(129, 17), (130, 385), (127, 496)])
def test_hook_refuses_what_has_no_image(n, d):
    N, ctx = _native()
    x = _rows(n, d, np.float32)
    if not R.h_slices_ok(R.kg(d)):
        m = _matrix(x, "euclidean")
        assert _read(m, F32, np.float32).size == R.n_pad(n) * R.kg(d) * 4
        with pytest.raises(ValueError, match="no fp16 image"):
            _read(m, H, np.float16)
        return
    m = _matrix(x, "euclidean")
    with pytest.raises(ValueError, match="unknown buffer"):
        _read(m, 18, np.uint8)
    with pytest.raises(ValueError, match="destination"):      # a capacity below the size
        nb = C.c_size_t(0)
        buf = np.empty(8, dtype=np.uint8)
        N._check(ctx.lib.kz_selftest_image(ctx.handle, m.handle, None, SQN, 0, None, buf.ctypes.data_as(C.c_void_p), 8, C.byref(nb)))
    b = _matrix((x != 0).astype(np.float32), "jaccard")
    with pytest.raises(ValueError, match="rows-only or boolean"):
        _read(b, SQN, np.float64)
    dev = ctx.to_device(x)
    ro = N.DeviceMatrix(ctx, None, "euclidean", device_ptr=dev.ptr.value, shape=x.shape, dtype=np.float32, borrow=True, keepalive=dev,
                        rows_only=True)
    with pytest.raises(ValueError, match="rows-only or boolean"):
        _read(ro, SQN, np.float64)
    rows_v, cols_v = N.DeviceMatrix.precomputed(ctx, np.abs(x))
    with pytest.raises(ValueError, match="precomputed"):
        _read(rows_v, SQN, np.float64)
    man = _matrix(x, "manhattan")
    assert _read(man, SQN, np.float64).shape == (n,)
    with pytest.raises(ValueError, match="MFMA metrics"):
        _read(man, F32, np.float32)


@pytest.mark.parametrize("d", [4, 20, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_rows_four_bytes_off_a_16_byte_boundary(d, metric):
    """Every kernel of kz_pack.hip takes its scalar path (kz_row_vec_ok); creation and images only, no search."""
    x = _rows(129, d, np.float32)
    m = _misaligned(x, metric)
    sqn = check_creation(m, x, metric)
    check_lower_images(m, x, metric, sqn)
    # bit for bit what the aligned matrix gives (kz_row4: both paths feed the same fma chain)
    a = _matrix(x, metric)
    _assert_bits(sqn, _read(a, SQN, np.float64), "sqn of the misaligned rows")
    if R.h_slices_ok(R.kg(d)):
        mu, S, v, h, rowq, dmax, packed, bias = _own_image(m, x, metric, sqn, check_centre_of=(m, x, metric, sqn))
        _assert_bits(packed, _read(a, H, np.float16), "fp16 image of the misaligned rows")
        _assert_bits(rowq, _read(a, ROWQ, np.float64).reshape(-1, 3), "rowq of the misaligned rows")


@pytest.mark.parametrize("n,d", [(129, 33), (1000, 20), (127, 260), (300, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_correlation_row_state(n, d, dtype):
    x = _rows(n, d, dtype)
    m = _matrix(x, "correlation")
    corr = _read(m, CORR, np.float64).reshape(n, 2)
    x64 = x.astype(np.float64)
    mean = x64.sum(axis=1) / d            # numpy's pairwise sum
    u = x64 - mean[:, None]
    s0, s1 = np.zeros(n), np.zeros(n)
    for j in range(0, d & ~1, 2):         # scipy's two interleaved partial sums
        s0 += u[:, j] * u[:, j]
        s1 += u[:, j + 1] * u[:, j + 1]
    s = s0 + s1
    if d & 1:
        s = s + u[:, d - 1] * u[:, d - 1]
    _assert_bits(corr[:, 0], mean, "row mean")
    _assert_bits(corr[:, 1], np.sqrt(s), "norm of the centred row")
    assert _read(_matrix(x, "euclidean"), CORR, np.float64).size == 0


# ---- finiteness ----------------------------------------------------------------------------------------------------------------
# (row, column) of the bad value: the first element, the last element of an odd d, the last row; and, at 65541 x 20, a row of the third
# grid-stride trip of kz_norms_kernel (32768 rows per trip) and the last row
SMALL_BAD = ((129, 33), [(0, 0), (5, 32), (128, 7)])
LARGE_BAD = ((65541, 20), [(65537, 3), (65540, 19)])


def _device_rows(x, metric):
    N, ctx = _native()
    dev = ctx.to_device(x)
    return N.DeviceMatrix(ctx, None, metric, device_ptr=dev.ptr.value, shape=x.shape, dtype=x.dtype, borrow=True, keepalive=dev)


@pytest.mark.parametrize("shape,places", [SMALL_BAD, LARGE_BAD], ids=["129x33", "65541x20"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_non_finite_input_is_flagged(shape, places, dtype, metric):
    N, ctx = _native()
    base = _rows(*shape, dtype)
    for bad in (np.nan, np.inf, -np.inf):
        for (r, c) in places:
            x = base.copy()
            x[r, c] = bad
            with pytest.raises(ValueError, match="NaN, infinity"):          # host rows: at creation
                N.DeviceMatrix(ctx, x, metric)
            m = _device_rows(x, metric)                                      # device rows: nothing is waited for ...
            with pytest.raises(ValueError, match="NaN, infinity"):          # ... the hook reads the verdict
                _read(m, SQN, np.float64)
            if shape[0] < 1000 or (bad is np.nan and c == 19):
                m = _device_rows(x, metric)
                with pytest.raises(ValueError, match="NaN, infinity"):      # ... and so does the first search
                    N.knn(ctx, m, m, 1)
    assert _stats(_device_rows(base, metric))[1] == 0


def _row_with_sq(target):
    """[x0, x1] float64 with RN(x0^2 + x1^2) == target, where x0^2 is exact: what kz_norms_kernel's fma chain gives for the row."""
    t = int(target)
    x0 = (math.isqrt(t) >> 24) << 24          # 26 significant bits: the square is exact in float64
    x1 = math.isqrt(t - x0 * x0)
    assert float(x0 * x0 + x1 * x1) == target and float(x0) == x0 and float(x1) == x1
    return [float(x0), float(x1)]


def test_input_limit_is_1e30_to_the_ulp():
    N, ctx = _native()
    below, above = np.nextafter(1e30, 0.0), np.nextafter(1e30, np.inf)
    x = np.array([[1.0, 2.0], _row_with_sq(below), [3.0, 4.0]])
    m = N.DeviceMatrix(ctx, x, "euclidean")
    sqn = _read(m, SQN, np.float64)
    assert sqn[1] == below and _stats(m)[1] == 0
    x[1] = _row_with_sq(1e30)                 # the limit itself passes
    assert _read(N.DeviceMatrix(ctx, x, "euclidean"), SQN, np.float64)[1] == 1e30
    x[1] = _row_with_sq(above)
    with pytest.raises(ValueError, match="1e30"):
        N.DeviceMatrix(ctx, x, "euclidean")
    with pytest.raises(ValueError, match="1e30"):
        _read(_device_rows(x, "euclidean"), SQN, np.float64)


# ---- centre --------------------------------------------------------------------------------------------------------------------
def test_scale_exponent_is_clamped():
    x = np.ldexp(_rows(300, 40, np.float64), -110)
    for metric in METRICS:
        m = _matrix(x, metric)
        scale = _read(m, SCALE, np.float64)
        if metric == "euclidean":
            assert scale[0] == 2.0 ** 100 and scale[1] == 2.0 ** -200
        sqn = _read(m, SQN, np.float64)
        check_centre(m, x, metric, sqn, _read(m, MU, np.float32), scale)
    # (the lower clamp, 2^-100, needs |x| >= 2^113: past the input limit of |x|^2 <= 1e30, no valid matrix reaches it)
    big = np.ldexp(_rows(130, 40, np.float64), 45)
    m = _matrix(big, "euclidean")
    assert _read(m, SCALE, np.float64)[0] == R.scale_of(np.abs(big).max()) >= 2.0 ** -40


def test_centre_is_inherited():
    d = 40
    xa, xb, xc = _rows(300, d, np.float32, 1), _rows(200, d, np.float32, 2) + np.float32(0.5), _rows(150, d, np.float32, 3)
    a, b, c = _matrix(xa, "euclidean"), _matrix(xb, "euclidean"), _matrix(xc, "euclidean")
    sqn_b = _read(b, SQN, np.float64)
    # with partner B the centre is B's (the index of the pair), and both images share it
    mu_a = _read(a, MU, np.float32, partner=b)
    check_centre(b, xb, "euclidean", sqn_b, mu_a, _read(a, SCALE, np.float64, partner=b))
    _assert_bits(_read(b, MU, np.float32), mu_a, "mu of the partner")
    sa = _read(a, SCALE, np.float64)
    _assert_bits(_read(b, SCALE, np.float64), sa, "scale of the partner")
    check_h_image(a, xa, "euclidean", _read(a, SQN, np.float64), mu_a, float(sa[0]), _read(a, H, np.float16), _read(a, H_BIAS, np.float32),
                  _read(a, ROWQ, np.float64), _read(a, DMAX, np.float64))
    # a third matrix ensured against an A that already has an image gets A's (that is B's) centre, not its own
    _assert_bits(_read(c, MU, np.float32, partner=a), mu_a, "mu of the third matrix")
    check_h_image(c, xc, "euclidean", _read(c, SQN, np.float64), mu_a, float(sa[0]), _read(c, H, np.float16), _read(c, H_BIAS, np.float32),
                  _read(c, ROWQ, np.float64), _read(c, DMAX, np.float64))
    own = _matrix(xc, "euclidean")
    assert not np.array_equal(_read(own, MU, np.float32), mu_a)


# ---- regimes -------------------------------------------------------------------------------------------------------------------
REGIMES = ("normal", "clamp", "flush", "offset")


def _regime(name, n_q, n_i, d, dtype):
    """(query, index): the centre is taken from the index."""
    if name == "normal":
        q, y = V.base_pair(n_q, n_i, d, dtype, 71, "randn")
    elif name == "clamp":      # a partner 2^10 times larger than the matrix the centre came from: every row is clamped
        q, y = V.mismatch(10, "query", n_q, n_i, d, dtype, 72, "randn")
    elif name == "flush":      # S is clamped at 2^100: the largest elements land near 2^-8, everything under 2^-14 is flushed
        q, y = V.pow2(V.POW2_BELOW_THE_SCALE_CLAMP, n_q, n_i, d, dtype, 73, "randn")[1]
    else:
        q, y = V.offset(V.OFFSET_TIES, n_q, n_i, d, dtype, 74)
    q, y = q.copy(), y.copy()
    for x in (q, y):
        x[len(x) // 2] = 0.0
        x[1] = 0.0
        x[1, d - 1] = x[0, 0]
        x[len(x) - 1] = x[0]
    return q, y


def _regime_pair(name, dtype, metric):
    q, y = _regime(name, 256, 384, 300, dtype)
    qm, ym = _matrix(q, metric), _matrix(y, metric)
    sq, sy = _read(qm, SQN, np.float64), _read(ym, SQN, np.float64)
    Y = _own_image(ym, y, metric, sy, check_centre_of=(ym, y, metric, sy))
    Q = _own_image(qm, q, metric, sq, partner=ym)
    _assert_bits(Q[0], Y[0], "shared mu")
    assert Q[1] == Y[1]
    return Q, Y


@pytest.mark.parametrize("name,dtype", [(r, t) for r in REGIMES for t in DTYPES if not (r == "flush" and t == np.float32)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_fp16_image_regimes(name, dtype):
    Q, Y = _regime_pair(name, dtype, "euclidean")
    mu, S, v, h, rowq, dmax = Q[:6]
    live = np.abs(v) > 0
    if name == "clamp":
        assert (np.abs(h[live]) == np.float16(R.FP16_MAX)).mean() > 0.5          # the regime is what it says
        assert np.median(rowq[:, 2] / np.sqrt(rowq[:, 0])) > 0.5                 # ... and the clamped part is in the residual
    if name == "flush":
        assert S == 2.0 ** 100 and 0.01 < (h[live] == 0).mean() < 0.98
    if name == "offset":
        assert np.abs(mu[:300]).max() > 1e3 and dmax[1] < 2.0 ** -9 * np.sqrt(dmax[2])


@pytest.mark.parametrize("name", REGIMES)
def test_products_stay_inside_the_bound(name):
    """What the certification assumes of these buffers: for EVERY pair, the product of the fp16 operands is
    within rq Yh + qh Ry + rq Ry of the product of the centred rows -- rq, qh from the query's rowq, Yh, Ry from the index's d_max.
    (q_c = q_h + r_q, y_c = y_h + r_y, Cauchy-Schwarz on the three cross terms.)  The last term is numpy's own error on two float64
    dot products of d terms, each at most d 2^-53 |a| |b|."""
    dtype = np.float64
    for metric in METRICS:
        (mu, S, qv, qh16, q_rowq, _, _, _), (_, _, yv, yh16, y_rowq, y_dmax, _, _) = _regime_pair(name, dtype, metric)
        d = qv.shape[1]
        qc, yc = qv.astype(np.float64), yv.astype(np.float64)
        qh, yh = qh16.astype(np.float64) / S, yh16.astype(np.float64) / S      # decoded from what the image holds (checked bit for bit above)
        diff = np.abs(qh @ yh.T - qc @ yc.T)
        nq = np.maximum(np.sqrt(q_rowq[:, 0]), q_rowq[:, 1])
        ny = np.maximum(np.sqrt(y_rowq[:, 0]), y_rowq[:, 1])
        bound = (q_rowq[:, 2] * y_dmax[0] + q_rowq[:, 1] * y_dmax[1] + q_rowq[:, 2] * y_dmax[1])[:, None] + 4 * d * U * np.outer(nq, ny)
        assert (diff <= bound).all(), (metric, float((diff - bound).max()))
        if name != "normal":
            assert diff.max() > 0


# ---- variants ------------------------------------------------------------------------------------------------------------------
def _variant_setup(n, d, dtype, metric):
    x = _rows(n, d, dtype)
    m = _matrix(x, metric)
    sqn = _read(m, SQN, np.float64)
    mu, S, v, h, rowq, dmax, packed, bias = _own_image(m, x, metric, sqn)
    return x, m, sqn, mu, S, packed, bias


def _check_dealt(x, m, metric, sqn, mu, S, own_packed, own_bias, P):
    n, d = x.shape
    nsr = R.h_nsr(R.kg(d))
    npad = R.n_pad(n)
    _poison(npad * nsr * 32 + 32 * 4096, npad * 4, npad * 4)
    perm = _read(m, DEALT_PERM, np.int32, arg=P)
    _assert_bits(perm, R.dealt_perm(n, P), f"perm of P={P}")
    packed, bias = _read(m, DEALT_H, np.float16, arg=P), _read(m, DEALT_BIAS, np.float32, arg=P)
    check_h_image(m, x, metric, sqn, mu, S, packed, bias, perm=perm[:n])
    # image row r and its bias: bit for bit the own image's row perm[r]
    row, k = R.grid(n, 16 * nsr)
    _assert_bits(packed[R.h_offset(row, k, nsr)], own_packed[R.h_offset(perm[:n, None].astype(np.int64), k, nsr)], "dealt rows")
    _assert_bits(bias[:n], own_bias[perm[:n]], "dealt bias")


@pytest.mark.parametrize("dtype,metric", [(np.float32, "euclidean"), (np.float64, "cosine")], ids=["float32-euclidean", "float64-cosine"])
def test_dealt_images(dtype, metric):
    x, m, sqn, mu, S, packed, bias = _variant_setup(1000, 20, dtype, metric)
    for P in (2, 3, 7, 1000):
        _check_dealt(x, m, metric, sqn, mu, S, packed, bias, P)
    # two slots: 5 evicts the slot not selected last (2), the second 2 evicts 3
    for P in (2, 3, 5, 2):
        _check_dealt(x, m, metric, sqn, mu, S, packed, bias, P)
    N, ctx = _native()
    with pytest.raises(ValueError, match="dealt ranges"):
        _read(m, DEALT_PERM, np.int32, arg=1001)


def test_dealt_image_past_one_grid_trip():
    x, m, sqn, mu, S, packed, bias = _variant_setup(65541, 20, np.float32, "euclidean")
    _check_dealt(x, m, "euclidean", sqn, mu, S, packed, bias, 3)


@pytest.mark.parametrize("dtype,metric", [(np.float32, "cosine"), (np.float64, "euclidean")], ids=["float32-cosine", "float64-euclidean"])
def test_row_list_image(dtype, metric):
    x, m, sqn, mu, S, own_packed, own_bias = _variant_setup(1000, 33, dtype, metric)
    n, d = x.shape
    nsr = R.h_nsr(R.kg(d))
    rows = np.random.RandomState(9).randint(0, n, size=300).astype(np.int32)
    rows[:4] = [999, 0, 999, 500]                 # repeats, the last row, the zero row
    _poison(384 * nsr * 32 + 32 * 4096, 384 * 4)
    packed, bias = _read(m, ROWS_H, np.float16, arg=300, rows=rows), _read(m, ROWS_BIAS, np.float32, arg=300, rows=rows)
    assert packed.size == 384 * nsr * 16 and bias.size == 384
    check_h_image(m, x, metric, sqn, mu, S, packed, bias, perm=rows)
    row, k = R.grid(300, 16 * nsr)
    _assert_bits(packed[R.h_offset(row, k, nsr)], own_packed[R.h_offset(rows[:, None].astype(np.int64), k, nsr)], "listed rows")
    _assert_bits(bias[:300], own_bias[rows], "listed bias")
    row, k = R.grid(384, 16 * nsr)
    assert (packed[R.h_offset(row, k, nsr)][300:].view(np.uint16) == 0).all() and (bias[300:] == -np.inf).all()
    with pytest.raises(ValueError, match="no matrix row"):
        _read(m, ROWS_BIAS, np.float32, arg=2, rows=np.array([0, n], dtype=np.int32))
