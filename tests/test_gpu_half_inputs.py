"""float16 / bfloat16 rows read in place (KZ_F16, KZ_BF16): a matrix of 2-byte rows behaves like the KZ_F64 matrix that holds the same
values widened exactly -- the same neighbour indices, the same distance BITS, float64 outputs, the same errors.

Inputs: drawn in float32 and rounded to the half type (tests/half_inputs.py), so every value is representable.  First oracle: the
same call on KZ_F64 matrices of the widened values (the route the goldens pin), compared with np.array_equal on indices and
distance bits.  Second oracle: oracle.kiez_oracle on the float64 values -- distances everywhere; indices only at d >= 30 on data
checked to have no duplicated rows (half grids make exact ties common, and scikit-learn's tie order is implementation-defined).
Tolerance of the second oracle: both sides are float64 evaluations of |x|^2 - 2 x.y + |y|^2 (or of the normalised dot product) in
different summation orders; the round-off of either is below (d + 3) 2^-53 (|x|^2 + |y|^2) <= 2103 x 1.1e-16 x 2 x 2100 x 1.5 < 1.5e-9
on a squared distance of order 2 d at the widest case, i.e. relative 1e-12; rtol = 1e-9 with atol = 1e-9 leaves three orders.

Routes (asserted from kz_knn_stats): fp16 first pass, split-bf16 first pass (option precision = 2), float32 operands (precision =
1, and d = 400), every row through the exact kernels (eps_scale huge: n_fallback_rows == q_count), tight clusters that send
rows down the tiers, the shared sweep (dual_force), and the long-k route (k = 200: the finalize build for many candidates).  Every case that sets a context option puts it back in a `finally`: the context is shared with the suite.
`pytest -m gpu`."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import half_inputs as H

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

METRICS = ("euclidean", "sqeuclidean", "cosine")
N_Q, N_I = 300, 700
# 1, 5: the scalar path, a pitch that is not 8-byte aligned, heavy ties (grid data); 32, 200: the vector path; 260: the second trip of
# the 256-element lane loop; 400: the float32-operand widths 385 .. 496; 768, 1536: the wide and parity-split builds; 2100: beyond
WIDTHS = (1, 5, 30, 32, 200, 260, 300, 400, 768, 1536, 2100)
KS = (1, 10, 40)
OPTION_DEFAULTS = {"precision": 0, "eps_scale": 1.0, "dual_force": 0}


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    try:
        yield c
    finally:
        for name, value in OPTION_DEFAULTS.items():
            c.set_option(name, value)


def _half_matrix(ctx, dev_rows, elem, metric):
    from kiez_amd import _native as N
    return N.DeviceMatrix(ctx, dev_rows, metric, elem="bfloat16" if elem == "bfloat16" else None)


def _pair(n_q, n_i, d, elem, seed, kind="normal"):
    q_dev, q64 = H.draw(n_q, d, elem, seed, kind)
    y_dev, y64 = H.draw(n_i, d, elem, seed + 1000, kind)
    return q_dev, q64, y_dev, y64


def _knn_both(ctx, q_dev, q64, y_dev, y64, elem, metric, k, single=False, options=None):
    """(dist, ind, stats) of the half route and of the KZ_F64 route, under `options` (put back afterwards)."""
    from kiez_amd import _native as N
    try:
        for name, value in (options or {}).items():
            ctx.set_option(name, value)
        out = []
        for y, q, half in ((y_dev, q_dev, True), (y64, q64, False)):
            ym = _half_matrix(ctx, y, elem, metric) if half else N.DeviceMatrix(ctx, y, metric)
            qm = ym if single else (_half_matrix(ctx, q, elem, metric) if half else N.DeviceMatrix(ctx, q, metric))
            assert ym.elem == (elem if half else "float64")
            dd, ii, st = N.knn(ctx, qm, ym, k, exclude_self=single)
            out.append((dd.numpy(), ii.numpy(), st))
    finally:
        for name in (options or {}):
            ctx.set_option(name, OPTION_DEFAULTS[name])
    return out


def _assert_same_bits(half, wide, what):
    assert half[0].dtype == np.float64 and half[1].dtype == np.int64, what
    bad = (half[1] != wide[1]).any(axis=1).sum()
    assert bad == 0, f"{what}: indices differ from the KZ_F64 route in {bad} rows"
    assert np.array_equal(half[0].view(np.uint64), wide[0].view(np.uint64)), f"{what}: distance bits differ from the KZ_F64 route"
    assert half[2]["first_pass"] == wide[2]["first_pass"], f"{what}: the half route started on another tier"


def _assert_oracle(half, q64, y64, k, metric, d, what, single=False):
    from oracle import kiez_oracle as O
    od, oi = O.knn_exact(q64, y64, k, metric, exclude_self=single)
    np.testing.assert_allclose(half[0], od, rtol=1e-9, atol=1e-9, err_msg=what)
    if d >= 30:
        assert not H.has_duplicate_rows(y64), f"{what}: the drawn index has duplicated rows"
        np.testing.assert_array_equal(half[1], oi, err_msg=what)


def _parity_cases():
    """The grid thinned: every width with both half types; metric and k cycle so that every (type, metric) and every k occurs."""
    cases = []
    for wi, d in enumerate(WIDTHS):
        for ei, elem in enumerate(H.HALF_ELEMS):
            cases.append((elem, METRICS[(wi + ei) % 3], KS[(wi + 2 * ei) % 3], d))
    return cases


@pytest.mark.parametrize("elem,metric,k,d", _parity_cases(), ids=lambda v: str(v))
def test_native_parity(ctx, elem, metric, k, d):
    q_dev, q64, y_dev, y64 = _pair(N_Q, N_I, d, elem, 7 * d, "grid" if d < 30 else "normal")
    half, wide = _knn_both(ctx, q_dev, q64, y_dev, y64, elem, metric, k)
    what = f"{elem} {metric} k={k} d={d}"
    print(what, "first_pass", half[2]["first_pass"], "escalated", half[2]["n_escalated_rows"], "fallback", half[2]["n_fallback_rows"])
    _assert_same_bits(half, wide, what)
    _assert_oracle(half, q64, y64, k, metric, d, what)
    if d in (32, 200, 260, 300, 768, 1536):
        assert half[2]["first_pass"] == 2, f"{what}: the fp16 first pass did not run"
    if d in (400, 2100):
        assert half[2]["first_pass"] == 0, f"{what}: float32 operands expected at this width"


@pytest.mark.parametrize("elem", H.HALF_ELEMS)
def test_native_parity_exclude_self_on_one_matrix(ctx, elem):
    y_dev, y64 = H.draw(N_I, 32, elem, 3)
    half, wide = _knn_both(ctx, y_dev, y64, y_dev, y64, elem, "euclidean", 10, single=True)
    _assert_same_bits(half, wide, f"{elem} single")
    _assert_oracle(half, y64, y64, 10, "euclidean", 32, f"{elem} single", single=True)
    assert (half[1] != np.arange(N_I)[:, None]).all()


@pytest.mark.parametrize("elem,metric,d,options,first_pass", [
    ("float16", "euclidean", 200, {"precision": 2}, 1), ("bfloat16", "cosine", 32, {"precision": 2}, 1),
    ("bfloat16", "sqeuclidean", 200, {"precision": 1}, 0), ("float16", "cosine", 260, {"precision": 1}, 0),
])
def test_routes_split_bf16_and_float32_operands(ctx, elem, metric, d, options, first_pass):
    q_dev, q64, y_dev, y64 = _pair(N_Q, N_I, d, elem, d)
    half, wide = _knn_both(ctx, q_dev, q64, y_dev, y64, elem, metric, 10, options=options)
    _assert_same_bits(half, wide, f"{elem} {metric} d={d} {options}")
    assert half[2]["first_pass"] == first_pass, half[2]
    _assert_oracle(half, q64, y64, 10, metric, d, f"{elem} {metric} d={d} {options}")


@pytest.mark.parametrize("elem,metric,d", [("float16", "euclidean", 33), ("bfloat16", "cosine", 260), ("float16", "sqeuclidean", 768),
                                           ("bfloat16", "euclidean", 5)])
def test_route_every_row_through_the_exact_kernels(ctx, elem, metric, d):
    """An inflated rounding bound: no tier certifies a row.  (d = 33, 5: rows of an odd width are gathered for the re-search 2 bytes
    at a time.)"""
    q_dev, q64, y_dev, y64 = _pair(N_Q, N_I, d, elem, 11 * d, "grid" if d < 30 else "normal")
    half, wide = _knn_both(ctx, q_dev, q64, y_dev, y64, elem, metric, 10, options={"eps_scale": 1e30})
    _assert_same_bits(half, wide, f"{elem} {metric} d={d} exact")
    assert half[2]["n_fallback_rows"] == N_Q, half[2]
    _assert_oracle(half, q64, y64, 10, metric, d, f"{elem} {metric} d={d} exact")


@pytest.mark.parametrize("elem", H.HALF_ELEMS)
def test_route_tight_clusters_go_down_the_tiers(ctx, elem):
    """Clusters three orders of magnitude tighter than their distance from the centre (the `cliff` kind): rows the fp16 tier cannot
    certify are escalated.  Rounded to a half type such rows collide: the KZ_F64 route is the oracle, ties by the smaller index."""
    q_dev, q64, y_dev, y64 = _pair(400, 900, 32, elem, 21, "tight")
    half, wide = _knn_both(ctx, q_dev, q64, y_dev, y64, elem, "sqeuclidean", 10)
    print(elem, {k: half[2][k] for k in ("first_pass", "n_first_pass_fail", "n_escalated_rows", "n_fallback_rows")})
    _assert_same_bits(half, wide, f"{elem} tight")
    assert half[2]["first_pass"] == 2
    assert half[2]["n_first_pass_fail"] > 0 and half[2]["n_escalated_rows"] + half[2]["n_fallback_rows"] > 0, half[2]
    assert half[2]["n_escalated_rows"] == wide[2]["n_escalated_rows"] and half[2]["n_fallback_rows"] == wide[2]["n_fallback_rows"]
    # (distances only -- rounded rows collide; squared distances: a collided pair is exactly 0 here and within round-off of 0 there)
    _assert_oracle(half, q64, y64, 10, "sqeuclidean", 1, f"{elem} tight")


@pytest.mark.parametrize("elem,metric", [("float16", "euclidean"), ("bfloat16", "cosine")])
def test_shared_sweep_both_directions(ctx, elem, metric):
    """kz_knn_dual (forced onto a shape where the cost model would search twice): both directions, the KZ_F64 bits."""
    from kiez_amd import _native as N
    a_dev, a64, b_dev, b64 = _pair(1500, 2000, 64, elem, 17)
    try:
        ctx.set_option("dual_force", 1)
        res = []
        for a, b, half in ((a_dev, b_dev, True), (a64, b64, False)):
            am = _half_matrix(ctx, a, elem, metric) if half else N.DeviceMatrix(ctx, a, metric)
            bm = _half_matrix(ctx, b, elem, metric) if half else N.DeviceMatrix(ctx, b, metric)
            (d_ab, i_ab, s_ab), (d_ba, i_ba, s_ba) = N.knn_dual(ctx, am, bm, 10)
            res.append(((d_ab.numpy(), i_ab.numpy(), s_ab), (d_ba.numpy(), i_ba.numpy(), s_ba)))
    finally:
        ctx.set_option("dual_force", 0)
    for direction in (0, 1):
        _assert_same_bits(res[0][direction], res[1][direction], f"{elem} {metric} shared sweep direction {direction}")
    assert res[0][0][2]["dual"] == 1, res[0][0][2]
    _assert_oracle(res[0][0], a64, b64, 10, metric, 64, f"{elem} {metric} shared sweep a -> b")
    _assert_oracle(res[0][1], b64, a64, 10, metric, 64, f"{elem} {metric} shared sweep b -> a")


@pytest.mark.parametrize("elem,metric,d", [("float16", "euclidean", 32), ("bfloat16", "cosine", 300)])
def test_route_long_k_finalize_builds(ctx, elem, metric, d):
    """200 neighbours: lists of 128 over several index ranges, more than 160 selected candidates per query -- the finalize build for
    many candidates (four candidate rows per step) on half rows; d = 32 through its pipelined re-rank, d = 300 through its generic loop."""
    q_dev, q64, y_dev, y64 = _pair(N_Q, 20000, d, elem, 3 * d)
    half, wide = _knn_both(ctx, q_dev, q64, y_dev, y64, elem, metric, 200)
    st = half[2]
    print(elem, metric, d, {k: st[k] for k in ("first_pass", "list_len", "n_splits", "n_fallback_rows", "max_err_ratio")})
    _assert_same_bits(half, wide, f"{elem} {metric} d={d} k=200")
    assert st["first_pass"] == 2 and st["list_len"] == 128 and st["n_splits"] >= 4, st          # the long-k route of the fused kernels
    assert st["n_fallback_rows"] < N_Q // 10 and 0.0 < st["max_err_ratio"] < 1.0, st            # ... whose finalize kernel re-ranked the rows
    _assert_oracle(half, q64, y64, 200, metric, d, f"{elem} {metric} d={d} k=200")


# ---- 2. alignment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", H.HALF_ELEMS)
@pytest.mark.parametrize("d,options", [(5, None), (33, None), (33, {"eps_scale": 1e30}), (34, None), (36, None)])
def test_alignment_borrowed_rows_slice_and_copy(ctx, elem, d, options):
    """Borrowed device rows of an odd width; a row slice that starts one row in (odd d: the base is 2-byte aligned only); the aligned
    copy of the same rows; host rows.  The same bits from all of them."""
    from kiez_amd import _native as N
    y_dev, y64 = H.draw(N_I + 1, d, elem, 5 * d, "grid" if d < 30 else "normal")
    q_dev, q64 = H.draw(N_Q + 1, d, elem, 5 * d + 1, "grid" if d < 30 else "normal")
    kw = {"elem": "bfloat16"} if elem == "bfloat16" else {}
    try:
        for name, value in (options or {}).items():
            ctx.set_option(name, value)
        got = {}
        y_big, q_big = ctx.to_device(y_dev), ctx.to_device(q_dev)
        y_cp, q_cp = ctx.to_device(y_dev[1:]), ctx.to_device(q_dev[1:])
        for name, ya, qa in (("slice", y_big.view_rows(1, N_I), q_big.view_rows(1, N_Q)), ("copy", y_cp, q_cp)):
            if name == "slice" and d % 2:
                assert ya.ptr.value % 4 == 2        # (allocations are at least 4-byte aligned: one odd row in is 2-byte aligned only)
            ym = N.DeviceMatrix(ctx, None, "euclidean", device_ptr=ya.ptr.value, shape=ya.shape, dtype=ya.dtype, borrow=True, keepalive=ya, **kw)
            qm = N.DeviceMatrix(ctx, None, "euclidean", device_ptr=qa.ptr.value, shape=qa.shape, dtype=qa.dtype, borrow=True, keepalive=qa, **kw)
            assert ym.elem == elem
            dd, ii, st = N.knn(ctx, qm, ym, 10)
            got[name] = (dd.numpy(), ii.numpy(), st)
        ym, qm = _half_matrix(ctx, y_dev[1:], elem, "euclidean"), _half_matrix(ctx, q_dev[1:], elem, "euclidean")
        dd, ii, st = N.knn(ctx, qm, ym, 10)
        got["host"] = (dd.numpy(), ii.numpy(), st)
        ym, qm = N.DeviceMatrix(ctx, y64[1:], "euclidean"), N.DeviceMatrix(ctx, q64[1:], "euclidean")
        dd, ii, st = N.knn(ctx, qm, ym, 10)
        wide = (dd.numpy(), ii.numpy(), st)
    finally:
        for name in (options or {}):
            ctx.set_option(name, OPTION_DEFAULTS[name])
    for name in ("slice", "copy", "host"):
        _assert_same_bits(got[name], wide, f"{elem} d={d} {name}")
    if options:
        assert got["slice"][2]["n_fallback_rows"] == N_Q


# ---- 3. values -------------------------------------------------------------------------------------------------------------------
def _special_f16(d):
    rng = np.random.default_rng(d)
    y = rng.standard_normal((200, d)).astype(np.float16)
    y[0] = 0.0                                               # an all-zero row (cosine: sklearn's normalize leaves it zero)
    y[1] = np.float16(-0.0)
    y[2] = np.float16(65504.0)
    y[3] = np.float16(-65504.0)
    y[4, ::2] = np.float16(65504.0)
    y[5] = (rng.integers(1, 1024, d).astype(np.uint16)).view(np.float16)          # fp16 subnormals (exponent field 0)
    y[6] = (rng.integers(1, 1024, d).astype(np.uint16) | 0x8000).view(np.float16)
    y[7] = y[5]
    y[8, : d // 2] = np.float16(-0.0)
    return y


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [7, 64])
def test_values_fp16_subnormals_extremes_and_zero_rows(ctx, metric, d):
    y = _special_f16(d)
    q = np.ascontiguousarray(y[::-1][:120])
    assert (np.abs(y[5].astype(np.float64)) < 6.2e-5).all() and (y[5] != 0).all()
    y64, q64 = y.astype(np.float64), q.astype(np.float64)
    half, wide = _knn_both(ctx, q, q64, y, y64, "float16", metric, 10)
    _assert_same_bits(half, wide, f"special values {metric} d={d}")
    assert np.isfinite(half[0]).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("e", [-40, -10, 20, 40])
def test_values_bf16_at_the_scales_of_the_value_regimes(ctx, metric, e):
    """tests/value_regimes.py's power-of-two scales that fit under the input limit |x|^2 <= 1e30: a power of two moves the exponent of
    a bfloat16 value and nothing else, so the scaled rows are representable."""
    q_dev, q64, y_dev, y64 = _pair(200, 500, 64, "bfloat16", 64 + e)
    s = 2.0 ** e
    q_s, y_s = H.bf16_bits((q64 * s).astype(np.float32)), H.bf16_bits((y64 * s).astype(np.float32))
    np.testing.assert_array_equal(H.bf16_widen(q_s), q64 * s)
    half, wide = _knn_both(ctx, q_s, q64 * s, y_s, y64 * s, "bfloat16", metric, 10)
    _assert_same_bits(half, wide, f"bf16 scale 2^{e} {metric}")
    _assert_oracle(half, q64 * s, y64 * s, 10, metric, 64, f"bf16 scale 2^{e} {metric}")


def _bad_rows(which):
    """(device rows, elem) with one offending value: fp16 inf, fp16 NaN, a bfloat16 row of magnitude 1e16 (|x|^2 > 1e30)."""
    if which == "bf16_1e16":
        b, _ = H.draw(64, 32, "bfloat16", 1)
        b[3, :] = H.bf16_bits(np.full(32, 1e16, dtype=np.float32))
        return b, "bfloat16"
    h, _ = H.draw(64, 32, "float16", 1)
    h[3, 2] = np.float16(np.inf) if which == "f16_inf" else np.float16(np.nan)
    return h, "float16"


@pytest.mark.parametrize("which", ["f16_inf", "f16_nan", "bf16_1e16"])
def test_values_non_finite_rows_give_the_present_errors(ctx, which):
    from kiez_amd import _native as N
    rows, elem = _bad_rows(which)
    with pytest.raises(ValueError, match="NaN, infinity or a row with"):       # host rows: refused by kz_matrix_create (KZ_ERR_NONFINITE)
        _half_matrix(ctx, rows, elem, "euclidean")
    dev = ctx.to_device(rows)                                                   # device rows: by the first search
    kw = {"elem": "bfloat16"} if elem == "bfloat16" else {}
    m = N.DeviceMatrix(ctx, None, "euclidean", device_ptr=dev.ptr.value, shape=dev.shape, dtype=dev.dtype, borrow=True, keepalive=dev, **kw)
    with pytest.raises(ValueError, match="NaN, infinity or a row with"):
        N.knn(ctx, m, m, 5)


# ---- 4. refusals and the dispatch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", H.HALF_ELEMS)
@pytest.mark.parametrize("metric", ["manhattan", "chebyshev", "minkowski[3.0]", "braycurtis", "seuclidean", "correlation", "hamming",
                                    "jaccard", "yule"])
def test_create_refuses_half_rows_for_every_other_metric(ctx, elem, metric):
    import ctypes as C
    from kiez_amd import _native as N
    rows, _ = H.draw(16, 8, elem, 0)
    h = C.c_void_p()
    mid = N.METRIC_IDS[N.split_metric(metric)[0]]
    dev = ctx.to_device(rows)
    for mode, ptr in ((0, rows.ctypes.data_as(C.c_void_p)), (2, dev.ptr), (3, dev.ptr)):
        rc = ctx.lib.kz_matrix_create(ctx.handle, ptr, mode, 16, 8, N.ELEM_CODES[elem], mid, C.byref(h))
        msg = ctx.lib.kz_last_error().decode()
        assert rc == 3 and not h.value, (rc, msg)           # KZ_ERR_UNSUPPORTED, nothing created
        assert f"metric {mid}" in msg and ("KZ_F16" if elem == "float16" else "KZ_BF16") in msg, msg
    with pytest.raises(NotImplementedError):
        N.DeviceMatrix(ctx, rows, metric, elem=elem)


def test_precomputed_and_unknown_types_are_refused(ctx):
    import ctypes as C
    from kiez_amd import _native as N
    vals = np.ones((8, 8), dtype=np.float16)
    a, b = C.c_void_p(), C.c_void_p()
    for code in (N.KZ_F16, N.KZ_BF16):
        rc = ctx.lib.kz_matrix_create_precomputed(ctx.handle, vals.ctypes.data_as(C.c_void_p), 0, 8, 8, code, C.byref(a), C.byref(b))
        assert rc == 1 and not a.value and not b.value, rc
    h = C.c_void_p()
    for code in (4, -1, 17):
        rc = ctx.lib.kz_matrix_create(ctx.handle, vals.ctypes.data_as(C.c_void_p), 0, 8, 8, code, N.KZ_EUCLIDEAN, C.byref(h))
        assert rc == 1 and not h.value, (code, rc)
    with pytest.raises(ValueError):
        N.DeviceMatrix.precomputed(ctx, None, device_ptr=ctx.to_device(vals).ptr.value, shape=(8, 8), dtype=np.float16)


def test_shape_reports_the_type_and_mixed_types_keep_the_same_dtype_error(ctx):
    import ctypes as C
    from kiez_amd import _native as N
    for elem in H.HALF_ELEMS:
        rows, w64 = H.draw(40, 32, elem, 2)
        hm = _half_matrix(ctx, rows, elem, "euclidean")
        n, d, dt, me = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        N._check(ctx.lib.kz_matrix_shape(hm.handle, C.byref(n), C.byref(d), C.byref(dt), C.byref(me)))
        assert (n.value, d.value, dt.value, me.value) == (40, 32, N.ELEM_CODES[elem], N.KZ_EUCLIDEAN)
        for other in (N.DeviceMatrix(ctx, w64.astype(np.float32), "euclidean"), N.DeviceMatrix(ctx, w64, "euclidean")):
            with pytest.raises(ValueError, match="same dtype"):
                N.knn(ctx, hm, other, 5)
            with pytest.raises(ValueError, match="same dtype"):
                N.knn(ctx, other, hm, 5)
    f, _ = H.draw(40, 32, "float16", 2)
    b, _ = H.draw(40, 32, "bfloat16", 2)
    with pytest.raises(ValueError, match="same dtype"):
        N.knn(ctx, _half_matrix(ctx, f, "float16", "euclidean"), _half_matrix(ctx, b, "bfloat16", "euclidean"), 5)


def test_rows_only_source_and_pair_values(ctx):
    """rows_on_device = 3 (a row source for kz_dsl_fit) and kz_pair_values on half rows: the KZ_F64 values."""
    from kiez_amd import _native as N
    for elem in H.HALF_ELEMS:
        q_dev, q64, y_dev, y64 = _pair(64, 90, 33, elem, 9)
        kw = {"elem": "bfloat16"} if elem == "bfloat16" else {}
        ind = np.random.default_rng(0).integers(0, 90, (64, 6)).astype(np.int64)
        ind_d = ctx.to_device(ind)
        vals = []
        for q, y in ((q_dev, y_dev), (q64, y64)):
            qm = N.DeviceMatrix(ctx, q, "euclidean", **(kw if q is q_dev else {}))
            ym = N.DeviceMatrix(ctx, y, "euclidean", **(kw if q is q_dev else {}))
            out = ctx.empty((64, 6), np.float64)
            N._check(ctx.lib.kz_pair_values(ctx.handle, qm.handle, 0, 64, ym.handle, ind_d.ptr, 6, out.ptr))
            src = ctx.to_device(q)
            sm = N.DeviceMatrix(ctx, None, "euclidean", device_ptr=src.ptr.value, shape=src.shape, dtype=src.dtype, borrow=True, keepalive=src,
                                rows_only=True, **(kw if q is q_dev else {}))
            t2c = ctx.empty((90,), np.float64)
            tind = ctx.to_device(np.random.default_rng(1).integers(0, 64, (90, 4)).astype(np.int64))
            N._check(ctx.lib.kz_dsl_fit(ctx.handle, tind.ptr, 90, 4, sm.handle, ym.handle, 0, t2c.ptr))
            vals.append((out.numpy(), t2c.numpy()))
        assert np.array_equal(vals[0][0].view(np.uint64), vals[1][0].view(np.uint64)), elem
        assert np.array_equal(vals[0][1].view(np.uint64), vals[1][1].view(np.uint64)), elem


# ---- 5. through Kiez -------------------------------------------------------------------------------------------------------------
SHAPES = ((500, 400, 32), (300, 300, 300))
HUBNESS = [(None, {}), ("CSLS", {}), ("LocalScaling", {"method": "standard"}), ("LocalScaling", {"method": "nicdm"}),
           ("MutualProximity", {"method": "normal"}), ("MutualProximity", {"method": "empiric"}), ("DisSimLocal", {})]


@pytest.fixture(scope="module")
def kiez_data():
    out = {}
    for n_s, n_t, d in SHAPES:
        s16, s64 = H.draw(n_s, d, "float16", d)
        t16, t64 = H.draw(n_t, d, "float16", d + 1)
        gold = np.random.default_rng(d).integers(0, n_t, n_s).astype(np.int64)
        for a in (s16, s64, t16, t64, gold):
            a.setflags(write=False)
        out[(n_s, n_t, d)] = (s16, s64, t16, t64, gold)
    return out


def _kiez(hubness, kwargs, metric="euclidean"):
    from kiez_amd import Kiez
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=dict(kwargs))


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("hubness,kwargs", HUBNESS, ids=lambda v: str(v))
def test_kiez_float16_equals_the_float64_copies(kiez_data, shape, hubness, kwargs):
    import warnings
    s16, s64, t16, t64, gold = kiez_data[shape]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kh, kw = _kiez(hubness, kwargs).fit(s16, t16), _kiez(hubness, kwargs).fit(s64, t64)
        # nothing was widened  (no hubness reduction: only the target side is indexed, the source rows go up with the first search)
        assert kh.algorithm.target_index.elem == "float16" and getattr(kh.algorithm, "source_index", kh.algorithm.target_index).elem == "float16"
        assert kw.algorithm.target_index.elem == "float64"
        dh, ih = kh.kneighbors(5)
        dw, iw = kw.kneighbors(5)
        _same(ih, iw, f"{hubness} {kwargs} indices")
        _same(dh, dw, f"{hubness} {kwargs} distances")
        assert dh.dtype == np.float64
        _same(kh.gold_ranks(gold), kw.gold_ranks(gold), "gold_ranks")
        if hubness not in ("DisSimLocal",) and kwargs.get("method") != "empiric":
            _same(kh.gold_ranks(gold, reduced=True), kw.gold_ranks(gold, reduced=True), "gold_ranks reduced")
            for a, b in zip(kh.kneighbors_whole_index(10), kw.kneighbors_whole_index(10)):
                _same(a, b, "kneighbors_whole_index")
        for a, b in zip(kh.match(10), kw.match(10)):
            _same(a, b, "match")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kiez_sinkhorn_fit_and_cosine(kiez_data, shape):
    import warnings
    from kiez_amd import Sinkhorn
    s16, s64, t16, t64, gold = kiez_data[shape]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kh = _kiez(Sinkhorn, {"temperature": 0.05, "n_iter": 3}, "cosine").fit(s16, t16)
        kw = _kiez(Sinkhorn, {"temperature": 0.05, "n_iter": 3}, "cosine").fit(s64, t64)
        assert kh.algorithm.target_index.elem == "float16"
        _same(kh.hubness.source_potential_, kw.hubness.source_potential_, "f")
        _same(kh.hubness.target_potential_, kw.hubness.target_potential_, "g")
        for a, b in zip(kh.kneighbors(5), kw.kneighbors(5)):
            _same(a, b, "sinkhorn kneighbors")          # (cosine too: float64 out -- float32 is for float32 inputs only)
        for a, b in zip(kh.kneighbors_whole_index(10), kw.kneighbors_whole_index(10)):
            _same(a, b, "sinkhorn whole index")


def test_kiez_ad_hoc_query_of_another_type_runs_on_the_float64_pair(kiez_data):
    """A float32 `query=` against a float16 index: the index side is widened once, the search runs on the float64 pair; the same
    half type is searched in place; the next fit drops the widened copy."""
    from kiez_amd.neighbors import SklearnNN
    s16, s64, t16, t64, _ = kiez_data[SHAPES[0]]
    q32 = np.random.default_rng(4).standard_normal((50, 32)).astype(np.float32)
    nn_h, nn_w = SklearnNN(n_candidates=10, metric="euclidean"), SklearnNN(n_candidates=10, metric="euclidean")
    nn_h.fit(s16, t16)
    nn_w.fit(s64, t64)
    for a, b in zip(nn_h.kneighbors(5, query=q32), nn_w.kneighbors(5, query=q32.astype(np.float64))):
        _same(a, b, "float32 query")
    assert len(nn_h._wide) == 1 and nn_h.target_index.elem == "float16"
    wide = next(iter(nn_h._wide.values()))[1]
    assert wide.elem == "float64"
    for a, b in zip(nn_h.kneighbors(5, query=q32), nn_w.kneighbors(5, query=q32.astype(np.float64))):
        _same(a, b, "float32 query again")
    assert next(iter(nn_h._wide.values()))[1] is wide                                   # widened once
    q16 = q32.astype(np.float16)
    for a, b in zip(nn_h.kneighbors(5, query=q16), nn_w.kneighbors(5, query=q16.astype(np.float64))):
        _same(a, b, "float16 query")
    assert nn_h._aux[1].elem == "float16"
    dq = nn_h.ctx.to_device(q16)                                                        # a float16 DeviceArray: a borrowed input
    for a, b in zip(nn_h.kneighbors(5, query=dq), nn_w.kneighbors(5, query=q16.astype(np.float64))):
        _same(a, b, "float16 DeviceArray query")
    nn_h.fit(dq, nn_h.ctx.to_device(t16))
    assert nn_h._wide == {} and nn_h.source_index.elem == "float16"
    for a, b in zip(nn_h.kneighbors(5), nn_w.kneighbors(5, query=q16.astype(np.float64))):
        _same(a, b, "fit on float16 DeviceArrays")
    # two DeviceArrays of different element types, one of them float16: the half side is widened to float64 (both sides of a search
    # have one type), whatever the hubness reduction asks of the pair
    from kiez_amd import Kiez
    for hub in (None, "CSLS"):
        kz_m = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub)
        kz_w = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub)
        kz_m.fit(nn_h.ctx.to_device(s16), nn_h.ctx.to_device(t64))
        kz_w.fit(s64, t64)
        assert kz_m.algorithm.target_index.elem == "float64" and getattr(kz_m.algorithm, "source_index", kz_m.algorithm.target_index).elem == "float64"
        for a, b in zip(kz_m.kneighbors(5), kz_w.kneighbors(5)):
            _same(a, b, f"float16 + float64 DeviceArrays {hub}")
    # other metrics keep widening on the host
    nn_m = SklearnNN(n_candidates=10, metric="manhattan")
    nn_m.fit(s16, t16)
    assert nn_m.target_index.elem == "float64"
    with pytest.raises(ValueError, match="device inputs must be 2D float32/float64 arrays"):
        nn_m.fit(dq)


# ---- 6. torch (a subprocess: torch must be imported before the library is loaded) -------------------------------------------------
TORCH_SCRIPT = r"""
import sys, warnings
sys.path.insert(0, %r)
import torch
import numpy as np
from kiez_amd import Kiez
warnings.simplefilter("ignore")
g = torch.Generator().manual_seed(0)
s32, t32 = torch.randn(500, 32, generator=g), torch.randn(400, 32, generator=g)
def kiez(hub):
    return Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=hub)
for dt in (torch.float16, torch.bfloat16):
    sh, th = s32.to(dt), t32.to(dt)
    for hub in (None, "CSLS", "DisSimLocal"):
        want_d, want_i = kiez(hub).fit(sh.to(torch.float64).to("cuda"), th.to(torch.float64).to("cuda")).kneighbors(5)
        for dev in ("cuda", "cpu"):
            st, tt = sh.to(dev), th.to(dev)
            k = kiez(hub).fit(st, tt)
            nn = k.algorithm
            want = str(dt).replace("torch.", "")
            sides = [(nn.target_index, tt)] + ([(nn.source_index, st)] if hasattr(nn, "source_index") else [])
            for m, t in sides:
                assert m.elem == want, (m.elem, want)
                assert dev != "cuda" or m.rows_ptr == t.data_ptr()     # CUDA tensors: borrowed, read in place
            d, i = k.kneighbors(5)
            assert nn._matrix_for(st).elem == want and (dev != "cuda" or nn._matrix_for(st).rows_ptr == st.data_ptr())
            assert isinstance(d, torch.Tensor) and d.dtype == torch.float64 and i.dtype == torch.int64 and d.device.type == dev
            assert torch.equal(i.cpu(), want_i.cpu()), (dt, hub, dev)
            assert torch.equal(d.cpu(), want_d.cpu()), (dt, hub, dev)
    # two tensors of different element types, one of them half: both sides of a search have one type -- the half side is widened to
    # float64 (two half types: both), and every direction a reduction asks for gives what the float64 pair gives
    s64, t64 = sh.to(torch.float64), th.to(torch.float64)
    for pair in ((sh, t64), (s64, th), (sh, t32.to(torch.bfloat16 if dt == torch.float16 else torch.float16))):
        tw = pair[1].to(torch.float64)
        for hub in (None, "CSLS", "MutualProximity", "DisSimLocal"):
            for dev in ("cuda", "cpu"):
                want_d, want_i = kiez(hub).fit(s64.to(dev), tw.to(dev)).kneighbors(5)
                k = kiez(hub).fit(pair[0].to(dev), pair[1].to(dev))
                nn = k.algorithm
                assert nn.target_index.elem == "float64" and getattr(nn, "source_index", nn.target_index).elem == "float64"
                d, i = k.kneighbors(5)
                assert torch.equal(i.cpu(), want_i.cpu()) and torch.equal(d.cpu(), want_d.cpu()), (dt, pair[1].dtype, hub, dev)
                gold = np.arange(400) %% 500
                assert np.array_equal(nn.gold_ranks(gold, s_to_t=False), kiez(hub).fit(s64.to(dev), tw.to(dev)).algorithm.gold_ranks(gold, s_to_t=False)) if hub else True
    # a NaN in a CUDA half tensor: reported by the first search, not by fit
    bad = sh.to("cuda").clone()
    bad[3, 2] = float("nan")
    k = kiez(None).fit(bad, th.to("cuda"))
    try:
        k.kneighbors(5)
        raise SystemExit("NaN input was not rejected")
    except ValueError as e:
        assert "NaN" in str(e), e
print("HALF_TORCH_OK")
"""


def test_torch_half_tensors_subprocess():
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT % str(ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HALF_TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
