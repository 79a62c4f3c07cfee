"""The fused sweep kernels -- the largest device code of the tree: kz_knn_h16.h, kz_knn_hx16.h, kz_knn_h64.h, kz_knn_bf16.h, the float32
kz_knn_cand_kernel, the epilogues kz_knn_epi3.h / kz_knn_epi4.h / kz_tile_epilogue* -- run ONE launch at a time through the hook
kz_selftest_sweep (the stages every search runs, stopped before the finalize kernel), their raw candidate lists and event log judged by
tests/sweep_restate.py against float64 reference keys made from the operand images the launch read (kz_selftest_image).

Why directly: end to end a lossy sweep is repaired downstream -- a dropped candidate leaves a row uncertified, the row is searched again
on a lower tier, the answer is still exact and nothing asserts how many rows took that way -- and the certification ASSUMES the contract
checked here (every row outside a list lies at or below the list's smallest key; the log holds every group with an event, once).

Data: 300 query rows (2 tiles + 44 rows; the 64-query build's last unit is half empty), 3 109 index rows (24 tiles + 37 rows: the last
tile is mostly pad rows), standard normal, over 1 and 3 index ranges.  Every entry tests/test_gpu_kernel_table.py enumerates is run and
must report itself (list length, slice count, workgroups and query tiles per item): fp16 narrow / wide / parity-split x K' in ordinary
and dual-pass builds, the 64-query entries, split-bf16, float32.  Entries this module cannot reach: none.

Dual builds, two settings: the shared-sweep form (theta constant per index tile -- the key of rank 12 among the tile's rows for a median
query --, qnbias = -bias(q)) and the range re-search form of kz_range_sweep_rows (theta = 0, qnbias = the key of rank 200 per query,
lists seeded at +inf: they stay empty and the log holds the range).  A theta that varies INSIDE a tile is not in the sweep kernels'
contract and is not tested: they read one value per tile, the first row's (kz_knn_h16.h: `tbuf[th_cur * 64]`; the rows of the sorted
image are ordered by threshold), and kz_dual_scatter_kernel applies the per-row values behind the sweep.

Adversarial orders (d = 64 and 128, where the tolerance is far below the key spacing): index rows a_t u + 1e-3 noise with a_t = t / n_i,
queries +4u -- keys rise with the row number: every key of every tile is an event, the pool overflows, the resumable path runs on every
tile -- and -4u (nothing is an event after the first tiles); and 40 identical copies of one row among each query's best.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import image_restate as I
from tests import sweep_restate as S

pytestmark = pytest.mark.gpu

BIAS, F32, BF, H, H_BIAS = 1, 3, 4, 9, 10   # KZ_IMG_* of kz_selftest_image
KPS = [16, 32, 64, 128]
_F, _I32 = C.POINTER(C.c_float), C.POINTER(C.c_int32)


class Swp(C.Structure):   # kz_selftest_swp, include/kiez_amd.h
    _fields_ = [("tier", C.c_int32), ("KP", C.c_int32), ("q64", C.c_int32), ("dual", C.c_int32), ("n_ranges", C.c_int32),
                ("q_begin", C.c_int64), ("q_count", C.c_int64), ("h_qfloor", _F), ("h_theta", _F), ("h_qnbias", _F),
                ("log_cap", C.c_int64), ("list_capacity", C.c_int64), ("h_out_key", _F), ("h_out_idx", _I32), ("h_log_keys", _F),
                ("h_log_meta", _I32), ("n_list", C.c_int64), ("log_count", C.c_uint64),
                ("n_regions", C.c_int32), ("halves", C.c_int32), ("contig", C.c_int32), ("qt0", C.c_int32),
                ("qt_end", C.c_int32 * 8), ("pieces", C.c_int32 * 8), ("base", C.c_int64 * 8),
                ("wg_per_item", C.c_int32), ("tiles_per_item", C.c_int32), ("n_slices", C.c_int32), ("entry_KP", C.c_int32),
                ("n_items", C.c_int32), ("reserved", C.c_int32)]


_HIP_ERROR = []   # a runtime error of the library in one test: the tests behind it touch the device no more
OBSERVED = {}     # family -> [largest |key - ref| / tol, largest undecidable rows per list]: printed, never asserted


def _native():
    from kiez_amd import _native as N
    assert not _HIP_ERROR, f"an earlier test of this module ended with a runtime error of the library: {_HIP_ERROR[0]}"
    return N, N.Context.get()


def _read(m, what, dtype, partner=None):
    N, ctx = _native()
    head = (ctx.handle, m.handle, partner.handle if partner is not None else None, what, 0, None)
    nb = C.c_size_t(0)
    N._check(ctx.lib.kz_selftest_image(*head, None, 0, C.byref(nb)), "kz_selftest_image")
    out = np.empty(nb.value, dtype=np.uint8)
    N._check(ctx.lib.kz_selftest_image(*head, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(nb)), "kz_selftest_image")
    return out.view(dtype)


class Data:
    """The two device matrices of a case, and the reference keys of the tier's images as they lie on the device."""

    def __init__(self, tier, X, Y):
        N, ctx = _native()
        self.tier, self.d = tier, X.shape[1]
        self.qm, self.im = N.DeviceMatrix(ctx, X, "euclidean"), N.DeviceMatrix(ctx, Y, "euclidean")
        n_q, n_i, d = len(X), len(Y), self.d
        qp, yp = I.n_pad(n_q), I.n_pad(n_i)
        self.q_bias = None
        if tier == S.TIER_H:
            nsr = I.h_nsr(I.kg(d))
            q_ops = S.unpack_h(_read(self.qm, H, np.float16, partner=self.im), qp, nsr)
            y_ops = S.unpack_h(_read(self.im, H, np.float16), yp, nsr)
            bias = _read(self.im, H_BIAS, np.float32)
            self.q_bias = _read(self.qm, H_BIAS, np.float32, partner=self.im)
        elif tier == S.TIER_BF:
            q_ops, y_ops = S.unpack_bf(_read(self.qm, BF, np.uint16), qp, d), S.unpack_bf(_read(self.im, BF, np.uint16), yp, d)
            bias = _read(self.im, BIAS, np.float32)
        else:
            q_ops, y_ops = S.unpack_f32(_read(self.qm, F32, np.float32), qp, d), S.unpack_f32(_read(self.im, F32, np.float32), yp, d)
            bias = _read(self.im, BIAS, np.float32)
        assert len(bias) == yp and np.isneginf(bias[n_i:]).all(), "pad rows of the bias row must hold -inf"
        self.ref = S.reference(tier, d, q_ops, y_ops, bias, n_q, n_i)


@functools.lru_cache(maxsize=None)
def _normal(tier, d):
    return Data(tier, *S.data(d))


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _sweep(data, KP, n_ranges, *, q64=False, dual=False, q_begin=0, q_count=None, qfloor=None, theta=None, qnbias=None, log_cap=1 << 18):
    """One call of the hook (two: the geometry first): (Geometry, keys, ids, log or None, the filled struct)."""
    N, ctx = _native()
    t = Swp()
    t.tier, t.KP, t.q64, t.dual, t.n_ranges = data.tier, KP, int(q64), int(dual), n_ranges
    t.q_begin, t.q_count = q_begin, data.ref.n_q - q_begin if q_count is None else q_count
    hold = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (qfloor, theta, qnbias)]
    t.h_qfloor, t.h_theta, t.h_qnbias, t.log_cap = _ptr(hold[0], _F), _ptr(hold[1], _F), _ptr(hold[2], _F), log_cap if dual else 0
    lk, lm = (np.zeros((log_cap, 4), dtype=np.float32), np.zeros((log_cap, 2), dtype=np.int32)) if dual else (None, None)
    t.h_log_keys, t.h_log_meta = _ptr(lk, _F), _ptr(lm, _I32)

    def call():
        try:
            N._check(ctx.lib.kz_selftest_sweep(ctx.handle, data.qm.handle, data.im.handle, C.byref(t)), "kz_selftest_sweep")
        except RuntimeError as e:
            if not isinstance(e, NotImplementedError):   # (a refusal for want of a build is no runtime error of the device)
                _HIP_ERROR.append(str(e))
            raise
    call()
    assert 0 < t.n_list < 1 << 28 and t.n_regions >= 1
    keys, ids = np.zeros(t.n_list, dtype=np.float32), np.zeros(t.n_list, dtype=np.int32)
    t.h_out_key, t.h_out_idx, t.list_capacity = _ptr(keys, _F), _ptr(ids, _I32), t.n_list
    call()
    nr = t.n_regions
    geo = S.Geometry(data.tier, KP, list(t.qt_end[:nr]), list(t.pieces[:nr]), t.halves, t.contig, t.qt0, n_ranges, data.ref.n_i, t.q_begin, t.q_count)
    assert geo.lay.n_list == t.n_list and list(t.base[:nr]) == geo.lay.base
    log = dict(keys=lk, meta=lm, count=int(t.log_count), cap=log_cap) if dual else None
    return geo, keys, ids, log, t


def _observe(family, rep):
    o = OBSERVED.setdefault(family, [0.0, 0.0])
    o[0], o[1] = max(o[0], rep.max_ratio), max(o[1], rep.und_per_list())


@pytest.fixture(autouse=True)
def _print_observations():
    """What a maintainer wants to see beside a failure (pytest -s / the captured output): per family the largest |key - ref| / tol and
    the largest average of undecidable rows per list so far."""
    yield
    for family, (ratio, und) in sorted(OBSERVED.items()):
        print(f"observed[{family}]: largest |key - ref| / tol {ratio:.3f}, most undecidable rows per list {und:.2f}")


def _entry(t, KP, n_slices, wg_per_item=1, tiles_per_item=1):
    got = (t.entry_KP, t.n_slices, t.wg_per_item, t.tiles_per_item)
    assert got == (KP, n_slices, wg_per_item, tiles_per_item), f"the hook ran entry {got}"


def _run(family, data, KP, n_ranges, *, what, thresholds=None, **kw):
    """A launch, its lists (and log) checked."""
    if thresholds is not None:
        kw.update(dual=True, theta=thresholds[0], qnbias=thresholds[1])
    geo, keys, ids, log, t = _sweep(data, KP, n_ranges, **kw)
    rep = S.check_lists(keys, ids, geo, data.ref, kw.get("qfloor"))
    rep.assert_ok(f"{what}, K' = {KP}, {n_ranges} ranges: lists")
    _observe(family, rep)
    if log is not None:
        lrep = S.check_log(log["keys"], log["meta"], log["count"], log["cap"], geo, data.ref, kw["theta"], kw["qnbias"])
        lrep.assert_ok(f"{what}, K' = {KP}, {n_ranges} ranges: log of {log['count']} groups")
        assert log["count"] > 0
        _observe(family + " log", lrep)
    return geo, keys, ids, log, t


H_FAMILIES = {"narrow": (S.NARROW, 1), "wide": (S.WIDE, 1), "parity-split": (S.XWIDE, 2)}   # widths, workgroups per item


@pytest.mark.parametrize("KP", KPS)
@pytest.mark.parametrize("family", list(H_FAMILIES))
def test_fp16_entries(family, KP):
    dims, wg = H_FAMILIES[family]
    for d in dims:
        data = _normal(S.TIER_H, d)
        for n_ranges in (1, 3):
            t = _run(f"fp16 {family}", data, KP, n_ranges, what=f"fp16 {family}, d = {d}")[4]
            _entry(t, KP, I.h_nsr(I.kg(d)), wg)


@pytest.mark.parametrize("KP", KPS)
@pytest.mark.parametrize("family", list(H_FAMILIES))
def test_fp16_dual_entries(family, KP):
    dims, wg = H_FAMILIES[family]
    for d in dims:
        data = _normal(S.TIER_H, d)
        thr = S.shared_thresholds(data.ref, data.q_bias)
        for n_ranges in (1, 3):
            t = _run(f"fp16 {family} dual", data, KP, n_ranges, what=f"fp16 {family} dual pass, d = {d}", thresholds=thr)[4]
            _entry(t, KP, I.h_nsr(I.kg(d)), wg)


@pytest.mark.parametrize("dual", [False, True], ids=["ordinary", "dual"])
def test_64_query_entries(dual):
    for d in S.Q64:
        data = _normal(S.TIER_H, d)
        thr = S.shared_thresholds(data.ref, data.q_bias) if dual else None
        for n_ranges in (1, 3):
            t = _run("64-query" + (" dual" if dual else ""), data, 16, n_ranges, what=f"64-query build, d = {d}", thresholds=thr, q64=True)[4]
            _entry(t, 16, d // 16, 1, 2)


@pytest.mark.parametrize("KP", KPS)
def test_split_bf16_entries(KP):
    for d in S.NARROW:
        data = _normal(S.TIER_BF, d)
        for n_ranges in (1, 3):
            t = _run("split-bf16", data, KP, n_ranges, what=f"split-bf16, d = {d}")[4]
            _entry(t, KP, d // 16)


@pytest.mark.parametrize("KP", KPS)
def test_float32_entries(KP):
    for d in (200, 37):
        data = _normal(S.TIER_F32, d)
        for n_ranges in (1, 3):
            t = _run("float32", data, KP, n_ranges, what=f"float32 operands, d = {d}")[4]
            _entry(t, KP, I.h_nsr(I.kg(d)))


def test_a_row_range_off_the_first_tile():
    """Rows 130 .. 279: the launch starts at query tile 1, list row 2."""
    for tier, d in ((S.TIER_H, 64), (S.TIER_BF, 64), (S.TIER_F32, 200)):
        data = _normal(tier, d)
        geo = _run("row range", data, 16, 3, what=f"tier {tier}, rows 130 .. 279", q_begin=130, q_count=150)[0]
        assert geo.qt0 == 1
    data = _normal(S.TIER_H, 64)
    _run("row range", data, 16, 3, what="64-query build, rows 130 .. 279", q_begin=130, q_count=150, q64=True)
    _run("row range", data, 16, 3, what="dual pass, rows 130 .. 279", q_begin=130, q_count=150, thresholds=S.shared_thresholds(data.ref, data.q_bias))


# ---- adversarial orders -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ordered(tier, d, ties):
    rng = np.random.RandomState(7 + d)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    a = np.arange(S.N_I) / S.N_I
    Y = a[:, None] * u[None, :] + 1e-3 * rng.standard_normal((S.N_I, d))
    if ties:   # 40 copies of one row among the best of the +4u queries, 40 of another among the best of the -4u queries, all over the index
        where = rng.permutation(S.N_I)[:80]
        Y[where[:40]] = 1.0005 * u
        Y[where[40:]] = -0.0005 * u
    X = np.concatenate([np.tile(4.0 * u, (S.N_Q // 2, 1)), np.tile(-4.0 * u, (S.N_Q - S.N_Q // 2, 1))])
    return Data(tier, X.astype(np.float32), Y.astype(np.float32))


ADVERSARIAL = [("fp16", S.TIER_H, KP, False) for KP in KPS] + [("64-query", S.TIER_H, 16, True), ("split-bf16", S.TIER_BF, 16, False),
                                                               ("split-bf16", S.TIER_BF, 64, False), ("float32", S.TIER_F32, 16, False),
                                                               ("float32", S.TIER_F32, 128, False)]


@pytest.mark.parametrize("ties", [False, True], ids=["ordered", "ties"])
@pytest.mark.parametrize("name,tier,KP,q64", ADVERSARIAL, ids=[f"{a[0]}-{a[2]}" for a in ADVERSARIAL])
def test_adversarial_orders(name, tier, KP, q64, ties):
    for d in (64, 128):
        data = _ordered(tier, d, ties)
        for n_ranges in (1, 3):
            geo, keys, ids, _, _ = _run(f"adversarial {name}", data, KP, n_ranges, what=f"{name}, rising / falling keys, d = {d}", q64=q64)
            if not ties:   # (the tolerance is far below the spacing: the lists are the reference's top K', row for row, up to near-ties)
                off = geo.offsets()
                top = np.argsort(-data.ref.key, axis=1)[:, :4]
                got = ids[off].reshape(S.N_Q, -1)
                assert all(top[q, 0] in got[q] for q in range(S.N_Q)), "a query's best row is in none of its lists"
    if tier == S.TIER_H and not q64:
        # the dual build on the same orders: the rising keys fill the event pool with list AND column entries
        data = _ordered(tier, 64, ties)
        _run(f"adversarial {name} dual", data, KP, 3, what=f"{name} dual pass, rising / falling keys", thresholds=S.shared_thresholds(data.ref, data.q_bias))


# ---- seeded lists -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dual", [False, True], ids=["ordinary", "dual"])
@pytest.mark.parametrize("KP", KPS)
def test_seeded_lists(KP, dual):
    for d in (64, 208, 640, 1280):
        data = _normal(S.TIER_H, d)
        floor = S.rank_floor(data.ref, 2 * KP)
        thr = S.shared_thresholds(data.ref, data.q_bias) if dual else None
        for n_ranges in (1, 3):
            geo, keys, ids, _, _ = _run("seeded", data, KP, n_ranges, what=f"seeded lists, d = {d}", qfloor=floor, thresholds=thr)
            off = geo.offsets()
            n_ids = (ids[off] >= 0).sum(axis=(1, 2, 3))
            # a query without a floor fills its lists; a floored one keeps, per range, the rows above its floor (up to K' of them: about
            # 2 K' - 1 in all) and floor entries elsewhere -- counted on the reference keys, a tolerance to either side of the floor
            assert (n_ids[1::2] == KP * geo.n_pieces).all()
            tol, fl = data.ref.tol(), floor[:S.N_Q].astype(np.float64)[:, None]
            lo, hi = np.zeros(S.N_Q, dtype=np.int64), np.zeros(S.N_Q, dtype=np.int64)
            for piece in range(geo.n_pieces):
                dom = geo.domain(piece, 0)
                lo += np.minimum(KP, (data.ref.key[:, dom] > fl + tol[:, dom]).sum(axis=1))
                hi += np.minimum(KP, (data.ref.key[:, dom] > fl - tol[:, dom]).sum(axis=1))
            assert (lo[0::2] <= n_ids[0::2]).all() and (n_ids[0::2] <= hi[0::2]).all()
            assert n_ranges == 1 or (n_ids[0::2] < KP * geo.n_pieces).all(), "no floor entry is left: the case tests nothing"
    if KP == 16:
        data = _normal(S.TIER_H, 64)
        _run("seeded", data, 16, 3, what="seeded lists, 64-query build", qfloor=S.rank_floor(data.ref, 32), q64=True)


# ---- dual builds: the range re-search form, the overflow report ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 208, 384, 512, 2048])
def test_range_form(d):
    """kz_range_sweep_rows: theta = 0, qnbias = the key of rank 200, lists seeded at +inf -- they stay empty, the log holds the range."""
    data = _normal(S.TIER_H, d)
    theta, qnbias, inf = S.range_thresholds(data.ref)
    for n_ranges in (1, 3):
        geo, keys, ids, log, _ = _run("range form", data, 16, n_ranges, what=f"range form, d = {d}", qfloor=inf, thresholds=(theta, qnbias))
        off = geo.offsets()
        assert (ids[off] == -1).all() and np.isposinf(keys[off]).all()
        assert 50 * S.N_Q <= log["count"] <= 200 * S.N_Q + 4 * S.N_Q


@pytest.mark.parametrize("q64", [False, True], ids=["32-query", "64-query"])
def test_log_overflow_is_reported(q64):
    data = _normal(S.TIER_H, 64)
    theta, qnbias = S.shared_thresholds(data.ref, data.q_bias)
    geo, keys, ids, log, _ = _sweep(data, 16, 1, dual=True, q64=q64, theta=theta, qnbias=qnbias, log_cap=64)
    S.check_lists(keys, ids, geo, data.ref).assert_ok("lists beside an overflowing log")
    rep = S.check_log(log["keys"], log["meta"], log["count"], 64, geo, data.ref, theta, qnbias)
    assert rep.codes() == {"overflow"}, rep.errors
    full = _sweep(data, 16, 1, dual=True, q64=q64, theta=theta, qnbias=qnbias)[3]
    assert log["count"] == full["count"] > 64, "the counter counts every group, written or not"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    N, ctx = _native()
    data = _normal(S.TIER_H, 64)
    with pytest.raises(NotImplementedError, match="no sweep kernel"):      # the 64-query kernel is built for K' = 16 only
        _sweep(data, 32, 1, q64=True)
    with pytest.raises(NotImplementedError, match="no sweep kernel"):      # ... and for 4 .. 13 slices
        _sweep(_normal(S.TIER_H, 32), 16, 1, q64=True)
    with pytest.raises(NotImplementedError, match="fp16 tier only"):
        _sweep(_normal(S.TIER_F32, 200), 16, 1, q64=True)
    odd = Data(S.TIER_F32, *S.data(400))                                    # 25 slices: no fp16 and no split-bf16 kernel
    for tier in (S.TIER_H, S.TIER_BF):
        odd.tier = tier
        with pytest.raises(NotImplementedError, match="no kernel for d=400"):
            _sweep(odd, 16, 1)
    with pytest.raises(ValueError, match="query rows"):
        _sweep(data, 16, 1, q_count=0)
    with pytest.raises(ValueError, match="query rows"):
        _sweep(data, 16, 1, q_begin=200, q_count=101)
    with pytest.raises(ValueError, match="lists of 48"):
        _sweep(data, 48, 1)
    with pytest.raises(ValueError, match="a dual build needs"):
        _sweep(data, 16, 1, dual=True)
    with pytest.raises(ValueError, match="fp16 tier only"):
        _sweep(_normal(S.TIER_F32, 200), 16, 1, qfloor=np.zeros(384, dtype=np.float32))
    ctx.set_option("chunk_rows", 128)
    try:
        with pytest.raises(ValueError, match="more than one launch"):
            _sweep(data, 16, 1)
    finally:
        ctx.set_option("chunk_rows", 0)
    # matrices the sweep is not for: another context's, another metric's
    other = N.Context(ctx.device)
    foreign = Data.__new__(Data)
    foreign.tier, foreign.ref, foreign.im = S.TIER_H, data.ref, data.im
    foreign.qm = N.DeviceMatrix(other, S.data(64)[0], "euclidean")
    with pytest.raises(ValueError, match="foreign matrix"):
        _sweep(foreign, 16, 1)
    foreign.qm = N.DeviceMatrix(ctx, S.data(64)[0], "manhattan")
    foreign.im = N.DeviceMatrix(ctx, S.data(64)[1], "manhattan")
    with pytest.raises(ValueError, match="euclidean family or cosine"):
        _sweep(foreign, 16, 1)
    foreign.qm = N.DeviceMatrix(ctx, S.data(64)[0], "cosine")
    foreign.im = data.im
    with pytest.raises(ValueError, match="share width, metric"):
        _sweep(foreign, 16, 1)
    _run("fp16 narrow", data, 16, 1, what="after the refusals")   # (a refusal leaves the context usable)
