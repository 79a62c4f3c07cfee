"""The contract of the fused sweep kernels (kiez_amd/csrc/kz_knn.hip: kz_knn_cand_kernel; kz_knn_bf16.h; kz_knn_h16.h, kz_knn_hx16.h,
kz_knn_h64.h with the epilogues kz_knn_epi3.h / kz_knn_epi4.h), checked from outside in numpy float64 (test infrastructure of
tests/test_sweep_restate.py and tests/test_gpu_sweep_direct.py).  Nothing here restates a kernel: the checkers take the raw candidate
lists and the raw event log of one launch (hook kz_selftest_sweep) and the operand images the launch read (hook kz_selftest_image,
un-laid-out with tests/image_restate.py) and ask what the kernel headers promise:

  lists   each list holds the K' largest APPROXIMATE keys of the index rows it is responsible for (its domain): fp16 and split-bf16 one
          list per query and index range; float32 operands two per range, lane half h seeing the rows with (row & 4) == 4 h
          (kz_knn_device.h "list(q, h) sees index rows with (row & 4) == 4h").  The two half lists of a float32 range prune with the
          LARGER of their two thresholds (kz_tile_epilogue: tau_eff), so what bounds a row outside them is the larger of their two
          minima -- the finalize kernel's piece_bound takes the maximum over a query's full lists in the same way.
  log     (dual builds) every group of four keys -- one query, index rows row0 .. row0 + 3 -- whose largest key reaches
          fl(qnbias(q) + theta(first row of the tile)) is in the log, once (kz_tile_epilogue3: cthr).  The kernel reads ONE theta per
          tile, the first row's: the rows of the sorted image are ordered by threshold, so that is the tile's smallest.  A theta that
          varies inside a tile is applied per key by kz_dual_scatter_kernel behind the sweep, not by the sweep.

Reference keys: float64 sums of the image's own operand values plus the float32 bias row as stored -- fp16: q_h.y_h + bias_h;
split-bf16: hi.hi + hi.lo + lo.hi + bias, the three products the kernel forms; float32: q.y + bias.  Tolerance per pair: the
accumulation factor the library certifies with (kz_gamma_acc_h; the accumulation part of kz_bf16_gamma; gamma_f32 of kz_knn_impl) times
|bias(y)| + |q| |y| of the image rows.  Nothing is measured on the code under test.
"""
import numpy as np

from tests import finalize_restate as F
from tests import image_restate as I

TILE = 128
TIER_F32, TIER_BF, TIER_H = 0, 1, 2
U24 = 2.0 ** -24


# ---- reference keys -------------------------------------------------------------------------------------------------------------------
def d_pad(d):
    return (d + 15) // 16 * 16


def factor(tier, d):
    """The accumulation factor of the tier's certification bound."""
    if tier == TIER_H:
        return F.gamma_acc_h(d)                       # kz_gamma_acc_h: 2 (d_pad + 16) 2^-24
    if tier == TIER_BF:
        return 2.0 * (3 * d_pad(d) + 16) * U24        # kz_bf16_gamma without the split term
    return (d_pad(d) + 16) * U24                      # gamma_f32 of kz_knn_impl without the re-rank's 1e-12


def unpack_f32(img, n, d):
    """[n, d_pad] float64 operands of a float32 image (n = padded rows)."""
    r, k = I.grid(n, d_pad(d))
    return np.asarray(img, dtype=np.float32)[I.f32_offset(r, k, d)].astype(np.float64)


def unpack_bf(img, n, d):
    """(hi, lo) [n, d_pad] float64 of a split-bf16 image (uint16 bit patterns)."""
    r, k = I.grid(n, d_pad(d))
    img = np.asarray(img, dtype=np.uint16)
    return I.bf16_to_f64(img[I.bf_offset(r, k, d, 0)]), I.bf16_to_f64(img[I.bf_offset(r, k, d, 1)])


def unpack_h(img, n, nsr):
    """[n, 16 nsr] float64 of an fp16 image."""
    r, k = I.grid(n, 16 * nsr)
    return np.asarray(img, dtype=np.float16)[I.h_offset(r, k, nsr)].astype(np.float64)


class Ref:
    """Reference keys [n_q, n_i] of the real rows, and what the tolerance is made of."""

    def __init__(self, tier, d, key, q_norm, y_norm, bias):
        self.tier, self.d, self.key = tier, d, key
        self.q_norm, self.y_norm, self.bias = q_norm, y_norm, np.asarray(bias, dtype=np.float64)
        self.factor = factor(tier, d)
        self.n_q, self.n_i = key.shape

    def tol(self, rows=slice(None)):
        return self.factor * (np.abs(self.bias)[None, :] + self.q_norm[rows, None] * self.y_norm[None, :])


def reference(tier, d, q_ops, y_ops, bias32, n_q, n_i):
    """q_ops / y_ops: the un-laid-out operands of the two images (split-bf16: (hi, lo) pairs), padded rows included; bias32: the float32
    accumulator-init row of the index image as stored."""
    bias = np.asarray(bias32, dtype=np.float32).astype(np.float64)[:n_i]
    if tier == TIER_BF:
        qh, ql, yh, yl = q_ops[0][:n_q], q_ops[1][:n_q], y_ops[0][:n_i], y_ops[1][:n_i]
        key = qh @ yh.T + qh @ yl.T + ql @ yh.T
        qn, yn = np.linalg.norm(qh + ql, axis=1), np.linalg.norm(yh + yl, axis=1)
    else:
        q, y = q_ops[:n_q], y_ops[:n_i]
        key = q @ y.T
        qn, yn = np.linalg.norm(q, axis=1), np.linalg.norm(y, axis=1)
    return Ref(tier, d, key + bias[None, :], qn, yn, bias)


def cpu_images(tier, X, Y, metric="euclidean"):
    """Operand values as kz_pack.hip derives them, for tests without a device (same shapes and magnitudes as the device's images; the
    fp16 centre here is the float32 column mean of Y): (q_ops, y_ops, bias32) as `reference` takes them, and the same bias row of the
    query side (what a shared sweep's qnbias is the negative of)."""
    assert metric == "euclidean"
    X32, Y32 = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    d = X32.shape[1]
    pad = lambda a: np.pad(a, ((0, 0), (0, d_pad(d) - d)))
    if tier == TIER_H:
        mu = Y32.astype(np.float64).mean(axis=0).astype(np.float32)
        vq = (X32.astype(np.float64) - mu.astype(np.float64)).astype(np.float32)
        vy = (Y32.astype(np.float64) - mu.astype(np.float64)).astype(np.float32)
        S = I.scale_of(float(max(np.abs(vq).max(), np.abs(vy).max())))
        _, qh = I.h_pipeline(X32, mu, S)
        _, yh = I.h_pipeline(Y32, mu, S)
        bias = lambda v: (-0.5 * S * S * (v.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        return pad(qh.astype(np.float64)), pad(yh.astype(np.float64)), bias(vy), bias(vq)
    bias = lambda v: (-0.5 * (v.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    if tier == TIER_BF:
        split = lambda a: tuple(pad(I.bf16_to_f64(p)) for p in I.bf_split(a.astype(np.float64)))
        return split(X32), split(Y32), bias(Y32), bias(X32)
    return pad(X32.astype(np.float64)), pad(Y32.astype(np.float64)), bias(Y32), bias(X32)


# ---- the inputs of the two test modules ------------------------------------------------------------------------------------------------
N_Q, N_I = 300, 3109            # 2 query tiles + 44 rows; 24 index tiles + 37 rows (the last tile is mostly pad rows)
NARROW = [16 * s for s in range(2, 25)]     # 2 .. 24 slices
WIDE = [512, 640, 768, 896, 1024]           # 32 .. 64 slices
XWIDE = [1280, 1536, 1792, 2048]            # 80 .. 128 slices
Q64 = [16 * s for s in range(4, 14)]        # 4 .. 13 slices: the 64-query kernel


def data(d):
    """(queries, index): standard normal float32, fixed seeds."""
    return (np.random.RandomState(100003 + d).standard_normal((N_Q, d)).astype(np.float32),
            np.random.RandomState(200006 + d).standard_normal((N_I, d)).astype(np.float32))


def shared_thresholds(ref, q_bias32, rank=12):
    """The shared-sweep form of a dual launch: theta constant per index tile = the reference key of rank `rank` among the tile's rows for
    the query m of median bias, in the units of the test (key + bias(q) >= theta: plus bias(m)); qnbias = -bias(q), +inf on pad rows."""
    qb = np.asarray(q_bias32, dtype=np.float32)[:ref.n_q]
    m = int(np.argsort(qb)[ref.n_q // 2])
    n_t = (ref.n_i + TILE - 1) // TILE
    theta = np.full(n_t * TILE, np.inf, dtype=np.float32)
    for t in range(n_t):
        k = np.sort(ref.key[m, t * TILE:min((t + 1) * TILE, ref.n_i)])[::-1]
        theta[t * TILE:(t + 1) * TILE] = np.float32(k[min(rank, len(k)) - 1] + float(qb[m]))
    qnbias = np.full((ref.n_q + TILE - 1) // TILE * TILE, np.inf, dtype=np.float32)
    qnbias[:ref.n_q] = -qb
    return theta, qnbias


def range_thresholds(ref, rank=200):
    """The range re-search form (kz_range_sweep_rows): theta = 0, qnbias = the reference key of rank `rank` per query, qfloor = +inf."""
    n_t, q_pad = (ref.n_i + TILE - 1) // TILE, (ref.n_q + TILE - 1) // TILE * TILE
    qnbias = np.full(q_pad, np.inf, dtype=np.float32)
    qnbias[:ref.n_q] = np.sort(ref.key, axis=1)[:, -rank].astype(np.float32)
    return np.zeros(n_t * TILE, dtype=np.float32), qnbias, np.full(q_pad, np.inf, dtype=np.float32)


def rank_floor(ref, rank, every=2):
    """Seeded lists: qfloor = the reference key of rank `rank` for every `every`-th query, -inf for the rest (and on pad rows)."""
    q_pad = (ref.n_q + TILE - 1) // TILE * TILE
    fl = np.full(q_pad, -np.inf, dtype=np.float32)
    fl[0:ref.n_q:every] = np.sort(ref.key, axis=1)[0:ref.n_q:every, -rank].astype(np.float32)
    return fl


# ---- geometry of one launch -----------------------------------------------------------------------------------------------------------
class Geometry:
    """What kz_selftest_sweep reports of a launch: the list layout, and which index rows range `piece` covers (kz_plan_fill_work: ranges
    of ceil(n_ytiles / requested) tiles, the last one shorter)."""

    def __init__(self, tier, KP, qt_end, pieces, halves, contig, qt0, n_ranges, n_i, q_begin, q_count):
        self.tier, self.KP, self.qt0, self.n_i, self.q_begin, self.q_count = tier, KP, qt0, n_i, q_begin, q_count
        self.lay = F.Layout(qt_end, pieces, halves, contig, KP)
        self.n_ytiles = (n_i + TILE - 1) // TILE
        sp = min(n_ranges, self.n_ytiles)
        self.range_tiles = (self.n_ytiles + sp - 1) // sp
        self.n_pieces = (self.n_ytiles + self.range_tiles - 1) // self.range_tiles
        assert all(p == self.n_pieces for p in pieces), (pieces, self.n_pieces)
        # lists of a (query, range): float32 operands two (lane halves), else one in the lane-half-0 slots
        self.lists = 2 if tier == TIER_F32 else 1
        assert halves == self.lists and contig == (1 if tier == TIER_H else 0), (tier, halves, contig)

    def key(self):
        return (self.tier, self.KP, tuple(self.lay.qt_end), tuple(self.lay.pieces), self.qt0, self.q_begin, self.q_count)

    def piece_rows(self, piece):
        lo = piece * self.range_tiles * TILE
        return lo, min((piece + 1) * self.range_tiles * TILE, self.n_i)

    def domain(self, piece, h):
        """bool [n_i]: the rows list (range `piece`, lane half h) is responsible for."""
        lo, hi = self.piece_rows(piece)
        r = np.arange(self.n_i)
        dom = (r >= lo) & (r < hi)
        return dom & ((r & 4) == 4 * h) if self.tier == TIER_F32 else dom

    def offsets(self):
        """int64 [q_count, pieces, lists, KP]: where entry e of list (piece, h) of local query q lies (finalize_restate.Layout)."""
        key = self.key()
        if key not in _OFFSETS:
            row0 = self.q_begin - TILE * self.qt0
            out = np.stack([self.lay.offsets(row0 + q) for q in range(self.q_count)])
            _OFFSETS[key] = out.reshape(self.q_count, self.n_pieces, self.lists, self.KP)
        return _OFFSETS[key]


_OFFSETS = {}   # (the layouts of a test module are few: one per tier, list length, range count and row range)


# ---- lists ----------------------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.errors = []          # (code, text)
        self.bad_lists = None     # bool [q_count, pieces, lists]: lists with any violation
        self.undecidable = 0      # rows outside their list with ref > m - tol
        self.n_lists = 0
        self.max_ratio = 0.0      # largest |key - ref| / tol over the entries with an id

    def codes(self):
        return {c for c, _ in self.errors}

    def und_per_list(self):
        return self.undecidable / max(1, self.n_lists)

    def assert_ok(self, what=""):
        assert not self.errors, f"{what}: {len(self.errors)} violations, first: {self.errors[:3]}"


def check_lists(out_key, out_idx, geo, ref, qfloor=None):
    """The lists of one launch against the contract.  Codes: id (an id outside [0, n_i)), domain (an id of another range or lane half),
    key (|key - ref| > tol), dup (an id twice in a list), start (an entry without an id that is not the list's start value), floor (a
    seeded list holding an id whose key does not exceed the floor), outside (a domain row that is not in the list with ref > m + tol)."""
    rep = Report()
    off = geo.offsets()
    K, Ix = np.asarray(out_key, dtype=np.float32)[off], np.asarray(out_idx, dtype=np.int32)[off].astype(np.int64)
    rows = np.arange(geo.q_begin, geo.q_begin + geo.q_count)
    n_i, nq = geo.n_i, geo.q_count
    tol, refk = ref.tol(rows), ref.key[rows]
    start = np.full(nq, -np.inf, dtype=np.float32) if qfloor is None else np.asarray(qfloor, dtype=np.float32)[rows]
    bad = np.zeros(K.shape[:3], dtype=bool)
    qi = np.arange(nq)[:, None]

    def note(code, mask, piece, h, text):
        if mask.any():
            per_list = mask.any(axis=1) if mask.ndim == 2 else mask
            bad[:, piece, h] |= per_list
            q = int(np.flatnonzero(per_list)[0])
            rep.errors.append((code, f"{text}: {int(mask.sum())} times, first at query {int(rows[q])}, range {piece}, lane half {h}"))

    for piece in range(geo.n_pieces):
        mins, inlists, doms = [], [], []
        for h in range(geo.lists):
            k, i = K[:, piece, h, :].astype(np.float64), Ix[:, piece, h, :]
            dom = geo.domain(piece, h)
            has = i >= 0
            bad_id = (i < -1) | (i >= n_i)
            ic = np.clip(i, 0, n_i - 1)
            ok = has & ~bad_id
            note("id", bad_id, piece, h, "an id outside [0, n_i)")
            note("domain", ok & ~dom[ic], piece, h, "an id outside the list's domain")
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(ok, np.abs(k - refk[qi, ic]) / tol[qi, ic], 0.0)
            note("key", ok & ~(ratio <= 1.0), piece, h, "a key further from its reference than the tolerance")
            if ok.any():
                rep.max_ratio = max(rep.max_ratio, float(np.nanmax(np.where(ok, ratio, 0.0))))
            s = np.sort(np.where(ok, i, -1 - np.arange(i.shape[1])[None, :]), axis=1)
            note("dup", s[:, 1:] == s[:, :-1], piece, h, "an id twice in one list")
            note("start", ~has & ~(K[:, piece, h, :] == start[:, None]), piece, h, "an entry without an id that is not the list's start value")
            if qfloor is not None:
                note("floor", ok & ~(K[:, piece, h, :] > start[:, None]), piece, h, "a seeded list holds a key at or below its floor")
            with np.errstate(invalid="ignore"):
                m = np.where(np.isnan(k).any(axis=1), -np.inf, k.min(axis=1))
            inl = np.zeros((nq, n_i + 1), dtype=bool)          # (column n_i takes the entries without a usable id)
            np.put_along_axis(inl, np.where(ok, ic, n_i), True, axis=1)
            inl = inl[:, :n_i]
            mins.append(m)
            inlists.append(inl)
            doms.append(dom)
        # the two half lists of a float32 range prune with the larger threshold of the two
        m_eff = np.maximum.reduce(mins)
        for h in range(geo.lists):
            outside = doms[h][None, :] & ~inlists[h]
            note("outside", outside & (refk > m_eff[:, None] + tol), piece, h, "a domain row above the list's smallest key is not in the list")
            rep.undecidable += int((outside & (refk > m_eff[:, None] - tol)).sum())
            rep.n_lists += nq
    rep.bad_lists = bad
    return rep


def make_lists(geo, ref, n_list, qfloor=None):
    """(keys, ids) of a launch as a kernel that meets the contract with zero error would leave them: the K' largest float32(ref) of every
    domain above the list's start value, in no particular order; NaN / -1 in the slots no list owns."""
    keys, ids = np.full(n_list, np.nan, dtype=np.float32), np.full(n_list, -1, dtype=np.int32)
    off = geo.offsets()
    rows = np.arange(geo.q_begin, geo.q_begin + geo.q_count)
    start = np.full(geo.q_count, -np.inf, dtype=np.float32) if qfloor is None else np.asarray(qfloor, dtype=np.float32)[rows]
    k32 = ref.key[rows].astype(np.float32)
    for piece in range(geo.n_pieces):
        for h in range(geo.lists):
            dom = np.flatnonzero(geo.domain(piece, h))
            sub = k32[:, dom]
            order = np.argsort(-sub, axis=1, kind="stable")[:, :geo.KP]
            lk = np.take_along_axis(sub, order, axis=1)
            li = dom[order].astype(np.int32)
            if order.shape[1] < geo.KP:
                lk = np.pad(lk, ((0, 0), (0, geo.KP - order.shape[1])), constant_values=-np.inf)
                li = np.pad(li, ((0, 0), (0, geo.KP - order.shape[1])), constant_values=-1)
            take = lk > start[:, None]
            keys[off[:, piece, h, :]] = np.where(take, lk, start[:, None])
            ids[off[:, piece, h, :]] = np.where(take, li, -1)
    return keys, ids


# ---- event log ------------------------------------------------------------------------------------------------------------------------
def decode_meta(meta):
    """(query image row, first index row, tile) of log entries, as kz_dual_scatter_kernel decodes them."""
    x, y = np.asarray(meta)[:, 0].astype(np.int64), np.asarray(meta)[:, 1].astype(np.int64)
    ql, tg = x & 63, x >> 6
    row0 = (tg >> 4) * TILE + ((tg >> 2) & 3) * 32 + (tg & 3) * 8 + 4 * (ql >> 5)
    return y, row0, tg >> 4


def check_log(log_keys, log_meta, counter, log_cap, geo, ref, theta, qnbias):
    """The event log of one dual-pass launch.  Codes: where (an entry that names no query row of the launch or no index tile), key, test
    (no key of a logged group reaches the kernel's threshold), dup, missing (a pair with ref - theta >= qnbias + tol whose group is not
    in the log), overflow (the counter exceeds log_cap: reported, and only the log_cap entries there are judged -- `missing` is not)."""
    rep = Report()
    n = int(min(counter, log_cap))
    keys = np.asarray(log_keys, dtype=np.float32).reshape(-1, 4)[:n]
    meta = np.asarray(log_meta, dtype=np.int32).reshape(-1, 2)[:n]
    theta, qnbias = np.asarray(theta, dtype=np.float32), np.asarray(qnbias, dtype=np.float32)
    y, row0, tile = decode_meta(meta)
    rows = np.arange(geo.q_begin, geo.q_begin + geo.q_count)
    q_lo, q_hi = geo.qt0 * TILE, min(ref.n_q, (geo.qt0 + geo.lay.qt_end[-1]) * TILE)   # (whole tiles are swept; rows outside the call carry +inf)
    if counter > log_cap:
        rep.errors.append(("overflow", f"the counter says {counter} groups for a log of {log_cap}"))
    where = (y < q_lo) | (y >= q_hi) | (tile < 0) | (tile >= geo.n_ytiles) | (meta[:, 0] < 0)
    if where.any():
        rep.errors.append(("where", f"{int(where.sum())} entries name no query row or index tile of the launch, first {meta[np.flatnonzero(where)[0]].tolist()}"))
        keys, meta, y, row0, tile = (a[~where] for a in (keys, meta, y, row0, tile))
    r4 = row0[:, None] + np.arange(4)[None, :]
    real = r4 < geo.n_i                                    # (pad rows of the last tile: bias -inf, excluded)
    rc = np.clip(r4, 0, geo.n_i - 1)
    refk, tol = ref.key[y[:, None], rc], ref.factor * (np.abs(ref.bias)[rc] + ref.q_norm[y][:, None] * ref.y_norm[rc])
    with np.errstate(invalid="ignore"):
        ratio = np.where(real, np.abs(keys.astype(np.float64) - refk) / tol, 0.0)
    far = real & ~(ratio <= 1.0)
    if far.any():
        rep.errors.append(("key", f"{int(far.sum())} logged keys further from their reference than the tolerance (largest ratio {np.nanmax(ratio):.3g})"))
    rep.max_ratio = float(ratio.max()) if ratio.size else 0.0
    # the kernel's own float32 test (kz_tile_epilogue3): the group's largest key against fl(qnbias(q) + theta of the tile's first row)
    with np.errstate(invalid="ignore", over="ignore"):
        cthr = (qnbias[y] + theta[tile * TILE]).astype(np.float32)
        passes = keys.max(axis=1) >= cthr
    if not passes.all():
        rep.errors.append(("test", f"{int((~passes).sum())} logged groups hold no key that reaches the threshold"))
    code = meta[:, 0].astype(np.int64) * (1 << 32) + y
    if len(np.unique(code)) != len(code):
        rep.errors.append(("dup", f"{len(code) - len(np.unique(code))} groups are logged more than once"))
    if counter <= log_cap:
        logged = np.zeros((ref.n_q, geo.n_i), dtype=bool)
        logged[np.broadcast_to(y[:, None], rc.shape)[real], rc[real]] = True
        th_row = theta[(np.arange(geo.n_i) // TILE) * TILE].astype(np.float64)
        with np.errstate(invalid="ignore"):
            need = ref.key[rows] - th_row[None, :] >= qnbias[rows].astype(np.float64)[:, None] + ref.tol(rows)
        missing = need & ~logged[rows]
        if missing.any():
            q, r = (int(a[0]) for a in np.nonzero(missing))
            rep.errors.append(("missing", f"{int(missing.sum())} pairs above their threshold lie in no logged group, first (query {int(rows[q])}, row {r})"))
        with np.errstate(invalid="ignore"):
            und = np.abs(ref.key[rows] - th_row[None, :] - qnbias[rows].astype(np.float64)[:, None]) < ref.tol(rows)
        rep.undecidable, rep.n_lists = int(und.sum()), geo.q_count
    return rep


def make_log(geo, ref, theta, qnbias):
    """(keys [n, 4], meta [n, 2]) of the groups a kernel with zero error would log, in the 32-query builds' format."""
    theta, qnbias = np.asarray(theta, dtype=np.float32), np.asarray(qnbias, dtype=np.float32)
    rows = np.arange(geo.q_begin, geo.q_begin + geo.q_count)
    n_pad = geo.n_ytiles * TILE
    k32 = np.full((geo.q_count, n_pad), -np.inf, dtype=np.float32)
    k32[:, :geo.n_i] = ref.key[rows].astype(np.float32)
    g = k32.reshape(geo.q_count, n_pad // 4, 4)                       # group G = rows 4 G .. 4 G + 3
    G = np.arange(n_pad // 4)
    tile, within = (4 * G) // TILE, (4 * G) % TILE
    with np.errstate(invalid="ignore", over="ignore"):
        cthr = (qnbias[rows][:, None] + theta[tile * TILE][None, :]).astype(np.float32)
    q, gi = np.nonzero(g.max(axis=2) >= cthr)
    tg = tile[gi] * 16 + (within[gi] >> 5) * 4 + ((within[gi] >> 3) & 3)
    lane = (rows[q] & 31) + 32 * ((within[gi] >> 2) & 1)
    meta = np.stack([(tg << 6) | lane, rows[q]], axis=1).astype(np.int32)
    return g[q, gi].copy(), meta
