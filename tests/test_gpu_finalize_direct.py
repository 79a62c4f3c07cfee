"""The finalize kernels (kz_finalize_query in kiez_amd/csrc/kz_knn_finalize.h: rank select for M <= 64, radix select beyond;
kz_finalize_query_wide in kz_knn_fin_wide.h) on candidate lists WRITTEN BY THE TEST, through the hook kz_selftest_finalize -- the
product's parameter fill and launcher, nothing restated in C -- against tests/finalize_restate.py.

Why directly: behind a real sweep the lists come from a correct first pass on benign data, a true neighbour is practically never
outside them, and a certification that is too lax (a bound left out, a cut that is not counted, eps for 2 eps, <= for <) changes no
answer.  Here one launch carries one scenario per query row, each built so that ONE term of the bound decides with a margin of half an
eps_q (tests/finalize_restate.py: SCENARIOS), and the property cases run the first pass's contract with perturbed keys for all index
rows (property_rows): what the kernel certifies must be the whole index's float64 top-k.

Shapes: 2 048 index rows, 200 query rows, 197 of them per launch from local row 2 at list row 3 (two query tiles = two regions with
different numbers of ranges = two launches, the smaller one on the second stream).  eps_q is set to about 1e-3 of a query's key spread
(gamma on the float32 tier, the context's eps_scale on the fp16 tier), so a quarter of an eps is ~1e9 round-offs of a key.

What is asserted, per row: the verdict is the restatement's wherever its |margin| >= 0.25 (scenarios: every row, and it is what the
scenario was built for; property cases: >= 0.05, at most 5 % of the rows inside, 20 % .. 80 % uncertified); indices equal; distances
and fail_tau bit-equal to kz_pair_values on the same pairs (with scikit-learn's dtype rule applied), which lie within (d + 8) 2^-53
(|q| + |y|)^2 of a math.fsum evaluation; the launch's maximal error ratio equals the restatement's; the build the launcher chose is
the one the case names.

Not reachable at these shapes (open): the wide kernel's cosine re-rank WITHOUT the normalised float64 rows (kz_matrix_norm64 only
declines an index of more than 8 GB).
"""
import ctypes as C

import numpy as np
import pytest

from tests import finalize_restate as R
from tests import half_inputs as H

pytestmark = pytest.mark.gpu

SQN, STATS, MU, SCALE, ROWQ, DMAX = 0, 2, 7, 8, 11, 12   # KZ_IMG_* of kz_selftest_image
N_I, N_Q, Q_BEGIN, LIST_ROW0, Q_COUNT = 2048, 200, 2, 3, R.PROPERTY_ROWS
_F, _I, _L, _D = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


class Fin(C.Structure):   # kz_selftest_fin, include/kiez_amd.h
    _fields_ = [("k", C.c_int32), ("exclude_self", C.c_int32), ("tier", C.c_int32), ("KP", C.c_int32), ("KSEL", C.c_int32),
                ("n_regions", C.c_int32), ("halves", C.c_int32), ("contig", C.c_int32), ("dual_col", C.c_int32), ("n_idx_map", C.c_int32),
                ("qt_end", C.c_int32 * 8), ("pieces", C.c_int32 * 8), ("gamma", C.c_double),
                ("q_begin", C.c_int64), ("q_count", C.c_int64), ("list_row0", C.c_int64), ("n_list", C.c_int64),
                ("h_key", _F), ("h_idx", _I), ("h_self_ids", _L), ("h_list_floor", _F), ("h_excl_floor", _F), ("h_idx_map", _I),
                ("h_row_map", _I), ("h_out_dist", _D), ("h_out_ind", _L), ("h_fail_list", _I), ("h_fail_tau", _D),
                ("n_fail", C.c_int32), ("build", C.c_int32), ("err_ratio", C.c_double)]


_HIP_ERROR = []   # a runtime error of the library in one test: the tests behind it touch the device no more


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


def _matrix(x32, elem, metric, misaligned=False):
    """(device matrix, the stored values in float64).  misaligned: float32 rows borrowed 4 bytes off a 16-byte boundary."""
    N, ctx = _native()
    if elem in H.HALF_ELEMS:
        dev, x64 = H.round_to(x32, elem)
        return N.DeviceMatrix(ctx, dev, metric, elem=elem), x64
    x = np.ascontiguousarray(x32, dtype=elem)
    if misaligned:
        flat = np.zeros(x.size + 1, dtype=np.float32)
        flat[1:] = x.ravel()
        buf = ctx.to_device(flat)
        assert buf.ptr.value % 16 == 0
        return N.DeviceMatrix(ctx, None, metric, device_ptr=buf.ptr.value + 4, shape=x.shape, dtype=np.float32, borrow=True, keepalive=buf), x.astype(np.float64)
    return N.DeviceMatrix(ctx, x, metric), x.astype(np.float64)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _launch(case, qm, im, lay, keys, idx, *, gamma=0.0, self_ids=None, list_floor=None, excl_floor=None, idx_map=None, row_map=None):
    """One call of the hook: dict(failed {output row: tau}, dist, ind, ratio, build)."""
    N, ctx = _native()
    t = Fin()
    t.k, t.exclude_self, t.tier, t.KP, t.KSEL = case.k, case.exclude_self, case.tier, case.KP, case.KSEL
    t.n_regions, t.halves, t.contig, t.dual_col = len(lay.qt_end), lay.halves, lay.contig, case.dual_col
    for r in range(len(lay.qt_end)):
        t.qt_end[r], t.pieces[r] = lay.qt_end[r], lay.pieces[r]
    t.gamma, t.q_begin, t.q_count, t.list_row0, t.n_list = gamma, Q_BEGIN, Q_COUNT, LIST_ROW0, len(keys)
    out_rows = qm.shape[0] if row_map is not None else Q_COUNT
    dist, ind = np.zeros((out_rows, case.k)), np.zeros((out_rows, case.k), dtype=np.int64)
    fail, tau = np.zeros(Q_COUNT, dtype=np.int32), np.zeros(Q_COUNT)
    hold = [np.ascontiguousarray(a) if a is not None else None for a in (keys, idx, self_ids, list_floor, excl_floor, idx_map, row_map)]
    t.h_key, t.h_idx, t.h_self_ids = _ptr(hold[0], _F), _ptr(hold[1], _I), _ptr(hold[2], _L)
    t.h_list_floor, t.h_excl_floor, t.h_idx_map, t.h_row_map = _ptr(hold[3], _F), _ptr(hold[4], _F), _ptr(hold[5], _I), _ptr(hold[6], _I)
    t.n_idx_map = 0 if idx_map is None else len(idx_map)
    t.h_out_dist, t.h_out_ind, t.h_fail_list, t.h_fail_tau = _ptr(dist, _D), _ptr(ind, _L), _ptr(fail, _I), _ptr(tau, _D)
    try:
        N._check(ctx.lib.kz_selftest_finalize(ctx.handle, qm.handle, im.handle, C.byref(t)), "kz_selftest_finalize")
    except RuntimeError as e:
        _HIP_ERROR.append(str(e))
        raise
    assert 0 <= t.n_fail <= Q_COUNT and (fail[t.n_fail:] == -1).all() and len(set(fail[:t.n_fail])) == t.n_fail
    return dict(failed={int(r): float(v) for r, v in zip(fail[:t.n_fail], tau[:t.n_fail])}, dist=dist, ind=ind, ratio=t.err_ratio, build=t.build)


class Units:
    """What the kernels read of the two matrices, read back from the device: per query row qref and eps per unit of the case's free
    factor (gamma / eps_scale), the key scale."""

    def __init__(self, case, qm, im):
        cosine = case.metric == "cosine"
        self.q_sqn = _read(qm, SQN, np.float64)
        y_max = float(_read(im, STATS, np.float64)[0])
        n = qm.shape[0]
        if case.tier == 2:
            rowq = _read(qm, ROWQ, np.float64, partner=im).reshape(n, 3)
            dmax, hs = _read(im, DMAX, np.float64), _read(im, SCALE, np.float64)
            self.scale, self.qref = float(hs[1]), rowq[:, 0].copy()
            self.unit = np.asarray([R.eps_tier2(rowq[q], dmax, y_max, self.q_sqn[q], case.d, 1.0, cosine, case.dual_col) for q in range(n)])
            self.unit_pair = [np.asarray([R.eps_tier2(rowq[q], dmax, y_max, self.q_sqn[q], case.d, 1.0, cosine, f) for q in range(n)]) for f in (0, 1)]
        else:
            self.scale, self.qref = 1.0, self.q_sqn
            self.unit = np.asarray([R.eps_tier0(1.0, float(self.q_sqn[q]) if cosine else float(np.sqrt(self.q_sqn[q])), y_max, cosine) for q in range(n)])


def _maps(case, rng, n_i=N_I):
    """idx_map: list entry r stands for index row idx_map[r] (64 more entries map to -1: empty); row_map: image row -> matrix row."""
    if not case.maps:
        return None, None, None
    idx_map = np.concatenate([rng.permutation(n_i), np.full(64, -1)]).astype(np.int32)
    inv = np.empty(n_i, dtype=np.int32)
    inv[idx_map[:n_i]] = np.arange(n_i, dtype=np.int32)
    return idx_map, inv, rng.permutation(N_Q).astype(np.int32)


def _run_and_check(case, qm, im, Xs, Ys, V, units, factor, rows, expects, band, brute):
    """Launch the rows (local q -> dict(keys, ids, list_floor, excl_floor, self_id, eps)) and hold every row against the restatement."""
    N, ctx = _native()
    N_I = len(Ys)
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    which = "wide" if case.build == R.BUILD_WIDE else "generic"
    rng = np.random.RandomState(len(case.name))
    lay = case.layout()
    idx_map, inv, row_map = _maps(case, rng, N_I)
    keys = np.full(lay.n_list, np.nan, dtype=np.float32)
    idx = np.full(lay.n_list, -1, dtype=np.int32)
    qrow = [int(row_map[Q_BEGIN + q]) if row_map is not None else Q_BEGIN + q for q in range(Q_COUNT)]
    list_floor = np.full(N_Q, -np.inf, dtype=np.float32) if case.floor else None
    excl_floor = np.full(N_Q, -np.inf, dtype=np.float32) if case.dual else None
    self_ids = np.zeros(Q_COUNT, dtype=np.int64) if case.self_ids else None
    for q, row in enumerate(rows):
        off = lay.offsets(LIST_ROW0 + q)
        ids = row["ids"]
        if inv is not None:   # (empty places: -1, or an entry of the map that holds -1)
            ids = np.where(ids >= 0, inv[np.maximum(ids, 0)], np.where(rng.rand(len(ids)) < 0.5, -1, N_I + rng.randint(64, size=len(ids)))).astype(np.int32)
        keys[off], idx[off] = row["keys"], ids
        if row.get("list_floor") is not None:
            list_floor[Q_BEGIN + q] = row["list_floor"]      # (by image row)
        if row.get("excl_floor") is not None:
            excl_floor[qrow[q]] = row["excl_floor"]          # (by matrix row)
        if self_ids is not None:
            self_ids[q] = row["self_id"]
    if tier_h:
        ctx.set_option("eps_scale", factor)
    try:
        got = _launch(case, qm, im, lay, keys, idx, gamma=factor, self_ids=self_ids, list_floor=list_floor, excl_floor=excl_floor,
                      idx_map=idx_map, row_map=row_map)
    finally:
        ctx.set_option("eps_scale", 1.0)
    assert got["build"] == case.build, f"the launcher chose build {got['build']}"
    f32_rows = case.elem == "float32"
    res, n_band, n_fail, worst = [], 0, 0, 0.0
    pairs = np.full((N_Q, case.k + 1), -1, dtype=np.int64)   # the pairs whose values kz_pair_values is asked for: outputs, tau's candidate
    for q, row in enumerate(rows):
        qr = qrow[q]
        out = qr if row_map is not None else q
        r = R.finalize_row(row["keys"], row["ids"], V[qr], KP=case.KP, KS=case.KS, k=case.k, exclude_self=case.exclude_self,
                           self_row=row["self_id"] if self_ids is not None else qr, n_i=N_I, eps=row["eps"], scale=units.scale, qref=units.qref[qr],
                           cosine=cosine, tier_h=tier_h, list_floor=row.get("list_floor") if case.floor else None,
                           excl_floor=(row.get("excl_floor") if row.get("excl_floor") is not None else -np.inf) if case.dual else None,
                           metric=case.metric, f32_rows=f32_rows)
        res.append(r)
        m, failed = r["margin"][which], out in got["failed"]
        if not (which == "wide" and r["V"] < case.k_eff):   # (the wide build leaves such a row before it looks at the keys)
            worst = max(worst, r["ratio"])
        n_fail += failed
        if abs(m) < band:
            n_band += 1
        else:
            assert failed == (not r["certified"][which]), f"row {q} ({row.get('name')}): kernel {'failed' if failed else 'certified'}, margin {m}, ratio {r['ratio']}"
            if expects is not None:
                assert failed == (not expects[q]), f"row {q}: {row['name']} is built to {'certify' if expects[q] else 'fail'}"
        if failed:
            tau = got["failed"][out]
            if r["tau"][which] == np.inf:
                assert tau == np.inf, f"row {q} ({row.get('name')}): fail_tau {tau}"
            elif abs(m) >= band or not r["certified"][which]:
                pairs[qr, case.k] = r["cand"][case.k_eff - 1]
            assert (got["ind"][out] == -1).all() and np.isnan(got["dist"][out]).all(), f"row {q}: an uncertified row has outputs"
        else:
            n_out = len(r["ind"])
            assert np.array_equal(got["ind"][out, :n_out], r["ind"]) and (got["ind"][out, n_out:] == -1).all(), f"row {q} ({row.get('name')}): indices"
            pairs[qr, :n_out] = r["ind"]
            if brute:   # the whole index's top-k by (value, id), self removed as the output step removes it
                want = list(R.brute_topk(V[qr], case.k_eff))
                if case.exclude_self:
                    s = row["self_id"] if self_ids is not None else qr
                    want.pop(want.index(s) if s in want else 0)
                assert list(got["ind"][out]) == want[:case.k], f"row {q}: certified, but not the whole index's top-k"
    # distances and fail_tau: the bits of kz_pair_values on the same pairs, which lie within the round-off bound of an exact evaluation
    pv = N.pair_values(ctx, qm, 0, N_Q, im, ctx.to_device(pairs)).numpy()
    for q, row in enumerate(rows):
        qr = qrow[q]
        out = qr if row_map is not None else q
        if out in got["failed"]:
            if pairs[qr, case.k] >= 0:
                assert got["failed"][out] == pv[qr, case.k], f"row {q} ({row.get('name')}): fail_tau {got['failed'][out]} != {pv[qr, case.k]}"
                j = pairs[qr, case.k]
                exact = R.exact_value_fsum(Xs[qr], Ys[j], case.metric)
                assert abs(pv[qr, case.k] - exact) <= R.value_bound(Xs[qr], Ys[j], case.d), f"row {q}: fail_tau, value of pair ({qr}, {j})"
            continue
        n_out = int((pairs[qr, :case.k] >= 0).sum())
        want = np.asarray([R.output_distance(float(v), case.metric, f32_rows) for v in pv[qr, :n_out]])
        assert np.array_equal(got["dist"][out, :n_out].view(np.uint64), want.view(np.uint64)), f"row {q} ({row.get('name')}): distances"
        for c in range(n_out):
            j = pairs[qr, c]
            exact = R.exact_value_fsum(Xs[qr], Ys[j], case.metric)
            assert abs(pv[qr, c] - exact) <= R.value_bound(Xs[qr], Ys[j], case.d), f"row {q}: value of pair ({qr}, {j})"
    assert abs(got["ratio"] - worst) <= 1e-6 * max(worst, 1e-30), f"maximal error ratio {got['ratio']}, restated {worst}"
    return res, n_band, n_fail, got["ratio"]


def _self_id(q, row, values):
    """self_ids of a row: the best candidate (first in the output), a later one, one that is in no list; where copies of one row lie
    across the k-th place, the copy with the largest id (behind its duplicates)."""
    valid = row["ids"][row["ids"] >= 0]
    g0 = len(values) - R.N_TIES
    copies = valid[(valid >= g0) & (valid < g0 + R.N_GROUPS * R.GROUP)]
    if row.get("name") == "dup_k" and len(copies):
        return int(copies.max())
    order = valid[np.argsort(values[valid], kind="stable")]
    absent = next(j for j in range(len(values)) if j not in set(valid.tolist()))
    return int([order[0], order[min(3, len(order) - 1)], absent][q % 3]) if len(valid) else 0


def _scenario_inputs(case):
    """Matrices, exact values and units of a scenario case.  The dual cases: rows that fp16 holds exactly around a zero centre (then the
    reverse direction's extra term is a large part of eps_q), queries three times the index rows' size."""
    rng = np.random.RandomState(11)
    if case.dual:
        c0 = rng.randint(-6, 7, size=case.d) / 4.0
        A = np.concatenate([c0 + rng.randint(-6, 7, size=(N_I // 2 - 128, case.d)) / 64.0, rng.randint(-64, 65, size=(128, case.d)) / 64.0])
        Y = np.concatenate([A, -A])[rng.permutation(N_I)].astype(np.float32)
        w = rng.randn(N_Q, case.d) * 0.7
        w -= np.outer(w @ c0, c0) / float(c0 @ c0)
        X = (np.round((2.0 * c0 + 4.0 * w) * 64) / 64).astype(np.float32)
        im, Ys = _matrix(Y, case.elem, case.metric)
    else:
        Y, queries = R.scenario_data(7, N_Q, N_I, case.d, case.metric)
        im, Ys = _matrix(Y, case.elem, case.metric, case.misaligned)
        X = queries(_read(im, MU, np.float32) if case.tier == 2 and case.metric != "cosine" else None)
    qm, Xs = _matrix(X, case.elem, case.metric, case.misaligned)
    V = R.exact_values(Xs, Ys, case.metric)
    return qm, im, Xs, Ys, V, Units(case, qm, im)


def _spread_factor(case, units, V):
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    spread = np.asarray([np.ptp(R.exact_key(V[q], units.qref[q], cosine, tier_h)) for q in range(N_Q)])
    return 1e-3 * float(np.median(spread / units.unit))


@pytest.mark.parametrize("case", R.SCENARIO_CASES, ids=repr)
def test_scenarios(case):
    qm, im, Xs, Ys, V, units = _scenario_inputs(case)
    factor = _spread_factor(case, units, V)
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    rng = np.random.RandomState(5)
    _, _, row_map = _maps(case, np.random.RandomState(len(case.name)))
    rows, expects, seen = [], [], []
    if case.dual:   # (the flag's eps: this launch's; the scenario between the two bounds needs both)
        assert (units.unit_pair[1] >= 5.0 / 3.0 * units.unit_pair[0]).all(), "the reverse direction's term is too small a part of eps_q on this data"
    for q in range(Q_COUNT):
        qr = int(row_map[Q_BEGIN + q]) if row_map is not None else Q_BEGIN + q
        region = (LIST_ROW0 + q) // 128
        geom = case.geom(region)
        names = R.scenario_names(geom, has_floor=case.floor, dual=case.dual, zero_level=not cosine)
        name = names[(q + q // len(names)) % len(names)]
        eps = factor * units.unit[qr]
        pair = (factor * units.unit_pair[0][qr], factor * units.unit_pair[1][qr]) if case.dual else None
        min_gap = 200 * (case.d + 8) * 2.0 ** -53 * (np.sqrt((Xs[qr] ** 2).sum()) + np.sqrt((Ys ** 2).sum(1).max())) ** 2
        def builder(b_eps=pair[0] if name == "excl_between" else eps, qr=qr, geom=geom, q=q, min_gap=min_gap):
            return R.RowBuilder(V[qr], units.qref[qr], b_eps, units.scale, cosine, tier_h, geom, np.random.RandomState(1000 + q), min_gap=min_gap)
        row = R.scenario_or_fallback(builder, name, prefer=qr if case.exclude_self and not case.self_ids else None, eps_pair=pair)
        if row["name"] == "excl_between":
            row["expect"] = not case.dual_col
        row["eps"] = eps
        row["self_id"] = _self_id(q, row, V[qr])
        rows.append(row)
        expects.append(row["expect"])
        seen.append(row["name"])
    wanted = set(R.scenario_names(case.geom(0), has_floor=case.floor, dual=case.dual, zero_level=not cosine)) | set(
        R.scenario_names(case.geom(1), has_floor=case.floor, dual=case.dual, zero_level=not cosine))
    assert all(seen.count(name) >= 3 for name in wanted), {name: seen.count(name) for name in wanted}
    res, n_band, n_fail, ratio = _run_and_check(case, qm, im, Xs, Ys, V, units, factor, rows, expects, band=0.25, brute=False)
    assert n_band == 0, f"{n_band} rows are nearer than 0.25 eps to the edge"
    which = "wide" if case.build == R.BUILD_WIDE else "generic"
    for q, (row, r) in enumerate(zip(rows, res)):
        assert r["certified"][which] == row["expect"], f"row {q}: the restatement does not say what {row['name']} is built for (margin {r['margin'][which]})"
    if not case.dual and case.floor:
        assert 1.5 <= ratio <= 1.56   # (the rows with one key 1.52 eps off; float32 rounding of the key moves it by up to 0.02)
    print(f"finalize_direct {case.name}: build {case.build}, {n_fail} of {Q_COUNT} rows uncertified, max error ratio {ratio:.4f}")


def test_index_of_fewer_rows_than_neighbours():
    """Three index rows, k = 5, one list with three entries and no floor: the set is complete, the row is answered with three
    neighbours (generic build); with one entry missing it fails with tau = +inf."""
    case = R.Case("tiny", "float32", 8, "sqeuclidean", 0, 16, 1, 1, (1, 1), 0, 5, R.BUILD_ORDINARY, floor=False)
    N, ctx = _native()
    rng = np.random.RandomState(3)
    Y, X = rng.randn(3, 8).astype(np.float32), rng.randn(N_Q, 8).astype(np.float32)
    im, qm = N.DeviceMatrix(ctx, Y, "sqeuclidean"), N.DeviceMatrix(ctx, X, "sqeuclidean")
    V = R.exact_values(X, Y, "sqeuclidean")
    lay = case.layout()
    keys, idx = np.full(lay.n_list, -np.inf, dtype=np.float32), np.full(lay.n_list, -1, dtype=np.int32)
    for q in range(Q_COUNT):
        off = lay.offsets(LIST_ROW0 + q)
        n = 3 if q % 2 == 0 else 2
        idx[off[:n]] = rng.permutation(3)[:n]
        keys[off[:n]] = (0.5 * ((X[Q_BEGIN + q].astype(np.float64) ** 2).sum() - V[Q_BEGIN + q][idx[off[:n]]])).astype(np.float32)
    got = _launch(case, qm, im, lay, keys, idx, gamma=1e-6)
    assert got["build"] == R.BUILD_ORDINARY
    for q in range(Q_COUNT):
        if q % 2:
            assert got["failed"].get(q) == np.inf
        else:
            assert q not in got["failed"] and list(got["ind"][q]) == list(np.lexsort((np.arange(3), V[Q_BEGIN + q]))) + [-1, -1]
            assert np.isnan(got["dist"][q, 3:]).all() and not np.isnan(got["dist"][q, :3]).any()


def test_the_verdict_is_a_strict_inequality():
    """eps_q = 0 (gamma = 0) on integer data, where keys are exact in float32: the k-th candidate ties exactly with the selection's cut
    (every selected entry behind the second has the same distance) -- an outside row may tie with it too, the row must fail; with one
    selected entry further away the cut lies below the k-th key and the row is certified.  Rank select (16 entries) and radix select
    (80).  Open: the same on the wide kernel (its eps_q cannot be made zero)."""
    case = R.Case("strict", "float32", 8, "sqeuclidean", 0, 16, 1, 1, (1, 5), 0, 3, R.BUILD_ORDINARY, floor=False)
    N, ctx = _native()
    q0 = np.asarray([1, -2, 0, 3, 1, 0, -1, 2], dtype=np.float32)
    rows = [q0 + np.eye(8)[0], q0 + np.eye(8)[1] + np.eye(8)[2]]                      # squared distances 1, 2
    rows += [q0 + 2 * np.eye(8)[a] + s * np.eye(8)[b] for a in range(8) for b in range(8) if a != b for s in (1, -1)][:40]   # 5
    rows += [q0 + 2 * np.eye(8)[a] + np.eye(8)[(a + 1) % 8] - np.eye(8)[(a + 2) % 8] for a in range(8)]                    # 6
    Y, X = np.asarray(rows, dtype=np.float32), np.tile(q0, (N_Q, 1))
    im, qm = N.DeviceMatrix(ctx, Y, "sqeuclidean"), N.DeviceMatrix(ctx, X, "sqeuclidean")
    V = R.exact_values(X[:1], Y, "sqeuclidean")[0]
    assert list(V[:2]) == [1.0, 2.0] and (V[2:42] == 5.0).all() and (V[42:] == 6.0).all()
    key = (0.5 * (float((q0.astype(np.float64) ** 2).sum()) - V)).astype(np.float32)
    lay = case.layout()
    keys, idx = np.full(lay.n_list, -np.inf, dtype=np.float32), np.full(lay.n_list, -1, dtype=np.int32)
    rng = np.random.RandomState(1)
    want = {}
    for q in range(Q_COUNT):
        tied = 2 + rng.permutation(40)[:14 if q % 2 else 13]
        ids = np.concatenate([[0, 1], tied, [] if q % 2 else [42 + q % 8]]).astype(np.int32)
        off = lay.offsets(LIST_ROW0 + q)
        n_lists = len(off) // 16
        slots = np.concatenate([li * 16 + rng.permutation(16)[:(16 + n_lists - 1 - li) // n_lists] for li in range(n_lists)])[:16]
        idx[off[slots]], keys[off[slots]] = ids, key[ids]
        want[q] = [0, 1, int(tied.min())]
    got = _launch(case, qm, im, lay, keys, idx, gamma=0.0)
    assert got["build"] == R.BUILD_ORDINARY
    for q in range(Q_COUNT):
        if q % 2:
            assert got["failed"].get(q) == 5.0, f"row {q}: the k-th key EQUALS the cut, the row must fail"
        else:
            assert q not in got["failed"] and list(got["ind"][q]) == want[q], f"row {q}"


@pytest.mark.parametrize("bad", ["id", "idx_map", "row_map", "self_ids", "KP", "entries", "lds", "ksel", "tier_layout", "tier_width", "n_list", "rows",
                                 "idx_map_interleaved", "excl_with_floor", "excl_many_lists"])
def test_bad_geometry_is_refused_before_any_launch(bad):
    N, ctx = _native()
    rng = np.random.RandomState(0)
    d = 400 if bad == "tier_width" else 32   # (385 .. 496 columns: 25 .. 31 slices of 16, which no build of the fp16 kernel sweeps)
    Y, X = rng.randn(300, d).astype(np.float32), rng.randn(N_Q, d).astype(np.float32)
    im, qm = N.DeviceMatrix(ctx, Y, "sqeuclidean"), N.DeviceMatrix(ctx, X, "sqeuclidean")
    kw = dict(KP=16, halves=1, contig=1, pieces=(2, 2), KSEL=0, k=5, tier=0)
    extra = {}
    if bad == "KP":
        kw["KP"] = 48
    elif bad == "entries":
        kw.update(KP=128, pieces=(33, 1))
    elif bad == "lds":
        kw.update(KP=128, pieces=(32, 32), KSEL=1024)
    elif bad == "ksel":
        kw["KSEL"] = 3
    elif bad == "tier_layout":
        kw.update(tier=2, contig=0, halves=2)
    elif bad == "tier_width":
        kw["tier"] = 2
    elif bad == "idx_map_interleaved":   # (the wave-interleaved gather never applies the map: ids up to its length would pass the check)
        kw.update(contig=0)
    elif bad == "excl_with_floor":       # (the reverse direction's bound counts no list_floor ...
        kw.update(pieces=(1, 1))
    elif bad == "excl_many_lists":       #  ... and no second list)
        kw.update(pieces=(1, 2))
    case = R.Case("bad", "float32", d, "sqeuclidean", kw["tier"], kw["KP"], kw["halves"], kw["contig"], kw["pieces"], kw["KSEL"], kw["k"], 0, floor=False)
    lay = case.layout()
    keys, idx = np.zeros(lay.n_list + (1 if bad == "n_list" else 0), dtype=np.float32), np.full(lay.n_list + (1 if bad == "n_list" else 0), -1, dtype=np.int32)
    if bad == "id":
        idx[7] = 300
    elif bad == "idx_map":
        extra["idx_map"] = np.asarray([0, 1, 300], dtype=np.int32)
    elif bad == "idx_map_interleaved":
        extra["idx_map"] = np.arange(300, dtype=np.int32)
    elif bad == "excl_with_floor":
        extra["excl_floor"], extra["list_floor"] = np.zeros(N_Q, dtype=np.float32), np.zeros(N_Q, dtype=np.float32)
    elif bad == "excl_many_lists":
        extra["excl_floor"] = np.zeros(N_Q, dtype=np.float32)
    elif bad == "row_map":
        extra["row_map"] = np.full(N_Q, N_Q, dtype=np.int32)
    elif bad == "self_ids":
        case.exclude_self, case.self_ids = 1, True
        extra["self_ids"] = np.full(Q_COUNT, 300, dtype=np.int64)
    elif bad == "rows":
        lay = R.Layout([1], [2], 1, 1, 16)   # (one query tile: list rows 3 .. 199 do not fit)
        keys, idx = np.zeros(lay.n_list, dtype=np.float32), np.full(lay.n_list, -1, dtype=np.int32)
    with pytest.raises(ValueError, match="kz_selftest_finalize"):
        _launch(case, qm, im, lay, keys, idx, gamma=1e-6, **extra)


PROPERTY = [R.property_case(b, M) for b in R.PROPERTY_BUILDS for M in R.PROPERTY_M]


@pytest.mark.parametrize("case", PROPERTY, ids=repr)
def test_property(case):
    """Perturbed keys for all index rows, lists by the first pass's contract, random validity and floors (finalize_restate.property_rows)."""
    M = case.geom(0)[0] * case.KP
    n_i = R.property_n_i(M)
    X, Y = R.property_data(1000 + M, N_Q, n_i, case.d)
    im, Ys = _matrix(Y, case.elem, case.metric)
    qm, Xs = _matrix(X, case.elem, case.metric)
    V = R.exact_values(Xs, Ys, case.metric)
    units = Units(case, qm, im)
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    which = "wide" if case.build == R.BUILD_WIDE else "generic"
    sl = slice(Q_BEGIN, Q_BEGIN + Q_COUNT)
    K = np.stack([R.exact_key(V[q], units.qref[q], cosine, tier_h) for q in range(Q_BEGIN, Q_BEGIN + Q_COUNT)])
    factor, rows = R.property_rows(K, units.unit[sl], units.scale, case.geom(0), M, which)
    rng = np.random.RandomState(M)
    for q, row in enumerate(rows):
        row["list_floor"] = row["list_floor"] if row["list_floor"] > -np.inf else None
        row["self_id"] = int(rng.randint(n_i)) if q % 3 else int(R.brute_topk(V[Q_BEGIN + q], 1)[0])
    res, n_band, n_fail, ratio = _run_and_check(case, qm, im, Xs, Ys, V, units, factor, rows, None, band=0.05, brute=True)
    assert n_band <= 0.05 * Q_COUNT, f"{n_band} rows within 0.05 eps of the edge"
    assert 0.2 * Q_COUNT <= n_fail <= 0.8 * Q_COUNT, f"{n_fail} of {Q_COUNT} rows uncertified"
    assert ratio <= 0.95
    print(f"finalize_direct {case.name}: build {case.build}, {n_fail} of {Q_COUNT} rows uncertified, {n_band} at the edge, max error ratio {ratio:.4f}")
