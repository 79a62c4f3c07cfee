"""The checkers of tests/sweep_restate.py on lists and logs built from the reference keys themselves, on the data of
tests/test_gpu_sweep_direct.py (300 query rows, 3 109 index rows, standard normal): they accept what meets the contract, and they reject
every mutation a lossy sweep could leave behind -- the entry of rank K'/2 replaced by the row of rank K' + 1 (a dropped candidate), a
duplicated id, an id of another range or lane half, a pad-row id, a key off by four tolerances, a qualifying group missing from the log,
a group logged twice.  The dropped candidate must be seen in EVERY list at every width the GPU module sweeps.

Undecidable rows -- rows outside a list whose reference key lies within the tolerance of the list's smallest key -- are where the check
cannot say anything.  They are a property of the data and the tolerance, not of the kernels: at most K'/16 + 1 per list on average, or the
GPU module's check is empty and this module fails.  (Largest values on this data: d = 2048, K' = 16 over one range ~0.7 per list,
K' = 128 ~3.9.)"""
import numpy as np
import pytest

from tests import sweep_restate as S

H_DIMS = S.NARROW + S.WIDE + S.XWIDE


def _geometry(tier, KP, n_ranges, q_begin=0, q_count=S.N_Q):
    """The layout kz_plan_pass gives one launch with `n_ranges` forced ranges: one region, every query tile of the rows."""
    qt0 = q_begin // S.TILE
    n_qtiles = (q_begin + q_count - 1) // S.TILE - qt0 + 1
    n_yt = (S.N_I + S.TILE - 1) // S.TILE
    length = (n_yt + n_ranges - 1) // n_ranges
    pieces = (n_yt + length - 1) // length
    halves, contig = (2, 0) if tier == S.TIER_F32 else ((1, 0) if tier == S.TIER_BF else (1, 1))
    return S.Geometry(tier, KP, [n_qtiles], [pieces], halves, contig, qt0, n_ranges, S.N_I, q_begin, q_count)


_REFS = {}


def _ref(tier, d):
    if (tier, d) not in _REFS:
        X, Y = S.data(d)
        q_ops, y_ops, bias, q_bias = S.cpu_images(tier, X, Y)
        _REFS.clear()   # (one at a time: 7 MB each, 32 widths)
        _REFS[(tier, d)] = (S.reference(tier, d, q_ops, y_ops, bias, S.N_Q, S.N_I), q_bias)
    return _REFS[(tier, d)]


def _drop_candidate(geo, ref, keys, ids):
    """In every list: the entry of rank K'/2 replaced by the domain's row of rank K' + 1 (and its key)."""
    keys, ids = keys.copy(), ids.copy()
    off = geo.offsets()
    for piece in range(geo.n_pieces):
        for h in range(geo.lists):
            dom = np.flatnonzero(geo.domain(piece, h))
            sub = ref.key[geo.q_begin:geo.q_begin + geo.q_count][:, dom]
            nxt = np.argsort(-sub, axis=1, kind="stable")[:, geo.KP]
            o = off[:, piece, h, :]
            pos = np.argsort(-keys[o], axis=1, kind="stable")[:, geo.KP // 2 - 1]
            at = o[np.arange(geo.q_count), pos]
            keys[at] = sub[np.arange(geo.q_count), nxt].astype(np.float32)
            ids[at] = dom[nxt]
    return keys, ids


def _lists_case(tier, d, KP, n_ranges):
    ref, _ = _ref(tier, d)
    geo = _geometry(tier, KP, n_ranges)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list)
    rep = S.check_lists(keys, ids, geo, ref)
    rep.assert_ok(f"reference lists, tier {tier}, d = {d}, K' = {KP}, {n_ranges} ranges")
    assert rep.n_lists == S.N_Q * geo.n_pieces * geo.lists
    und = rep.und_per_list()
    assert und <= KP / 16 + 1, f"tier {tier}, d = {d}, K' = {KP}: {und:.2f} undecidable rows per list: the check is empty on this data"
    mk, mi = _drop_candidate(geo, ref, keys, ids)
    bad = S.check_lists(mk, mi, geo, ref)
    assert "outside" in bad.codes()
    # (float32 operands: the two half lists of a range prune with the larger of their thresholds, so the half with the smaller minimum
    #  may lawfully miss a row below the other half's minimum -- the drop must be seen in the half list with the larger one)
    seen = bad.bad_lists.any(axis=2) if tier == S.TIER_F32 else bad.bad_lists
    assert seen.all(), f"tier {tier}, d = {d}, K' = {KP}: a dropped candidate goes unseen in {int((~seen).sum())} lists"
    return und


@pytest.mark.parametrize("d", H_DIMS)
def test_fp16_reference_lists_pass_and_a_dropped_candidate_is_seen_in_every_list(d):
    _lists_case(S.TIER_H, d, 16, 3)
    _lists_case(S.TIER_H, d, 16, 1)
    _lists_case(S.TIER_H, d, 128, 1)
    _lists_case(S.TIER_H, d, 128, 3)


@pytest.mark.parametrize("d", [32, 200, 384])
@pytest.mark.parametrize("tier", [S.TIER_BF, S.TIER_F32])
def test_other_tiers_reference_lists_pass_and_a_dropped_candidate_is_seen(tier, d):
    for KP, n_ranges in ((16, 1), (16, 3), (128, 1), (128, 3)):
        _lists_case(tier, d, KP, n_ranges)


@pytest.mark.parametrize("KP", [32, 64])
def test_middle_list_lengths_and_a_row_range_off_the_first_tile(KP):
    ref, _ = _ref(S.TIER_H, 64)
    geo = _geometry(S.TIER_H, KP, 3, q_begin=130, q_count=150)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list)
    S.check_lists(keys, ids, geo, ref).assert_ok("rows 130 .. 279")
    mk, mi = _drop_candidate(geo, ref, keys, ids)
    assert S.check_lists(mk, mi, geo, ref).bad_lists.all()


def _one(geo, piece=0, h=0, q=7):
    return geo.offsets()[q, piece, h, :]


@pytest.mark.parametrize("tier", [S.TIER_H, S.TIER_BF, S.TIER_F32])
def test_list_mutations_are_rejected(tier):
    ref, _ = _ref(tier, 64)
    geo = _geometry(tier, 16, 3)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list)
    S.check_lists(keys, ids, geo, ref).assert_ok()

    def mutated(change):
        k, i = keys.copy(), ids.copy()
        change(k, i)
        rep = S.check_lists(k, i, geo, ref)
        assert rep.bad_lists.sum() == 1 and rep.bad_lists[7, 0, 0], "the violation belongs to one list"
        return rep.codes()

    o = _one(geo)

    def dup(k, i):
        i[o[3]], k[o[3]] = i[o[5]], k[o[5]]
    assert "dup" in mutated(dup)

    def other_range(k, i):   # (the best row of range 1, with its own key)
        o1 = _one(geo, piece=1)
        i[o[3]], k[o[3]] = i[o1[0]], k[o1[0]]
    assert "domain" in mutated(other_range)

    if tier == S.TIER_F32:
        def other_half(k, i):
            o1 = _one(geo, h=1)
            i[o[3]], k[o[3]] = i[o1[0]], k[o1[0]]
        assert "domain" in mutated(other_half)

    def pad_row(k, i):
        i[o[3]] = S.N_I + 5
    assert "id" in mutated(pad_row)

    def negative(k, i):
        i[o[3]] = -2
    assert "id" in mutated(negative)

    def key_off(k, i):
        k[o[3]] = np.float32(k[o[3]] + 4.0 * ref.tol([7])[0, i[o[3]]])
    assert "key" in mutated(key_off)

    def unwritten(k, i):
        k[o[3]], i[o[3]] = np.nan, -1
    assert {"start", "outside"} <= mutated(unwritten)


def test_seeded_lists():
    ref, _ = _ref(S.TIER_H, 64)
    geo = _geometry(S.TIER_H, 16, 1)
    floor = S.rank_floor(ref, 32)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list, floor)
    rep = S.check_lists(keys, ids, geo, ref, floor)
    rep.assert_ok("seeded reference lists")
    off = geo.offsets()
    assert (ids[off] >= 0).all()   # (a floor at rank 32: the 16 best all lie above it -- the lists are full)
    floor = S.rank_floor(ref, 8)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list, floor)
    S.check_lists(keys, ids, geo, ref, floor).assert_ok("lists with floor entries")
    assert ((ids[off[0::2, 0, 0]] >= 0).sum(axis=1) == 7).all() and (ids[off[1::2]] >= 0).all()
    o = off[0, 0, 0]
    hole = int(np.flatnonzero(ids[o] < 0)[0])
    k2 = keys.copy()
    k2[o[hole]] = -np.inf   # (an empty entry of a seeded list that lost its floor)
    assert "start" in S.check_lists(k2, ids, geo, ref, floor).codes()
    k2, i2 = keys.copy(), ids.copy()
    below = int(np.argsort(-ref.key[0])[40])   # (a row below the floor, entered with its own key)
    k2[o[hole]], i2[o[hole]] = np.float32(ref.key[0, below]), below
    assert "floor" in S.check_lists(k2, i2, geo, ref, floor).codes()
    # the range re-search form: every list starts -- and stays -- at +inf
    inf = np.full_like(floor, np.inf)
    keys, ids = S.make_lists(geo, ref, geo.lay.n_list, inf)
    assert (ids == -1).all()
    S.check_lists(keys, ids, geo, ref, inf).assert_ok("lists at +inf")


@pytest.mark.parametrize("form", ["shared", "range"])
def test_log_checker(form):
    ref, q_bias = _ref(S.TIER_H, 64)
    geo = _geometry(S.TIER_H, 16, 1)
    theta, qnbias = S.shared_thresholds(ref, q_bias) if form == "shared" else S.range_thresholds(ref)[:2]
    lk, lm = S.make_log(geo, ref, theta, qnbias)
    n = len(lk)
    assert n > 10 * S.N_Q, "the thresholds leave the log nearly empty"
    cap = n + 100
    rep = S.check_log(lk, lm, n, cap, geo, ref, theta, qnbias)
    rep.assert_ok(f"reference log, {form} form")
    assert rep.und_per_list() <= 2.0, f"{rep.und_per_list():.2f} undecidable pairs per query"
    # one qualifying group removed: the group of the pair furthest above its threshold
    tile = S.decode_meta(lm)[2]
    with np.errstate(invalid="ignore"):
        margin = lk.max(axis=1).astype(np.float64) - (qnbias[lm[:, 1]].astype(np.float64) + theta[tile * S.TILE])
    g = int(np.argmax(margin))
    keep = np.arange(n) != g
    assert "missing" in S.check_log(lk[keep], lm[keep], n - 1, cap, geo, ref, theta, qnbias).codes()
    # one group twice
    twice = np.concatenate([np.arange(n), [g]])
    assert S.check_log(lk[twice], lm[twice], n + 1, cap, geo, ref, theta, qnbias).codes() == {"dup"}
    # a key off by four tolerances; a group below the threshold; an entry of no query row
    k2 = lk.copy()
    y, row0, _ = S.decode_meta(lm[g:g + 1])
    k2[g, 0] += np.float32(4.0 * ref.tol([int(y[0])])[0, int(row0[0])])
    assert "key" in S.check_log(k2, lm, n, cap, geo, ref, theta, qnbias).codes()
    low = int(np.argmin(ref.key[5]))
    m2 = np.concatenate([lm, [[((low // S.TILE * 16 + (low % S.TILE >> 5) * 4 + ((low % S.TILE >> 3) & 3)) << 6) | (5 + 32 * ((low >> 2) & 1)), 5]]]).astype(np.int32)
    r0 = low & ~3
    k2 = np.concatenate([lk, [ref.key[5, r0:r0 + 4].astype(np.float32)]])
    assert "test" in S.check_log(k2, m2, n + 1, cap, geo, ref, theta, qnbias).codes()
    m2 = lm.copy()
    m2[g, 1] = 3 * S.TILE
    assert "where" in S.check_log(lk, m2, n, cap, geo, ref, theta, qnbias).codes()
    # overflow: the counter says so, the entries that are there are still judged
    rep = S.check_log(lk[:64], lm[:64], n, 64, geo, ref, theta, qnbias)
    assert rep.codes() == {"overflow"}
    assert S.check_log(lk[:64] * 0, lm[:64], n, 64, geo, ref, theta, qnbias).codes() >= {"overflow", "key"}
