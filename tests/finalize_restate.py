"""The finalize step of kz_knn (kiez_amd/csrc/kz_knn_finalize.h, kz_knn_fin_wide.h) restated in float64 numpy:
where a query's list entries lie, the rounding bound eps_q, the selection of KS candidates, the bound B of everything outside them,
the 2 eps re-rank window, the verdict, fail_tau and the output step.  Written from the contract, one row at a time, with no regard
for speed: tests/test_finalize_restate.py holds it against a brute force over the whole index that shares none of it, and
tests/test_gpu_finalize_direct.py holds the three kernel builds against it.

The contract, for one query.  Every index row j has an approximate key a_j with |a_j scale - key_j| <= eps_q, where key_j is the exact
key (euclidean family: (qref - d2_j) / 2; cosine on float32 / split-bf16 operands: 1 - dist_j; cosine on fp16 operands: (qref - 2 dist_j) / 2).
The lists hold some of the rows.  Of the valid entries (id >= 0) the KS best by (key descending, id ascending) are SELECTED; of those, the ones
whose key is within 2 eps_q of the k_eff-th best selected key are RE-RANKED exactly.  B bounds the approximate key of every row that is
not re-ranked; the row is certified iff  B scale + eps_q < exact key of the k_eff-th best re-ranked candidate  (strictly), or, when nothing
bounds the outside at all (B = -inf: no list was full, nothing was cut, no floor), iff the candidates are min(k_eff, n_i) at least.

Where the builds differ (both sound):
  * exactly KS valid entries: the generic build counts the smallest selected key into B (V == KS), the wide build knows that the
    selection left nothing behind;
  * more exact ties at the k_eff-th place than KS: the wide build fails the row (tau = +inf), the generic one orders all of them;
  * the wide build fails a row with fewer than k_eff valid entries at once (the generic one only when something bounds the outside
    or the index has more rows than the row has candidates).
"""
import math

import numpy as np

TILE = 128
LSTRIDE = 64
FIN_MAXM = 4096
FIN_LDS_BYTES = 160 * 1024
BUILD_ORDINARY, BUILD_TWO_LOADS, BUILD_MANY, BUILD_WIDE = range(4)
INF = float("inf")


# ---- list layout ----------------------------------------------------------------------------------------------------------------------
class Layout:
    """Regions of query tiles [qt_end[r-1], qt_end[r]) with pieces[r] index ranges each, `halves` lists per (query, range); contig: a
    query's lists are one run of pieces x KP entries, else the wave-interleaved blocks [KP][64] of 32 queries x 2 lane halves."""

    def __init__(self, qt_end, pieces, halves, contig, KP):
        self.qt_end, self.pieces, self.halves, self.contig, self.KP = list(qt_end), list(pieces), halves, contig, KP
        self.base, total, t0 = [], 0, 0
        for t1, p in zip(self.qt_end, self.pieces):
            self.base.append(total)
            total += (t1 - t0) * TILE * p * (KP if contig else 2 * KP)
            t0 = t1
        self.n_list = total

    def region(self, list_row):
        qt = list_row // TILE
        r = 0
        while r + 1 < len(self.qt_end) and qt >= self.qt_end[r]:
            r += 1
        return r

    def entries(self, list_row):
        """M = pieces x halves x KP entries of a list row."""
        return self.pieces[self.region(list_row)] * self.halves * self.KP

    def contig_off(self, list_row, piece):
        r = self.region(list_row)
        row0 = self.qt_end[r - 1] * TILE if r else 0
        return self.base[r] + ((list_row - row0) * self.pieces[r] + piece) * self.KP

    def wave_base(self, list_row, piece):
        r = self.region(list_row)
        row0 = self.qt_end[r - 1] * TILE if r else 0
        return self.base[r] + (((list_row - row0) >> 5) * self.pieces[r] + piece) * self.KP * LSTRIDE

    def offsets(self, list_row):
        """Element offsets of the row's entries in the order the kernels number them: range, lane half, list entry."""
        KP, out = self.KP, []
        for piece in range(self.pieces[self.region(list_row)]):
            for h in range(self.halves):
                for e in range(KP):
                    if self.contig:
                        out.append(self.contig_off(list_row, piece) + h * KP + e)   # (halves = 1 in this layout)
                    else:
                        out.append(self.wave_base(list_row, piece) + e * LSTRIDE + h * 32 + list_row % 32)
        return np.asarray(out, dtype=np.int64)


def fin_wave_bytes(max_m, KS, wide=False):
    return ((max_m * 8 + KS * (20 if wide else 28)) + 15) & ~15


# ---- rounding bounds ------------------------------------------------------------------------------------------------------------------
def eps_tier0(gamma, q_norm, y_max, cosine):
    """float32 / split-bf16 operands: gamma (ymax^2 / 2 + |q| ymax); cosine: 1.001 gamma; +inf below the 1e-30 scale."""
    if cosine:
        return gamma * 1.001
    scale = 0.5 * y_max * y_max + q_norm * y_max
    return INF if scale < 1e-30 else gamma * scale


def gamma_acc_h(d):
    d_pad = (d + 15) // 16 * 16
    return 2.0 * (d_pad + 16) * 2.0 ** -24


def eps_tier2(rowq, dmax, y_max, q_sqn, d, eps_mult, cosine, dual_col=False):
    """fp16 operands: rowq = (|q_c|^2, |q_h|, |q_c - q_h|) of the query's image row, dmax = (max |y_h|, max |y_c - y_h|,
    max |y_c|^2) of the index image, y_max the index's largest raw row norm, q_sqn the query's raw squared norm."""
    qc2, qh, qr = (float(x) for x in rowq)
    Yh, Ry, Yc2 = (float(x) for x in dmax)
    qc, yc = math.sqrt(qc2), math.sqrt(Yc2)
    raw2 = 2.0 if cosine else q_sqn + y_max * y_max
    g = gamma_acc_h(d)
    e = eps_mult * (qr * Yh + qh * Ry + qr * Ry + g * (0.5 * Yc2 + qh * Yh) + 2.0 ** -23 * (qc + yc) ** 2 + 1e-12 * (0.5 * Yc2 + qc2) + 1e-14 * raw2)
    if dual_col:
        e += eps_mult * (g * 0.5 * qc2 + 2.0 ** -23 * (0.5 * Yc2 + 0.5 * qc2 + qh * Yh))
    return e


def exact_key(v, qref, cosine, tier_h):
    """The exact key of a candidate from its exact ranking value v (squared distance / cosine distance)."""
    if cosine and not tier_h:
        return 1.0 - v
    return 0.5 * (qref - (2.0 * v if cosine else v))


def output_distance(v, metric, f32_rows):
    """What kz_knn returns for the ranking value v: scikit-learn's conversions (euclidean on float32 rows: float32 argument, float64
    sqrt, float32 result)."""
    if metric != "euclidean":
        return v
    if f32_rows:
        return float(np.float32(np.sqrt(np.float64(np.float32(v)))))
    return math.sqrt(v)


# ---- one row --------------------------------------------------------------------------------------------------------------------------
def _sel_order(keys, ids):
    """Indices of the valid entries by (key descending, id ascending); -0 = +0."""
    valid = np.flatnonzero(ids >= 0)
    k = keys[valid].astype(np.float64) + 0.0   # (-0 + 0 = +0)
    return valid[np.lexsort((ids[valid], -k))]


def finalize_row(keys, ids, values, *, KP, KS, k, exclude_self, self_row, n_i, eps, scale=1.0, qref=0.0, cosine=False, tier_h=False,
                 list_floor=None, excl_floor=None, metric="sqeuclidean", f32_rows=True):
    """One query.  keys (float32) / ids (after idx_map; < 0: empty) are the row's entries in the kernels' order (lists of KP consecutive
    entries); values[j] = the exact float64 ranking value of index row j.  Returns a dict:
      V, Vr            valid selected / re-ranked candidates
      B                {"generic", "wide"}: the bound of everything that is not re-ranked, in list-key units.  With excl_floor (the reverse
                       direction of a shared sweep: one list of KP entries, KS = KP, no list_floor -- nothing else is launched with it and
                       the hook refuses anything else) the generic bound is excl_floor and, of a full list, the cut
      margin           {build: (key_k - eps - B scale) / eps}; +inf where nothing bounds the outside and the set is complete, -inf where
                       the row cannot be certified whatever the keys (too few candidates, an infinite floor, too many ties)
      certified        {build: bool}
      tau              {build: fail_tau of an uncertified row}
      ratio            max |key~ scale - key| / eps over the re-ranked candidates with v > 0
      ind, dist        the k output entries (of a certified row)
      cand             ids of the re-ranked candidates by (value, id)"""
    keys = np.asarray(keys, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    k_eff = k + (1 if exclude_self else 0)
    order = _sel_order(keys, ids)
    n_valid = len(order)
    sel = order[:KS]
    V = len(sel)
    skey = keys[sel].astype(np.float64)
    # everything outside the selection
    # (a full list may have evicted rows at or below its smallest key.  With KS = KP a full list implies a full selection whose cut is at
    #  least as large: the generic build counts the lists' minima only when KS > KP; the wide build, where KS > KP always, counts them always)
    full_min = -INF
    for l0 in range(0, len(keys), KP):
        if (ids[l0:l0 + KP] >= 0).all():
            full_min = max(full_min, float(keys[l0:l0 + KP].min()))
    floor_b = -INF if list_floor is None else float(list_floor)
    piece, piece_w = max(floor_b, full_min if KS > KP else -INF), max(floor_b, full_min)
    cut =float(skey[-1]) if V else -INF
    # the re-rank window
    if V > k_eff and eps < INF:
        thr = skey[k_eff - 1] * scale - 2.0 * eps
        inside = skey * scale >= thr
    else:
        inside = np.ones(V, dtype=bool)
    left_max = float(skey[~inside].max()) if (~inside).any() else -INF
    rr = sel[inside]
    Vr = len(rr)
    rid = ids[rr]
    rv = np.asarray([values[j] for j in rid], dtype=np.float64)
    eo = np.lexsort((rid, rv))
    cand, cval = rid[eo], rv[eo]
    ratio = 0.0
    if 0.0 < eps < INF:
        for a, v in zip(keys[rr].astype(np.float64), rv):
            if v > 0.0:
                ratio = max(ratio, abs(a * scale - exact_key(v, qref, cosine, tier_h)) / eps)
    key_k = exact_key(cval[k_eff - 1], qref, cosine, tier_h) if Vr >= k_eff else None
    B, margin, tau = {}, {}, {}
    # generic build (kz_finalize_query)
    b = piece
    if excl_floor is not None:
        # the reverse direction of a shared sweep: ONE list of KP entries, all of them selected, and no list_floor -- the only geometry
        # the product launches with excl_floor, and the only one the hook accepts with it.  The kernel's bound there is excl_floor and,
        # of a full list, the cut; that is the contract.
        assert list_floor is None and KS == KP and len(keys) == KP, "excl_floor goes with one list of KP entries and no list_floor"
        b = float(excl_floor)
        if V == KP:
            b = max(b, cut)
    elif V == KS:
        b = max(b, cut)
    b = max(b, left_max)
    B["generic"] = b
    if b == -INF and excl_floor is None:
        margin["generic"] = INF if V >= min(k_eff, n_i) else -INF
    elif V < k_eff or b == INF:
        margin["generic"] = -INF
    else:
        margin["generic"] = (key_k - eps - b * scale) / eps if eps > 0 else (INF if b * scale < key_k else -INF)
    tau["generic"] = float(cval[k_eff - 1]) if Vr >= k_eff else INF
    # wide build (kz_finalize_query_wide: ordinary direction only)
    b = max(piece_w, left_max)
    if n_valid > KS:
        b = max(b, cut)
    B["wide"] = b
    ties = int((cval <= cval[min(Vr, k_eff + 1) - 1]).sum()) if Vr else 0
    if V < k_eff or ties > KS:
        margin["wide"], tau["wide"] = -INF, INF
    else:
        tau["wide"] = float(cval[k_eff - 1])
        if b == -INF:
            margin["wide"] = INF if Vr >= min(k_eff, n_i) else -INF
        else:
            margin["wide"] = (key_k - eps - b * scale) / eps if eps > 0 else (INF if b * scale < key_k else -INF)
    certified = {w: (m > 0.0 and ratio <= 1.0) for w, m in margin.items()}
    # output step (kz_emit_sorted): among the first k + 1, drop the entry whose id is the query's own row; absent: the first one
    drop = -1
    if exclude_self:
        drop = 0
        for c in range(min(Vr, k + 1)):
            if cand[c] == self_row:
                drop = c
                break
    keep = [c for c in range(Vr) if c != drop][:k]
    return dict(V=V, Vr=Vr, B=B, key_k=key_k, margin=margin, certified=certified, tau=tau, ratio=ratio, cand=cand, cval=cval,
                ind=np.asarray([cand[c] for c in keep], dtype=np.int64),
                dist=np.asarray([output_distance(float(cval[c]), metric, f32_rows) for c in keep], dtype=np.float64))


# ---- the first pass's contract, for the property tests --------------------------------------------------------------------------------
def first_pass_lists(approx, n_lists, KP, floor, rng, deal="blocks"):
    """Lists as a correct first pass leaves them: the index rows are cut into n_lists ranges, every range keeps its KP best approximate
    keys ABOVE the floor (rows at or below it never enter), in no particular order, the unused places empty with a garbage key.
    Returns keys [n_lists KP] float32, ids [n_lists KP] int32."""
    n = len(approx)
    keys = np.full(n_lists * KP, -INF, dtype=np.float32)
    ids = np.full(n_lists * KP, -1, dtype=np.int32)
    if deal == "blocks":
        cuts = np.linspace(0, n, n_lists + 1).astype(np.int64)
        ranges = [np.arange(cuts[i], cuts[i + 1]) for i in range(n_lists)]
    else:
        ranges = [np.arange(i, n, n_lists) for i in range(n_lists)]
    for li, rows in enumerate(ranges):
        rows = rows[approx[rows] > floor]
        best = rows[np.lexsort((rows, -approx[rows].astype(np.float64)))][:KP]
        best = best[rng.permutation(len(best))]
        slot = rng.permutation(KP)[:len(best)]
        keys[li * KP + slot] = approx[best]
        ids[li * KP + slot] = best
        empty = np.setdiff1d(np.arange(KP), slot)
        keys[li * KP + empty] = rng.choice(np.asarray([-INF, 0.0, 1e30, -1e30], dtype=np.float32), size=len(empty))
    return keys, ids


def brute_topk(values, k_eff):
    """The whole index's k_eff best rows by (value, id)."""
    return np.lexsort((np.arange(len(values)), values))[:k_eff]


def perturbed_keys(exact_keys, eps, scale, rng, frac=0.9):
    """Approximate keys of ALL rows in list units: (key + delta) / scale rounded to float32, |delta| <= frac eps -- the rest of eps is left
    to the float32 rounding, which the callers keep far below it."""
    delta = rng.uniform(-frac, frac, size=len(exact_keys)) * eps
    a = ((exact_keys + delta) / scale).astype(np.float32)
    assert eps == 0.0 or (np.abs(a.astype(np.float64) * scale - exact_keys) <= eps).all()
    return a


# ---- exact values and test data -------------------------------------------------------------------------------------------------------
def exact_values(X, Y, metric):
    """[n_q, n_i] float64 ranking values (squared distance / cosine distance) of the rows as stored, each pair by one row-wise sum: equal
    index rows get equal values."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out = np.empty((len(X), len(Y)))
    if metric == "cosine":
        yn = np.sqrt((Y * Y).sum(1))
        yn[yn == 0] = 1.0
        Yn = Y / yn[:, None]
        for i, x in enumerate(X):
            xn = math.sqrt(float((x * x).sum())) or 1.0
            out[i] = np.clip(1.0 - (Yn * (x / xn)).sum(1), 0.0, 2.0)
    else:
        for i, x in enumerate(X):
            out[i] = ((Y - x) ** 2).sum(1)
    return out


def value_bound(x, y, d):
    """Round-off of one float64 evaluation of the ranking value against an exact one: (d + 8) 2^-53 (|q| + |y|)^2."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return (d + 8) * 2.0 ** -53 * (math.sqrt(float((x * x).sum())) + math.sqrt(float((y * y).sum()))) ** 2


def exact_value_fsum(x, y, metric):
    """One pair, exactly rounded sums (math.fsum) of exact float64 products of the stored elements."""
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    y = [float(v) for v in np.asarray(y, dtype=np.float64)]
    if metric == "cosine":
        xn = math.sqrt(math.fsum(a * a for a in x)) or 1.0
        yn = math.sqrt(math.fsum(b * b for b in y)) or 1.0
        return min(max(1.0 - math.fsum(a * b for a, b in zip(x, y)) / (xn * yn), 0.0), 2.0)
    return math.fsum((a - b) * (a - b) for a, b in zip(x, y))


PROPERTY_ROWS = 197   # rows of a property case: two query tiles, no multiple of 4


def property_rows(K, eps_unit, scale, geom, seed, which, floor_share=0.6, tunes=(1.0, 0.85, 1.2, 0.7, 1.4, 0.6, 1.7, 0.65, 0.75, 0.55, 0.92, 1.1, 1.3, 1.55, 2.0)):
    """Lists by the first pass's contract for every query of a case.  K [n_q, n_i]: exact keys; eps_unit [n_q]: what the case's free
    factor (gamma, eps_scale) multiplies into eps_q; which: the build whose verdicts count ("generic" / "wide").
      1. Without perturbation and floors: every row's slack s0 = key_k - B scale, the room the lists leave.
      2. floor_share of the rows get a floor u s0 below key_k, u uniform in (0.05, 1): their slack is u s0.
      3. The factor: tune x the median of slack / eps_unit, for the first tune of `tunes` with which the RESTATEMENT leaves 22 % .. 78 %
         of the rows uncertified and at most 4.5 % of them within 0.05 eps of the edge (the tests assert 20 % .. 80 % and 5 %).
      4. Perturbed keys (|delta| <= 0.9 eps) for ALL index rows, per range the KP best above the floor.
    Returns (factor, [dict(keys, ids, list_floor, eps)])."""
    n_lists, KP, KS, k_eff = geom
    n_q, n_i = K.shape

    def run(row, q, eps):
        # (qref = 0 and the value -2 key give exact_key = key)
        return finalize_row(row["keys"], row["ids"], -2.0 * K[q], KP=KP, KS=KS, k=k_eff, exclude_self=False, self_row=-1, n_i=n_i, eps=eps,
                            scale=scale, list_floor=row["list_floor"] if row["list_floor"] > -INF else None)

    def rows(eps_of, floors):
        rng, out = np.random.RandomState(seed), []
        for q in range(n_q):
            eps = eps_of(q)
            a = perturbed_keys(K[q], eps, scale, rng)
            keys, ids = first_pass_lists(a, n_lists, KP, floors[q], rng, deal="blocks" if q % 2 else "stride")
            out.append(dict(keys=keys, ids=ids, list_floor=np.float32(floors[q]), eps=eps))
        return out

    rng_f = np.random.RandomState(seed + 7919)
    floors, slack = np.full(n_q, -INF, dtype=np.float32), np.empty(n_q)
    for q, row in enumerate(rows(lambda q: 0.0, floors)):
        r = run(row, q, INF)   # (no window: B is what the lists leave outside)
        valid = row["ids"] >= 0
        low = r["B"]["generic"] if r["B"]["generic"] > -INF else float(row["keys"][valid].min())
        s0 = r["key_k"] - low * scale
        assert s0 > 0
        u = rng_f.uniform(0.05, 1.0)
        if rng_f.rand() < floor_share:
            floors[q] = np.float32((r["key_k"] - u * s0) / scale)
            s0 *= u
        slack[q] = s0 / eps_unit[q]
    tried = []
    for tune in tunes:
        factor = tune * float(np.median(slack))
        out = rows(lambda q: factor * eps_unit[q], floors)
        m = np.asarray([run(row, q, row["eps"])["margin"][which] for q, row in enumerate(out)])
        n_fail, n_edge = int((m <= 0).sum()), int((np.abs(m) < 0.05).sum())
        if 0.22 * n_q <= n_fail <= 0.78 * n_q and n_edge <= 0.045 * n_q:
            return factor, out
        tried.append((tune, n_fail, n_edge))
    raise AssertionError(f"no factor leaves both branches exercised and the edge thin: (tune, uncertified, at the edge) of {n_q} rows: {tried}")


def property_data(seed, n_q, n_i, d):
    """Data for the property tests: half of the index in a cluster, half broad; the queries at distances from the cluster's centre that
    are spread over a decade and a half, so that the room between the k-th key and the lists' bound differs as much from row to row."""
    rng = np.random.RandomState(seed)
    c0 = rng.randn(d)
    Y = np.concatenate([c0 + 0.15 * rng.randn(n_i // 2, d), 0.5 * c0 + rng.randn(n_i - n_i // 2, d)])
    s = np.exp(rng.uniform(math.log(0.08), math.log(2.5), size=n_q))
    X = c0 + s[:, None] * rng.randn(n_q, d)
    return X.astype(np.float32), Y[rng.permutation(n_i)].astype(np.float32)


# ---- the cases both test modules run ---------------------------------------------------------------------------------------------------
class Case:
    """One launch: element type, width, metric, tier, list geometry (two regions of one query tile each), selection, k."""

    def __init__(self, name, elem, d, metric, tier, KP, halves, contig, pieces, KSEL, k, build, exclude_self=0, self_ids=False, maps=False,
                 floor=True, dual=False, dual_col=0, misaligned=False):
        self.name, self.elem, self.d, self.metric, self.tier = name, elem, d, metric, tier
        self.KP, self.halves, self.contig, self.pieces, self.KSEL, self.k, self.build = KP, halves, contig, tuple(pieces), KSEL, k, build
        self.exclude_self, self.self_ids, self.maps, self.floor, self.dual, self.dual_col = exclude_self, self_ids, maps, floor, dual, dual_col
        self.misaligned = misaligned
        self.KS = KSEL if KSEL > 0 else KP
        assert not maps or contig, "idx_map goes with contiguous lists: the wave-interleaved gather does not apply it"
        self.k_eff = k + (1 if exclude_self else 0)

    def geom(self, region):
        return (self.pieces[region] * self.halves, self.KP, self.KS, self.k_eff)

    def layout(self):
        return Layout([1, 2], self.pieces, self.halves, self.contig, self.KP)

    def __repr__(self):
        return self.name


O, T, MN, W = BUILD_ORDINARY, BUILD_TWO_LOADS, BUILD_MANY, BUILD_WIDE
SCENARIO_CASES = [
    # the ordinary float32 build: rank select (M <= 64), radix select (M > 64)
    Case("rank16", "float32", 32, "sqeuclidean", 0, 16, 1, 0, (1, 1), 0, 10, O),
    Case("rank64_32", "float32", 32, "euclidean", 0, 16, 2, 0, (2, 1), 0, 10, O, exclude_self=1, self_ids=True),
    Case("rank64_sel40", "float32", 32, "sqeuclidean", 0, 16, 2, 0, (2, 2), 40, 28, O),
    Case("radix80_1024", "float32", 32, "cosine", 0, 16, 1, 1, (5, 64), 32, 20, O, maps=True),
    Case("radix512_256", "float32", 64, "sqeuclidean", 0, 16, 1, 1, (32, 16), 64, 50, O, exclude_self=1),
    Case("radix_nofloor", "float32", 32, "euclidean", 0, 16, 1, 1, (6, 5), 32, 20, O, floor=False),
    # two 16-byte loads per lane and row; the generic re-rank loop (a width that is no multiple of 4; rows off a 16-byte boundary)
    Case("two_loads", "float32", 300, "euclidean", 0, 64, 2, 0, (1, 2), 0, 50, T),
    Case("loop_d30", "float32", 30, "sqeuclidean", 0, 32, 1, 1, (1, 3), 0, 20, O, exclude_self=1, self_ids=True),
    Case("loop_misaligned", "float32", 32, "cosine", 0, 16, 1, 1, (4, 5), 32, 20, O, misaligned=True),
    # more than 160 selected on the float32 / split-bf16 tier: <float, 8, 2>, both layouts, one and two lists per range
    Case("many_wave2", "float32", 32, "sqeuclidean", 0, 128, 2, 0, (1, 2), 176, 160, MN),
    Case("many_wave1", "float32", 32, "cosine", 0, 64, 1, 0, (4, 8), 176, 160, MN, exclude_self=1, self_ids=True),
    Case("many_contig", "float32", 64, "euclidean", 0, 16, 1, 1, (32, 33), 176, 160, MN),
    # float64, float16 and bfloat16 rows: ordinary, d = 300, more than 160 selected
    Case("f64", "float64", 32, "euclidean", 0, 16, 1, 1, (4, 6), 32, 20, O),
    Case("f64_d300", "float64", 300, "sqeuclidean", 0, 64, 2, 0, (1, 1), 0, 50, O),
    Case("f64_many", "float64", 32, "cosine", 0, 16, 1, 1, (16, 32), 176, 160, MN),
    Case("f16", "float16", 32, "euclidean", 0, 16, 1, 1, (4, 6), 32, 20, O, exclude_self=1),
    Case("f16_d300", "float16", 300, "sqeuclidean", 0, 64, 2, 0, (1, 2), 0, 50, T),
    Case("f16_many", "float16", 32, "sqeuclidean", 0, 16, 1, 1, (16, 32), 176, 160, MN),
    Case("bf16", "bfloat16", 32, "cosine", 0, 16, 1, 1, (4, 6), 32, 20, O),
    Case("bf16_d300", "bfloat16", 300, "euclidean", 0, 64, 2, 0, (1, 2), 0, 50, T),
    Case("bf16_many", "bfloat16", 32, "sqeuclidean", 0, 16, 1, 1, (16, 32), 176, 160, MN),
    # the fp16 tier: the wide kernel at every lanes-per-row build (edge and inside), lists of 16 up to 512 entries, 33 .. 64 lists
    # of 16, lists of 128, both sorts (k <= 254, k >= 256), cosine (normalised float64 rows)
    Case("wide_d32", "float32", 32, "sqeuclidean", 2, 16, 1, 1, (32, 20), 256, 240, W),
    Case("wide_d64", "float32", 64, "cosine", 2, 16, 1, 1, (33, 64), 256, 240, W),
    Case("wide_d128", "float32", 128, "euclidean", 2, 128, 1, 1, (32, 8), 272, 258, W),
    Case("wide_d256", "float32", 256, "cosine", 2, 16, 1, 1, (32, 20), 272, 258, W, exclude_self=1, self_ids=True),
    Case("wide_d20", "float32", 20, "euclidean", 2, 16, 1, 1, (18, 32), 256, 240, W, maps=True),
    Case("wide_d52", "float32", 52, "cosine", 2, 16, 1, 1, (64, 33), 272, 258, W),
    Case("wide_d100", "float32", 100, "sqeuclidean", 2, 128, 1, 1, (32, 4), 256, 240, W, exclude_self=1),
    Case("wide_d200", "float32", 200, "sqeuclidean", 2, 16, 1, 1, (32, 33), 272, 258, W),
    # the fp16 tier's bound in the generic kernel: few selected; float64 rows with many selected
    Case("h_ordinary", "float32", 64, "sqeuclidean", 2, 64, 1, 1, (1, 2), 0, 50, O),
    Case("h_f64_many", "float64", 32, "euclidean", 2, 16, 1, 1, (16, 32), 176, 160, MN),
    # ... and its cosine re-rank from the raw rows (no normalised float64 rows: at most 160 selected), key (qref - 2 dist) / 2
    Case("h_cosine", "float32", 64, "cosine", 2, 64, 1, 1, (1, 2), 0, 50, O),
    Case("h_cosine_sel", "float32", 32, "cosine", 2, 16, 1, 1, (5, 8), 64, 40, O, exclude_self=1),
    # the reverse direction of a shared sweep: one list of events, everything else below excl_floor; with and without the extra term
    Case("dual", "float32", 32, "sqeuclidean", 2, 64, 1, 1, (1, 1), 0, 50, O, dual=True, floor=False),
    Case("dual_col", "float32", 32, "sqeuclidean", 2, 64, 1, 1, (1, 1), 0, 50, O, dual=True, dual_col=1, floor=False),
]

PROPERTY_M = {16: (16, 1), 32: (32, 1), 64: (16, 4), 80: (16, 5), 128: (64, 2), 256: (16, 16), 512: (16, 32), 528: (16, 33), 1024: (16, 64),
              4096: (128, 32)}   # M: (KP, lists)
PROPERTY_BUILDS = [   # (name, elem, d, metric, tier, build, many selected)
    ("ordinary", "float32", 32, "sqeuclidean", 0, O, False), ("two_loads", "float32", 300, "euclidean", 0, T, False),
    ("loop", "float32", 30, "cosine", 0, O, False), ("many", "float32", 32, "euclidean", 0, MN, True),
    ("wide8", "float32", 32, "sqeuclidean", 2, W, True), ("wide16", "float32", 52, "cosine", 2, W, True),
    ("wide32", "float32", 100, "euclidean", 2, W, True), ("wide64", "float32", 256, "sqeuclidean", 2, W, True),
    ("f64", "float64", 32, "cosine", 0, O, False), ("f16", "float16", 32, "sqeuclidean", 0, O, False),
    ("bf16", "bfloat16", 300, "sqeuclidean", 0, T, False),
]


def property_case(build, M):
    name, elem, d, metric, tier, b, many = build
    KP, lists = PROPERTY_M[M]
    k = max(3, min(100 if many else 10, M // 3))
    KSEL = 256 if many else {16: 0, 32: 0, 128: 0, 4096: 0}.get(M, 32 if M <= 80 else 64)
    inter = tier == 0 and lists % 2 == 0 and M in (64, 128, 512)
    return Case(f"{name}_M{M}", elem, d, metric, tier, KP, 2 if inter else 1, 0 if inter else 1, (lists // 2 if inter else lists,) * 2, KSEL, k,
                b, exclude_self=1 if M in (80, 528) else 0, self_ids=M == 80)


def property_n_i(M):
    return min(2048, max(200, M + M // 4))


N_DUP = 320                  # copies of ONE row at the end of the index: more equal keys than any selection holds
N_GROUPS, GROUP = 40, 6      # ... before them 40 cluster rows in 6 copies each: exact ties at whatever level a query needs them
N_TIES = N_DUP + N_GROUPS * GROUP   # rows at the end of the index that only the tie scenarios hand out
GAP = 1.5   # the candidates above the k_eff-th lie at least this many eps above it: clear of every key a scenario designs around it


def scenario_data(seed, n_q, n_i, d, metric):
    """Index: a tight cluster around c0 (many rows per eps around a query's key level, although eps is about 1e-3 of the whole key
    spread), 256 broad rows (the spread); the last N_TIES rows are the copies.  Returns (Y, queries): queries(centre) gives the query rows
    -- c0 / 2 relative to `centre` (the fp16 tier's mu; None: the origin) plus a part orthogonal to c0, so that for the euclidean
    family the cluster's keys straddle zero."""
    rng = np.random.RandomState(seed)
    c0 = rng.randn(d) * 1.5
    n_broad = 256
    Y = np.concatenate([c0 + 0.05 * rng.randn(n_i - n_broad, d), c0 * 0.5 + rng.randn(n_broad, d)]).astype(np.float32)
    Y = Y[rng.permutation(n_i)]
    g0 = n_i - N_TIES
    Y[g0:n_i - N_DUP] = np.repeat((c0 + 0.05 * rng.randn(N_GROUPS, d)).astype(np.float32), GROUP, axis=0)
    Y[n_i - N_DUP:] = c0.astype(np.float32)

    def queries(centre):
        mu = np.zeros(d) if centre is None else np.asarray(centre, dtype=np.float64)[:d]
        c = c0 - mu
        w = rng.randn(n_q, d) * 0.7
        w -= np.outer(w @ c, c) / float(c @ c)
        # q.c = |c|^2 / 2 puts the key of a row AT c at zero; a cluster row c + 0.05 eta has the key 0.05 (q - c).eta - 0.00125 |eta|^2,
        # of spread sigma around -0.00125 d.  The queries go a little further along c, so that zero lies 0.2 sigma below the
        # cluster's median: a few hundred rows on either side, which the scenarios with 250 candidates above zero, or below, need.
        sigma = 0.05 * math.sqrt(0.25 * float(c @ c) + 0.49 * (d - 1))
        alpha = 0.5 + (0.2 * sigma + 0.00125 * d) / float(c @ c)
        return (mu + alpha * c + w).astype(np.float32)
    return Y, queries


class RowBuilder:
    """One query's crafted lists.  K[j] = the exact key of index row j in key units; an entry is (id, key in list units, float32)."""

    def __init__(self, values, qref, eps, scale, cosine, tier_h, geom, rng, min_gap=0.0):
        """min_gap: of two free rows whose exact values are nearer than this only one is handed out (the tests want the candidates'
        exact order far above the round-off of one evaluation)."""
        n_free = len(values) - N_TIES
        self.v = values
        self.K = np.asarray([exact_key(v, qref, cosine, tier_h) for v in values])
        self.eps, self.scale, self.rng = eps, scale, rng
        self.n_lists, self.KP, self.KS, self.k_eff = geom
        self.free = np.ones(len(values), dtype=bool)
        self.free[n_free:] = False   # (the copies are handed out by dups() and dup_group() only)
        o = np.argsort(values[:n_free], kind="stable")
        near = np.flatnonzero(np.diff(np.asarray(values)[o]) < min_gap)
        self.free[o[near + 1]] = False
        self.n_free = n_free

    def a32(self, key):
        return np.float32(key / self.scale)

    def key_of(self, a):
        return float(a) * self.scale

    def take(self, target, lo=-INF, hi=INF):
        """The free row whose exact key is nearest to target inside (lo, hi)."""
        ok = np.flatnonzero(self.free & (self.K > lo) & (self.K < hi))
        assert len(ok), "no index row with an exact key in the interval: the data is too sparse for this scenario"
        j = int(ok[np.argmin(np.abs(self.K[ok] - target))])
        self.free[j] = False
        return j

    def entry(self, target_approx, lo=-INF, hi=INF, off=0.0):
        """An entry whose approximate key is target_approx and whose exact key is as near to target_approx - off eps as the data allows
        (inside (lo, hi)); the bound must hold for it with room: |approx - exact| <= 0.95 eps."""
        j = self.take(target_approx - off * self.eps, lo, hi)
        a = self.a32(target_approx)
        assert abs(self.key_of(a) - self.K[j]) <= 0.95 * self.eps, (self.key_of(a), self.K[j], self.eps)
        return (j, a)

    def exact_entries(self, n, lo=-INF, hi=INF, nearest_to=None):
        """n entries with approx = exact (rounded to float32) from the free rows inside (lo, hi): the nearest to a level, else the highest."""
        ok = np.flatnonzero(self.free & (self.K > lo) & (self.K < hi))
        assert len(ok) >= n, f"{n} rows wanted, {len(ok)} free inside the interval"
        o = ok[np.argsort(np.abs(self.K[ok] - nearest_to) if nearest_to is not None else -self.K[ok])][:n]
        self.free[o] = False
        return [(int(j), self.a32(self.K[j])) for j in o]

    def dups(self, n):
        j0 = len(self.K) - N_DUP
        return [(j0 + int(i), self.a32(self.K[j0])) for i in self.rng.permutation(N_DUP)[:n]]

    def dup_group(self, level):
        """The 6 copies of the group whose exact key is nearest to level: ([entries], key)."""
        g0 = len(self.K) - N_TIES
        g = int(np.argmin(np.abs(self.K[g0:g0 + N_GROUPS * GROUP:GROUP] - level)))
        j0 = g0 + g * GROUP
        return [(j0 + int(i), self.a32(self.K[j0])) for i in self.rng.permutation(GROUP)], float(self.K[j0])

    def level(self):
        """Where a scenario puts its k_eff-th candidate by default: the median of the free rows' keys (the cluster), lower where the
        k_eff - 1 candidates above it need the room (at least k_eff + 20 free rows more than GAP + 0.5 eps above)."""
        Ks = np.sort(self.K[self.free])[::-1]
        w = len(Ks) // 4   # (the middle of the densest quarter of the rows: the cluster's core, whatever else the index holds)
        i = int(np.argmin(Ks[:len(Ks) - w] - Ks[w:]))
        return min(float(Ks[i + w // 2]), float(Ks[self.k_eff + 20]) - (GAP + 0.5) * self.eps)

    def neg_level(self):
        """... and where every candidate's key is negative."""
        Ks = np.sort(self.K[self.free & (self.K < 0)])[::-1]
        return min(self.level(), float(Ks[self.k_eff + 10]) - (GAP + 0.3) * self.eps)

    def place(self, entries, pinned=()):
        """Entries into n_lists lists of KP places.  pinned: (list number, [entries], full): that list holds exactly these (full: it must
        have KP of them).  Every other list keeps one place empty where the room allows and gets the entries at random."""
        n_lists, KP = self.n_lists, self.KP
        keys = np.empty(n_lists * KP, dtype=np.float32)
        keys[:] = self.rng.choice(np.asarray([-INF, 0.0, -0.0, 1e30, -1e30, 3.5], dtype=np.float32), size=len(keys))
        ids = np.full(n_lists * KP, -1, dtype=np.int32)
        room = {li: KP for li in range(n_lists)}
        for li, ents, full in pinned:
            assert len(ents) <= KP and (not full or len(ents) == KP)
            slots = self.rng.permutation(KP)[:len(ents)]
            for s, (j, a) in zip(slots, ents):
                ids[li * KP + s], keys[li * KP + s] = j, a
            del room[li]
        spare = sum(room.values()) - len(entries)
        assert spare >= 0, "more entries than places"
        if spare >= len(room):
            room = {li: r - 1 for li, r in room.items()}
        slots = np.asarray([li * KP + s for li, r in room.items() for s in self.rng.permutation(KP)[:r]], dtype=np.int64)
        slots = slots[self.rng.permutation(len(slots))[:len(entries)]]
        for s, (j, a) in zip(slots, entries):
            ids[s], keys[s] = j, a
        return keys, ids

    # ---- the building blocks of a scenario (levels in key units, e = eps) ----
    def pivot(self, level=None):
        """The candidate that is to be the k_eff-th best exactly; by default at the median of the free rows' keys (the cluster)."""
        if level is None:   # (at or below the default level: the room above it is counted from there)
            lv = self.level()
            j = self.take(lv, hi=float(np.nextafter(lv, INF)))
        else:
            j = self.take(level)
        return j, float(self.K[j])

    def top(self, n, above, prefer=None):
        """n candidates with exact keys above `above` (the nearest), approx = exact."""
        out = []
        if prefer is not None and n > 0 and self.free[prefer] and self.K[prefer] > above:
            self.free[prefer] = False
            out.append((int(prefer), self.a32(self.K[prefer])))
        return out + self.exact_entries(n - len(out), lo=above, nearest_to=above)

    def between(self, n, lo, hi, below):
        """n entries with approximate keys evenly inside (lo, hi) and exact keys below `below`."""
        return [self.entry(lo + (hi - lo) * (i + 1) / (n + 1), hi=below, off=0.3) for i in range(n)]

    def n_left(self):
        """Entries a full selection leaves behind: 5 where the lists have the room (with KS > KP: and a free place per list), else what
        there is."""
        M = self.n_lists * self.KP
        need = self.n_lists if self.KS > self.KP else 0
        n = 5 if M - self.KS >= 5 + need else M - self.KS - need
        assert n >= 0
        return n


SCENARIOS = ("complete_ok", "complete_short", "cut_ok", "cut_fail", "evict_full", "evict_hole", "floor_above", "floor_below", "tie_cut",
             "tie_zero", "all_equal", "neg_cut_ok", "neg_tie", "sign_only", "window_perm", "window_inside", "violate", "dup_k")
DUAL_SCENARIOS = ("complete_ok", "complete_short", "excl_ok", "excl_fail", "excl_inf", "excl_full_fail", "excl_full_ok", "excl_hole_ok",
                  "excl_between")


def scenario_names(geom, *, has_floor, dual, zero_level):
    """The scenarios a geometry (n_lists, KP, KS, k_eff) can hold."""
    n_lists, KP, KS, k_eff = geom
    M = n_lists * KP
    if dual:
        return [s for s in DUAL_SCENARIOS]
    out = []
    for s in SCENARIOS:
        if s in ("evict_full", "evict_hole") and not (KS > KP and M >= KS + 5 + n_lists):
            continue
        if s in ("tie_cut", "tie_zero", "neg_tie", "all_equal") and not (M >= KS + 3 + (n_lists if KS > KP else 0) and KS - k_eff >= 4):
            continue
        if s in ("floor_above", "floor_below", "window_perm", "window_inside", "violate", "dup_k") and not has_floor:
            continue
        if s in ("tie_zero", "sign_only", "neg_cut_ok", "neg_tie") and not zero_level:   # (the cluster's keys straddle zero)
            continue
        if s in ("complete_ok", "complete_short", "window_perm", "window_inside", "violate", "dup_k") and not (k_eff + 2 <= min(KS, M - n_lists) - 1):
            continue
        out.append(s)
    return out


def scenario_or_fallback(make_builder, name, **kw):
    """scenario_row on a fresh builder; where this query's keys are too sparse around the level the scenario needs (the builder's
    assertions), the row becomes a complete_ok row instead.  The callers count how often every scenario was built."""
    try:
        return scenario_row(make_builder(), name, **kw)
    except AssertionError:
        return scenario_row(make_builder(), "complete_ok", **kw)


def scenario_row(b, name, prefer=None, eps_pair=None):
    """One crafted row: dict(keys, ids, list_floor, excl_floor, expect) -- expect: the verdict the scenario is built for (the restatement
    must say the same; `wide`: where the wide build's differs)."""
    e, KS, KP, k_eff, n_lists = b.eps, b.KS, b.KP, b.k_eff, b.n_lists
    M = n_lists * KP
    floor = excl = None
    pinned = ()
    expect = True

    def selection(K_k, pv, cut_level, n_above=0, above_lo=None, skip_top=0):
        """A full selection around the pivot: the top group, the pivot, entries between the cut and the pivot, the cut entry."""
        ents = b.top(k_eff - 1 - skip_top, K_k + GAP * e, prefer) + [pv]
        nb = KS - k_eff - 1
        assert nb >= n_above
        hi_lo = above_lo if above_lo is not None else cut_level
        above = b.between(n_above, hi_lo, K_k - 0.02 * e, K_k) if n_above else []
        rest = b.between(nb - n_above, cut_level, min(hi_lo, K_k - 0.02 * e), K_k) if nb - n_above else []
        return ents, above, rest, [b.entry(cut_level, hi=K_k, off=0.3)]

    if name in ("complete_ok", "complete_short", "excl_ok", "excl_fail", "excl_inf", "excl_hole_ok", "excl_between"):
        pj, K_k = b.pivot()
        short = name == "complete_short"
        ents = b.top(k_eff - 1 - (1 if short else 0), K_k + GAP * e, prefer) + [(pj, b.a32(K_k))]
        n_more = min(3, min(KS, M - n_lists) - 1 - len(ents)) if name != "excl_hole_ok" else KP - 1 - len(ents)
        if not short:   # (short: k_eff - 1 candidates in all)
            ents += b.exact_entries(max(0, n_more), hi=K_k - 5 * e, nearest_to=K_k - 5 * e)
        expect = not short
        if name == "excl_ok" or name == "excl_hole_ok":
            excl = b.a32(K_k - 1.5 * e)
        elif name == "excl_fail":
            excl, expect = b.a32(K_k - 0.5 * e), False
        elif name == "excl_inf":
            excl, expect = np.float32(INF), False
        elif name == "excl_between":
            # certified with the ordinary bound e0, failed with the reverse direction's larger e1: the floor where both margins are
            # (e1 - e0) / (e1 + e0) in size
            e0, e1 = eps_pair
            excl, expect = b.a32(K_k - 2.0 * e0 * e1 / (e0 + e1)), e <= e0
    elif name in ("cut_ok", "cut_fail", "floor_above", "floor_below", "neg_cut_ok", "excl_full_fail", "excl_full_ok"):
        level = b.neg_level() if name == "neg_cut_ok" else None
        pj, K_k = b.pivot(level)
        m = -0.5 if name in ("cut_fail", "excl_full_fail") else 0.5
        t, a, r, c = selection(K_k, (pj, b.a32(K_k)), K_k - e - m * e)
        n_left = 0 if name.startswith("excl") else b.n_left()
        ents = t + a + r + c + b.exact_entries(n_left, hi=K_k - 12 * e, nearest_to=K_k - 12 * e)
        expect = m > 0
        if name == "floor_above":
            floor, expect = b.a32(K_k - 0.5 * e), False
        elif name == "floor_below":
            floor = b.a32(K_k - 3 * e)
        elif name.startswith("excl"):
            excl = b.a32(K_k - 3 * e)
    elif name in ("evict_full", "evict_hole"):
        pj, K_k = b.pivot()
        n_top = k_eff - 1
        n_above = max(0, KP - 1 - n_top - 1)
        t, a, r, c = selection(K_k, (pj, b.a32(K_k)), K_k - 1.5 * e, n_above=n_above + 1, above_lo=K_k - 0.5 * e)
        # a[0] is the lowest of the entries above K_k - 0.5 e: move it ONTO that level -- the full list's minimum
        a = sorted(a, key=lambda x: float(x[1]))
        star = (a[0][0], b.a32(K_k - 0.5 * e))
        assert abs(b.key_of(star[1]) - b.K[star[0]]) <= 0.95 * e
        others = (a[1:] + t)[:KP - 1]   # (t ends with the pivot)
        assert len(others) == KP - 1
        in_list = {j for j, _ in others} | {star[0]}
        pool = [x for x in t + a[1:] + r + c if x[0] not in in_list]
        pool += b.exact_entries(b.n_left(), hi=K_k - 12 * e, nearest_to=K_k - 12 * e)
        if name == "evict_hole":
            pool.append(others.pop())
        pinned = ((int(b.rng.randint(n_lists)), [star] + others, name == "evict_full"),)
        ents, expect = pool, name == "evict_hole"
    elif name in ("tie_cut", "tie_zero", "neg_tie"):
        if name == "tie_zero":
            pj, K_k = b.pivot(0.5 * e)
            c_level = 0.0
        else:
            pj, K_k = b.pivot(b.neg_level() if name == "neg_tie" else None)
            c_level = K_k - 0.5 * e
        ents = b.top(k_eff - 1, K_k + GAP * e, prefer) + [(pj, b.a32(K_k))]
        ents += b.between(KS - k_eff - 3, c_level, K_k - 0.02 * e, K_k)
        tied = [b.entry(c_level, hi=K_k, off=0.3) for _ in range(6)]
        if name == "tie_zero":
            tied = [(j, np.float32(0.0 if i % 2 else -0.0)) for i, (j, _) in enumerate(tied)]
        ents, expect = ents + tied, False
    elif name == "all_equal":
        ents, expect = b.dups(KS + 3), False
    elif name == "sign_only":
        pj, K_k = b.pivot(0.75 * e)
        t, a, r, c = selection(K_k, (pj, b.a32(K_k)), -K_k)
        c = [(c[0][0], np.float32(-float(b.a32(K_k))))]   # (the pivot's key with the other sign)
        ents = t + a + r + c + b.exact_entries(b.n_left(), hi=K_k - 12 * e, nearest_to=K_k - 12 * e)
    elif name == "window_perm":
        pj, K_k = b.pivot()
        ents = b.top(k_eff - 3, K_k + GAP * e, prefer)
        centre = K_k + 0.125 * e   # (four candidates a quarter of an eps apart, their approximate keys mirrored at the centre)
        for lvl in (0.5, 0.25, 0.0, -0.25):
            j = pj if lvl == 0.0 else b.take(K_k + lvl * e, K_k + (lvl - 0.08) * e, K_k + (lvl + 0.08) * e)
            a = b.a32(2 * centre - b.K[j])
            assert abs(b.key_of(a) - b.K[j]) <= 0.95 * e
            ents.append((j, a))
        ents += b.exact_entries(max(0, min(5, KS - 1 - len(ents), M - n_lists - len(ents))), hi=K_k - 12 * e, nearest_to=K_k - 12 * e)
        floor = b.a32(K_k - 1.5 * e)
    elif name == "window_inside":
        pj, x = b.pivot()   # U: the k_eff-th by approximate key, over-estimated
        ents = b.top(k_eff - 1, x + GAP * e, prefer) + [(pj, b.a32(x + 0.85 * e))]
        w = b.entry(x - 0.65 * e, off=-0.85)   # W: 1.5 eps below U's approximate key, exactly better than U
        assert b.K[w[0]] > x
        ents.append(w)
        ents += b.exact_entries(max(0, min(5, KS - 1 - len(ents), M - n_lists - len(ents))), hi=x - 12 * e, nearest_to=x - 12 * e)
        floor = b.a32(b.K[w[0]] - 1.5 * e)
    elif name == "violate":
        pj, K_k = b.pivot()
        ents = b.top(k_eff - 1, K_k + GAP * e, prefer) + [(pj, b.a32(K_k))]
        j = b.take(K_k - 2.3 * e)
        ents.append((j, b.a32(b.K[j] + 1.52 * e)))   # inside the window, 1.52 eps off its exact key: a ratio >= 1.5 after float32 rounding
        floor, expect = b.a32(K_k - 1.5 * e), False
    elif name == "dup_k":
        copies, K_k = b.dup_group(b.level())
        ents = b.top(k_eff - 3, K_k + GAP * e, prefer) + copies
        ents += b.exact_entries(max(0, min(5, KS - 1 - len(ents), M - n_lists - len(ents))), hi=K_k - 12 * e, nearest_to=K_k - 12 * e)
        floor = b.a32(K_k - 1.5 * e)
    else:
        raise KeyError(name)
    keys, ids = b.place(ents, pinned)
    return dict(keys=keys, ids=ids, list_floor=floor, excl_floor=excl, expect=expect, name=name)
