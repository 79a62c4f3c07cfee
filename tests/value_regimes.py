"""Data far from unit scale (test infrastructure of tests/test_gpu_value_range.py, tests/test_value_regimes.py and tools/fuzz_values.py).

Every rounding bound of the search is built from magnitudes: the fp16 image's centre and power-of-two scale, the
per-row |x_c|^2, |x_h|, |r| and their per-matrix maxima, the raw maxima of the float32 / split-bf16 bound.  The regimes below put
those magnitudes where unit-scale `rand` / `randn` data never does.  Each regime is a function of (n_q, n_i, d, dtype, seed, ...)
that returns (query, index); `query is index` for a single matrix searched with exclude_self.

What a test may assert about a regime comes from the oracle alone (oracle.kiez_oracle, float64) and is proven on the CPU by
tests/test_value_regimes.py for every committed case:

  * power-of-two equivariance: scaling query and index by 2^e commutes with every rounding inside the normal range, so the
    neighbour indices are unchanged and the distances are multiplied by exactly 2^e / 4^e / 1 (`pow2_factor`);
  * `gap_ulps`: the smallest difference between consecutive squared distances of the oracle's first k + 1 neighbours, in ulps
    of |q|^2 + |y|^2 -- the scale at which the reference's expansion and the device's float64 re-rank both round.  From 2 ulps
    on the device orders a pair as the reference does (tests/test_gpu_near_ties.py); a case compared index for
    index has every row at >= STRICT_GAP_ULPS = 16.
"""
import numpy as np

LIMIT_SQ = 1e30          # the input limit: squared row norms up to 1e30 (kz_norms_kernel)
STRICT_GAP_ULPS = 16.0
TIE_ULPS = 2.0
TILE = 128

# one width per kernel family: the 64-query fp16 build (d <= 208), the fp16 builds up to 24 slices, 497 .. 1024, 1025 .. 2048, and
# a width whose FIRST pass has float32 operands (385 .. 496)
WIDTHS = (64, 200, 320, 768, 1536, 400)
POW2_EXPONENTS = (-66, -50, -40, -20, 20, 40, "max")
POW2_BELOW_THE_SCALE_CLAMP = -110   # the fp16 scale's exponent is clamped at +-100 (kz_center_finish_kernel): float64, no euclidean float32
MISMATCH_R = (2, 3, 6, 10, 20)
OFFSETS_STRICT = (1e2, 1e3, 1e4)
OFFSET_TIES = 1e5
OUTLIER_M = (1e3, 1e6, 1e9)
OUTLIER_WHERE = ("first", "middle", "last", "ragged")
OUTLIER_SIDE = ("index", "query", "both")


def base_pair(n_q, n_i, d, dtype, seed, gen="rand", single=False):
    """The unit-scale pair every regime starts from."""
    rng = np.random.RandomState(seed)
    g = rng.rand if gen == "rand" else rng.randn
    y = g(n_i, d).astype(dtype)
    q = y if single else g(n_q, d).astype(dtype)
    return q, y


def _max_sq(*mats):
    return max(float(np.einsum("ij,ij->i", m.astype(np.float64), m.astype(np.float64)).max()) for m in mats)


def e_max(q, y):
    """The largest e with every |2^e x|^2 < 1e30."""
    e = int(np.floor(0.5 * np.log2(LIMIT_SQ / _max_sq(q, y))))
    while _max_sq(q, y) * 4.0 ** e >= LIMIT_SQ:
        e -= 1
    return e


def pow2(e, n_q, n_i, d, dtype, seed, gen="rand", single=False):
    """(base, scaled, e): the base pair and the same pair times 2^e (exact in either dtype)."""
    q, y = base_pair(n_q, n_i, d, dtype, seed, gen, single)
    if e == "max":
        e = e_max(q, y)
    ys = np.ldexp(y, e).astype(dtype)
    qs = ys if single else np.ldexp(q, e).astype(dtype)
    return (q, y), (qs, ys), e


def pow2_factor(metric, e):
    """What a distance of `metric` is multiplied by when both matrices are multiplied by 2^e."""
    return {"euclidean": 2.0 ** e, "sqeuclidean": 4.0 ** e, "cosine": 1.0}[metric]


def cosine_row_scales(n_q, n_i, d, dtype, seed, single=False):
    """(base, scaled): `randn` rows, each times its own 2^U{-30 .. 30}: the cosine distance does not see it."""
    q, y = base_pair(n_q, n_i, d, dtype, seed, "randn", single)
    rng = np.random.RandomState(seed + 7919)
    ys = np.ldexp(y, rng.randint(-30, 31, size=(len(y), 1))).astype(dtype)
    qs = ys if single else np.ldexp(q, rng.randint(-30, 31, size=(len(q), 1))).astype(dtype)
    return (q, y), (qs, ys)


def mismatch(r, larger, n_q, n_i, d, dtype, seed, gen="rand"):
    """Query and index of different scale: `larger` ('query' | 'index') is the base times 2^r, the other one unscaled."""
    q, y = base_pair(n_q, n_i, d, dtype, seed, gen)
    if larger == "query":
        return np.ldexp(q, r).astype(dtype), y
    return q, np.ldexp(y, r).astype(dtype)


def offset(c, n_q, n_i, d, dtype, seed, single=False):
    """A common centre c * rand(d) plus unit-spread `randn`: the mean is c spreads from the origin."""
    rng = np.random.RandomState(seed)
    centre = c * rng.rand(d)
    y = (centre + rng.randn(n_i, d)).astype(dtype)
    q = y if single else (centre + rng.randn(n_q, d)).astype(dtype)
    return q, y


def outlier_row(n, where):
    if where == "first":
        return 0
    if where == "middle":
        return n // 2
    if where in ("last", "ragged"):
        return n - 1
    raise ValueError(where)


def outlier(m, where, side, n_q, n_i, d, dtype, seed, gen="rand", single=False):
    """Unit-scale rows with ONE row multiplied by m, in the index, in the query matrix or in both; `where`: row 0, a middle row,
    the last row, or ('ragged') the last row of a matrix of 128 j + 1 rows -- alone in its tile."""
    if where == "ragged":
        n_q, n_i = (n_q // TILE) * TILE + 1, (n_i // TILE) * TILE + 1
    q, y = base_pair(n_q, n_i, d, dtype, seed, gen, single)
    y = y.copy()
    if single or side in ("index", "both"):
        y[outlier_row(len(y), where)] *= dtype(m)
    if single:
        return y, y
    q = q.copy()
    if side in ("query", "both"):
        q[outlier_row(len(q), where)] *= dtype(m)
    return q, y


def heavy_rows(n_q, n_i, d, dtype, seed, light_first=True):
    """`randn` rows times 2^U{-6 .. 6}.  light_first: the first tile (128 rows) of either matrix holds rows of the smallest scale
    only, so a per-matrix maximum taken over the first tile alone is 2^12 short of the true one."""
    q, y = base_pair(n_q, n_i, d, dtype, seed, "randn")
    rng = np.random.RandomState(seed + 104729)
    eq, ey = rng.randint(-6, 7, size=(len(q), 1)), rng.randint(-6, 7, size=(len(y), 1))
    if light_first:
        eq[:TILE], ey[:TILE] = -6, -6
        ey[-1] = 6   # (and the largest row is the last one of the last, ragged tile)
    return np.ldexp(q, eq).astype(dtype), np.ldexp(y, ey).astype(dtype)


def limit(over, n_q, n_i, d, dtype, seed):
    """Rows with |x| just under (over=False) or just over 1e15: the unit-scale pair times the factor that puts the largest squared
    row norm of the two matrices at 0.98e30 / 1.02e30."""
    q, y = base_pair(n_q, n_i, d, dtype, seed)
    f = np.sqrt((1.02 if over else 0.98) * LIMIT_SQ / _max_sq(q, y))
    return (q.astype(np.float64) * f).astype(dtype), (y.astype(np.float64) * f).astype(dtype)


# ---- what the oracle alone says about a case ---------------------------------------------------------------------------
def _operands(q, y, metric):
    q64, y64 = np.asarray(q, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if metric == "cosine":
        qn, yn = np.sqrt(np.einsum("ij,ij->i", q64, q64)), np.sqrt(np.einsum("ij,ij->i", y64, y64))
        qn[qn == 0.0], yn[yn == 0.0] = 1.0, 1.0
        q64, y64 = q64 / qn[:, None], y64 / yn[:, None]
    return q64, y64


def neighbour_sq_distances(q, y, ind, metric):
    """(d2, unit): squared distances of the listed neighbours from the DIFFERENCES of the (cosine: normalised) float64 rows -- exact
    to a relative 1e-16 of d2 itself -- and the ulp of |q|^2 + |y|^2 for every pair."""
    q64, y64 = _operands(q, y, metric)
    qs, ys = np.einsum("ij,ij->i", q64, q64), np.einsum("ij,ij->i", y64, y64)
    d2 = np.empty(ind.shape, dtype=np.float64)
    for j in range(ind.shape[1]):
        diff = q64 - y64[ind[:, j]]
        d2[:, j] = np.einsum("ij,ij->i", diff, diff)
    return d2, np.spacing(qs[:, None] + ys[ind])


def gap_ulps(q, y, k, metric, exclude_self=False):
    """Per query row: the smallest gap between consecutive squared distances of the oracle's first k + 1 neighbours, in ulps of
    |q|^2 + |y|^2 (negative where the oracle's own order is not the exact one).  Returns (gaps [n_q], oracle indices [n_q, k + 1])."""
    from oracle import kiez_oracle as O
    kk = min(k + 1, len(y) - (1 if exclude_self else 0))
    _, oi = O.knn_exact(*_oracle_inputs(q, y, metric), kk, metric, exclude_self=exclude_self)
    d2, unit = neighbour_sq_distances(q, y, oi, metric)
    gaps = (d2[:, 1:] - d2[:, :-1]) / np.maximum(unit[:, 1:], unit[:, :-1])
    return gaps.min(axis=1), oi


def _oracle_inputs(q, y, metric):
    # cosine: float32 inputs are their exact float64 casts here, as in the rest of the suite
    if metric == "cosine":
        return np.asarray(q, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return q, y


def oracle_knn(q, y, k, metric, exclude_self=False):
    from oracle import kiez_oracle as O
    return O.knn_exact(*_oracle_inputs(q, y, metric), k, metric, exclude_self=exclude_self)


def tie_tolerant_rows(q, y, k, metric, oracle_ind_k1, got_ind):
    """Rows of got_ind [n_q, k] that differ from the oracle's first k columns, and whether every difference lies inside a run of
    oracle neighbours whose consecutive squared distances differ by < TIE_ULPS ulps of |q|^2 + |y|^2 (the run may reach the
    k + 1-th neighbour).  Returns (rows that needed the allowance, rows that are wrong)."""
    d2, unit = neighbour_sq_distances(q, y, oracle_ind_k1, metric)
    tied_next = np.abs(d2[:, 1:] - d2[:, :-1]) < TIE_ULPS * np.maximum(unit[:, 1:], unit[:, :-1])
    needed, wrong = [], []
    for r in np.flatnonzero((oracle_ind_k1[:, :k] != got_ind).any(axis=1)):
        needed.append(int(r))
        ok, p = True, 0
        while p < k:
            e = p
            while e < oracle_ind_k1.shape[1] - 1 and tied_next[r, e]:
                e += 1
            ref = set(oracle_ind_k1[r, p:e + 1].tolist())
            got = set(got_ind[r, p:min(e + 1, k)].tolist())
            ok = ok and (got == ref if e < k else got <= ref)
            p = e + 1
        if not ok:
            wrong.append(int(r))
    return needed, wrong


# ---- the committed cases ---------------------------------------------------------------------------------------------------
def _cycle(seq, i):
    return seq[i % len(seq)]


METRICS = ("euclidean", "sqeuclidean", "cosine")
DTYPES = (np.float32, np.float64)


def knn_cases():
    """The kz_knn cases of tests/test_gpu_value_range.py: dicts with regime, param, shape, d, dtype, metric, k, single, seed and
    `strict` (compared with the oracle index for index: the gap precondition is asserted for it on the CPU).  A covering set:
    every regime meets every width of WIDTHS, both dtypes, and each of its parameters at least once."""
    cases = []

    def add(regime, param, d, dtype, metric, k=10, single=False, n_q=257, n_i=1500, seed=0, strict=True, **extra):
        c = dict(regime=regime, param=param, d=d, dtype=dtype, metric=metric, k=k, single=single, n_q=n_q, n_i=n_i,
                 seed=1000 + len(cases) if seed == 0 else seed, strict=strict)
        c.update(extra)
        c["id"] = "-".join(str(v) for v in (regime, param, f"d{d}", np.dtype(dtype).name, metric, f"k{k}", "self" if single else f"{n_q}x{n_i}"))
        cases.append(c)

    # pow2: the seven exponents over the six widths; 2^-66 on float64 with sqeuclidean / cosine only (float32 products and
    # float32 euclidean distances leave the normal range there: the reference itself stops being equivariant)
    for i, e in enumerate(POW2_EXPONENTS):
        low = e == -66
        dtype = np.float64 if low else _cycle(DTYPES, i)
        metric = _cycle(("sqeuclidean", "cosine"), i) if low else _cycle(METRICS, i)
        add("pow2", e, _cycle(WIDTHS, i), dtype, metric, single=(i == 3), gen="randn" if metric == "cosine" else "rand")
    add("pow2", -50, 64, np.float32, "euclidean", n_i=2049)          # just above the float32 tiers' 1e-30 guard, float32 euclidean
    add("pow2", -66, 200, np.float64, "sqeuclidean", single=True)    # below it: every row of the float32 tiers goes to the exact kernels
    add("pow2", "max", 320, np.float32, "sqeuclidean", gen="rand")
    # 2^-110: the largest element times the clamped scale 2^100 is 2^-10 -- the image keeps the upper four binades, the rest is flushed
    add("pow2", POW2_BELOW_THE_SCALE_CLAMP, 64, np.float64, "sqeuclidean")
    add("pow2", POW2_BELOW_THE_SCALE_CLAMP, 768, np.float64, "cosine", gen="randn")
    for i, d in enumerate(WIDTHS):
        add("cosine_row_scales", "rows", d, _cycle(DTYPES, i + 1), "cosine", single=(i == 2))
    # mismatch: both directions for every r; k = 50 and the dealt-image k = 30 among them (`short`: the dealt route forced
    # onto this small index)
    i = 0
    for r in MISMATCH_R:
        for larger in ("query", "index"):
            k, short = (50, 0) if i in (2, 7) else ((30, 1) if i in (3, 4, 8) else (10, 0))
            add("mismatch", f"{larger}*2^{r}", _cycle(WIDTHS, i), _cycle(DTYPES, i), _cycle(("euclidean", "sqeuclidean"), i // 2), k=k,
                n_i=2049 if short else 1500, r=r, larger=larger, short=short, gen=_cycle(("rand", "randn"), i))
            i += 1
    add("mismatch", "query*2^20", 200, np.float32, "cosine", r=20, larger="query", gen="randn")
    for i, c in enumerate(OFFSETS_STRICT):
        for j, dtype in enumerate(DTYPES):
            add("offset", c, _cycle(WIDTHS, 2 * i + j), dtype, _cycle(METRICS, i + j), single=(i == 1 and j == 0), n_i=2049 if j else 1500)
    # 1e5 spreads: tie-tolerant.  The seeds are fixed by hand: the oracle's OWN expansion (|q|^2 - 2 q.y + |y|^2 over d terms of
    # ~1e10) is several ulps of |q|^2 + |y|^2 off here, and on some draws it orders a pair against exact arithmetic although the
    # two are more than 2 ulps apart (seed 1036 at d = 200: row 320, 2.3 ulps) -- there the device, which ordered that pair as exact
    # arithmetic does, would be held to the reference's mistake.  tests/test_value_regimes.py asserts that these draws have no such
    # pair; both keep rows with gaps under 2 ulps (of either sign), so the allowance is exercised.
    add("offset", OFFSET_TIES, 64, np.float32, "euclidean", n_q=500, n_i=4000, strict=False, seed=1036)
    add("offset", OFFSET_TIES, 200, np.float64, "sqeuclidean", n_q=500, n_i=4000, strict=False, seed=1035)
    # outlier: 3 factors x 3 sides x 4 places, twelve of them plus a single matrix, k = 50 and k = 30
    i = 0
    for where in OUTLIER_WHERE:
        for side in OUTLIER_SIDE:
            m = _cycle(OUTLIER_M, i + i // 3)
            k, short = (50, 0) if i == 5 else ((30, 1) if i in (1, 6) else (10, 0))
            add("outlier", f"{m:g}-{where}-{side}", _cycle(WIDTHS, i), _cycle(DTYPES, i), _cycle(("euclidean", "sqeuclidean"), i // 3), k=k,
                n_i=2049 if short else 1500, m=m, where=where, side=side, short=short)
            i += 1
    add("outlier", "1e+09-last-self", 64, np.float32, "euclidean", single=True, n_i=1500, m=1e9, where="last", side="both")
    add("outlier", "1e+06-ragged-self", 768, np.float64, "sqeuclidean", single=True, n_i=1500, m=1e6, where="ragged", side="both")
    for i, d in enumerate(WIDTHS):
        add("heavy_rows", "light_first", d, _cycle(DTYPES, i), _cycle(("euclidean", "sqeuclidean"), i), k=10 if i else 30, n_i=2049,
            short=0 if i else 1)
    for i, d in enumerate(WIDTHS):
        add("limit", "under", d, _cycle(DTYPES, i), _cycle(METRICS, i))
    return cases


def make(case):
    """(query, index) of a case of knn_cases(); pow2 / cosine_row_scales: ((base pair), (scaled pair), e or None)."""
    c = case
    shape = (c["n_q"], c["n_i"], c["d"], c["dtype"], c["seed"])
    if c["regime"] == "pow2":
        return pow2(c["param"], *shape, gen=c.get("gen", "rand"), single=c["single"])
    if c["regime"] == "cosine_row_scales":
        return cosine_row_scales(*shape, single=c["single"]) + (None,)
    if c["regime"] == "mismatch":
        return mismatch(c["r"], c["larger"], *shape, gen=c.get("gen", "rand"))
    if c["regime"] == "offset":
        return offset(c["param"], *shape, single=c["single"])
    if c["regime"] == "outlier":
        return outlier(c["m"], c["where"], c["side"], *shape, single=c["single"])
    if c["regime"] == "heavy_rows":
        return heavy_rows(*shape)
    if c["regime"] == "limit":
        return limit(c["param"] == "over", *shape)
    raise ValueError(c["regime"])


# (source, target) pairs of the fits of tests/test_gpu_value_range.py: the shared sweep and the image a target inherits
def fit_cases():
    cases = []

    def add(name, d, dtype, metric, maker, equivariant_e=None, n_s=1500, n_t=2100):
        cases.append(dict(id=f"{name}-d{d}-{np.dtype(dtype).name}-{metric}", name=name, d=d, dtype=dtype, metric=metric, maker=maker, e=equivariant_e,
                          n_s=n_s, n_t=n_t, seed=2000 + len(cases)))

    add("pow2(-40)", 64, np.float32, "euclidean", lambda s, t: (np.ldexp(s, -40), np.ldexp(t, -40)), -40)
    add("pow2(40)", 768, np.float32, "sqeuclidean", lambda s, t: (np.ldexp(s, 40), np.ldexp(t, 40)), 40)
    add("source*2^10", 200, np.float32, "euclidean", lambda s, t: (np.ldexp(s, 10), t))
    add("target*2^10", 320, np.float64, "sqeuclidean", lambda s, t: (s, np.ldexp(t, 10)))
    add("target*2^20", 1536, np.float32, "euclidean", lambda s, t: (s, np.ldexp(t, 20)))
    add("source*2^20", 64, np.float64, "euclidean", lambda s, t: (np.ldexp(s, 20), t))
    add("outlier-source", 200, np.float32, "euclidean", lambda s, t: (_with_outlier(s, 1e6, len(s) - 1), t), n_s=1537)
    add("outlier-target", 64, np.float32, "sqeuclidean", lambda s, t: (s, _with_outlier(t, 1e9, len(t) - 1)), n_t=2177)
    add("offset(1e3)", 200, np.float64, "euclidean", None)
    return cases


def _with_outlier(x, m, row):
    x = x.copy()
    x[row] *= x.dtype.type(m)
    return x


def make_fit(case):
    c = case
    if c["maker"] is None:
        s, t = offset(1e3, c["n_s"], c["n_t"], c["d"], c["dtype"], c["seed"])
        return s, t
    s, t = base_pair(c["n_s"], c["n_t"], c["d"], c["dtype"], c["seed"])
    s2, t2 = c["maker"](s, t)
    return s2.astype(c["dtype"]), t2.astype(c["dtype"])


# inputs of the tests of tests/test_gpu_value_range.py that are not cases of knn_cases(): every (query, index, metric) they compare
# with the oracle index for index is listed by oracle_compared_extras() and proven free of near-ties on the CPU
CLAMP_CASES = ((3, 64), (6, 768), (20, 200))                       # (r, d): float32, euclidean
REUSE_CASES = ((10, 64, np.float32), (20, 768, np.float64), (10, 1536, np.float32), (20, 320, np.float32))


def clamp_inputs(r, d):
    return mismatch(r, "query", 300, 1500, d, np.float32, 31 + r)


def reuse_inputs(r, d, dtype):
    """(query of the index's scale, index, a matrix 2^r times larger)."""
    q, y = base_pair(300, 1500, d, dtype, 41 + r)
    big = np.ldexp(base_pair(300, 1500, d, dtype, 43 + r)[0], r).astype(dtype)
    return q, y, big


def oracle_compared_extras():
    out = []
    for r, d in CLAMP_CASES:
        q, y = clamp_inputs(r, d)
        out.append((f"clamp-r{r}-d{d}", q, y, "euclidean"))
    for r, d, dtype in REUSE_CASES:
        q, y, big = reuse_inputs(r, d, dtype)
        for metric in ("euclidean", "cosine"):
            out += [(f"reuse-r{r}-d{d}-{metric}-same", q, y, metric), (f"reuse-r{r}-d{d}-{metric}-larger", big, y, metric),
                    (f"reuse-r{r}-d{d}-{metric}-larger-as-index", y, big, metric)]
    return out


def exact_order(q, y, k, metric, margin=4):
    """The first k + 1 neighbours in the order of the EXACT-difference squared distances: the oracle's first k + 1 + margin (its own
    expansion is a few ulps of |q|^2 + |y|^2 off, never `margin` places) re-sorted by neighbour_sq_distances, ties by index."""
    _, oi = oracle_knn(q, y, k + 1 + margin, metric)
    d2, _ = neighbour_sq_distances(q, y, oi, metric)
    order = np.lexsort((oi, d2), axis=1)
    return np.take_along_axis(oi, order, axis=1)[:, :k + 1]


# ---- the device side: one case through the three first-pass tiers, compared as the regime allows --------------------------------
PRECISIONS = (0, 2, 1)     # fp16 first pass (default), split-bf16, float32 operands
TIER_NAMES = {0: "f32", 1: "bf16x2", 2: "fp16"}   # kz_knn_stats.first_pass


def run_three(ctx, q, y, k, metric, single=False, short=0):
    """{precision: (dist, ind, stats)} of kz_knn under the three `precision` settings, fresh matrices each (`short`: the dealt
    short-list route of the fp16 kernel forced onto a small index)."""
    from kiez_amd import _native as N
    res = {}
    if short:
        ctx.set_option("short_ord_min_tiles", 2)
    try:
        for prec in PRECISIONS:
            ctx.set_option("precision", prec)
            ym = N.DeviceMatrix(ctx, y, metric)
            qm = ym if single else N.DeviceMatrix(ctx, q, metric)
            dd, ii, st = N.knn(ctx, qm, ym, k, exclude_self=single)
            res[prec] = (dd.numpy(), ii.numpy(), st)
    finally:
        ctx.set_option("precision", 0)
        ctx.set_option("short_ord_min_tiles", 48)
    return res


def stats_problems(st, n_q, what=""):
    """The design's own claim about the rounding bound: no re-ranked candidate's approximate key is further from its exact key than
    the bound (max_err_ratio < 1), and where the first pass certified a row at all it re-ranked something (> 0)."""
    out = []
    r = st["max_err_ratio"]
    if not r < 1.0:
        out.append(f"{what}: max_err_ratio {r:.4g} >= 1 (tier {TIER_NAMES[st['first_pass']]})")
    # (rows that went down: kz_knn counts them in n_first_pass_fail, the shared sweep's reverse direction only in the escalated /
    #  fallback totals -- which count a row once per level, so this errs on the side of not asking)
    gone_down = max(st["n_first_pass_fail"], min(n_q, st["n_escalated_rows"] + st["n_fallback_rows"]))
    if gone_down < n_q and not r > 0.0:
        out.append(f"{what}: max_err_ratio {r!r} although the first pass certified rows")
    return out


def three_problems(res, n_q, what=""):
    out = []
    for prec in PRECISIONS[1:]:
        if not np.array_equal(res[0][1], res[prec][1]):
            out.append(f"{what}: indices of precision {prec} differ from precision 0 in {(res[0][1] != res[prec][1]).any(axis=1).sum()} rows")
        if not np.array_equal(res[0][0], res[prec][0]):
            out.append(f"{what}: distance bits of precision {prec} differ from precision 0")
    for prec in PRECISIONS:
        out += stats_problems(res[prec][2], n_q, f"{what} precision {prec}")
    return out


def expected_first_pass(d):
    """kz_knn_stats.first_pass under precision 0 / 2 / 1 at width d: fp16, split-bf16 and float32 operands up to 24 slices of 16; no
    split-bf16 tier on the wide builds (497 .. 2048); float32 operands first everywhere else."""
    if (d + 15) // 16 <= 24:
        return {0: 2, 2: 1, 1: 0}
    if 497 <= d <= 2048:
        return {0: 2, 2: 0, 1: 0}
    return {0: 0, 2: 0, 1: 0}


def route_problems(res, d, k, short, what=""):
    """The routes a committed case is there for really ran: the three precisions started on the tiers the width has, and a `short`
    case took the dealt short-list route of the fp16 kernel (k / 5 lists of 16 over dealt index ranges; rows that were escalated as
    a whole report the longer lists of their second search)."""
    out = []
    want = expected_first_pass(d)
    got = {prec: res[prec][2]["first_pass"] for prec in PRECISIONS}
    if got != want:
        out.append(f"{what}: first-pass tiers {got}, expected {want}")
    st = res[0][2]
    if short and want[0] == 2 and not (st["n_splits"] >= (k + 4) // 5 - 1 and st["n_splits"] >= 2 and (st["list_len"] == 16 or st["n_escalated_rows"] > 0)):
        out.append(f"{what}: the dealt short-list route did not run ({st['n_splits']} lists of {st['list_len']})")
    return out


def oracle_problems(q, y, k, metric, single, got_ind, strict, what="", skip_rows=None):
    """Index for index where the case is strict; else tie-tolerant (tie_tolerant_rows) with at most 5 % of the rows needing it.
    skip_rows: rows on which the oracle itself orders a pair against exact arithmetic although it is >= TIE_ULPS apart (random
    draws of tools/fuzz_values.py; the committed cases are proven to have none): not compared."""
    if strict:
        _, oi = oracle_knn(q, y, k, metric, exclude_self=single)
        n_bad = int((oi != got_ind).any(axis=1).sum())
        return [f"{what}: {n_bad} rows differ from the oracle"] if n_bad else []
    _, oi1 = gap_ulps(q, y, k, metric, exclude_self=single)
    needed, wrong = tie_tolerant_rows(q, y, k, metric, oi1, got_ind)
    if skip_rows is not None and len(skip_rows):
        needed, wrong = [r for r in needed if r not in set(skip_rows)], [r for r in wrong if r not in set(skip_rows)]
    out = []
    if wrong:
        out.append(f"{what}: {len(wrong)} rows differ from the oracle outside a run of near-ties (first: {wrong[:5]})")
    if len(needed) > 0.05 * len(got_ind):
        out.append(f"{what}: {len(needed)} of {len(got_ind)} rows need the tie allowance (> 5 %)")
    return out


def ratios_of(res):
    """{tier name: max_err_ratio} of a run_three result (the tier that actually ran first under each precision)."""
    out = {}
    for prec in PRECISIONS:
        st = res[prec][2]
        t = TIER_NAMES[st["first_pass"]]
        out[t] = max(out.get(t, 0.0), st["max_err_ratio"])
    return out


def check_knn_case(ctx, case, strict=None, skip_rows=None, routes=False):
    """One case of knn_cases() (or a random one of tools/fuzz_values.py) on the device.  Returns (problems, {tier: ratio}, stats of
    the default precision).  routes: also assert which tiers and which list route ran (route_problems)."""
    c = case
    strict = c["strict"] if strict is None else strict
    metric, k, single, short = c["metric"], c["k"], c["single"], c.get("short", 0)
    data = make(c)
    problems = []
    if c["regime"] in ("pow2", "cosine_row_scales"):
        (q0, y0), (q, y), e = data
        base = run_three(ctx, q0, y0, k, metric, single, short)
        res = run_three(ctx, q, y, k, metric, single, short)
        problems += three_problems(base, len(q0), "base")
        factor = pow2_factor(metric, e) if c["regime"] == "pow2" else 1.0
        if not np.array_equal(res[0][1], base[0][1]):
            problems.append(f"scaled indices differ from the unscaled run in {(res[0][1] != base[0][1]).any(axis=1).sum()} rows")
        if not np.array_equal(res[0][0], base[0][0] * factor):
            problems.append("scaled distances are not the unscaled ones times the exact factor, bit for bit")
        problems += oracle_problems(q0, y0, k, metric, single, base[0][1], strict, "base", skip_rows)
        if routes:
            problems += route_problems(base, c["d"], k, short, "base")
    else:
        q, y = data
        res = run_three(ctx, q, y, k, metric, single, short)
    problems += three_problems(res, len(q), "run")
    problems += oracle_problems(q, y, k, metric, single, res[0][1], strict, "run", skip_rows)
    if routes:
        problems += route_problems(res, c["d"], k, short, "run")
    if c["regime"] == "mismatch":
        od, _ = oracle_knn(q, y, k, metric)
        if not np.allclose(res[0][0], od, rtol=1e-9, atol=0):
            problems.append("distances differ from the oracle beyond rtol 1e-9")
    if c["regime"] == "outlier" and c["m"] >= 1e9 and (single or c["side"] in ("index", "both")):
        # the scale comes from the outlier: the fp16 image of every other row is all zeros -- rows must really have gone down
        if not res[0][2]["n_first_pass_fail"] > 0:
            problems.append("no row failed the first pass although the bulk's image is empty")
    return problems, ratios_of(res), res[0][2]
