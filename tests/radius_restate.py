"""numpy restatement of kz_radius_neighbors / kz_radius_neighbors_reduced (include/kiez_amd.h): every pair within a threshold is the
full matrix of the values w -- the distances themselves, or their reduced distances of tests/reduced_rank_restate.py -- thresholded
by w <= radius (NaN: never) and each row ordered by (w, row), the order of tests/whole_index_restate.py, or by row alone; the
sort's key in numpy, and the precomputed matrices with chosen row lengths and keys that tests/test_gpu_radius_sort.py drives the
row sort and the chunk scan with.  Test infrastructure only -- the product path never imports it."""
import numpy as np

from tests import reduced_rank_restate as RD


def csr(w, radius, sort_results=True):
    """w [n_q, n_i] -> (indptr int64 [n_q + 1], ind int64 [total], values float64 [total]): row i holds the j with w_ij <= radius,
    ascending by (w, j) -- a stable sort of the row's entries, which come ascending by j; -0.0 == +0.0 to it -- or by j."""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = w <= radius                       # (NaN <= radius: False, also for radius = +inf)
    indptr = np.zeros(w.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(inside.sum(axis=1))
    ind, val = [], []
    for row, keep in zip(w, inside):
        j = np.flatnonzero(keep)
        if sort_results:
            j = j[np.argsort(row[j], kind="stable")]
        ind.append(j)
        val.append(row[j])
    return indptr, np.concatenate(ind).astype(np.int64), np.concatenate(val)


def radius_reduced(kind, d, q_state, t_state, radius, sort_results=True):
    """csr of the reduced distances of the distances d [n_q, n_i] (RD.reduce)."""
    return csr(RD.reduce(kind, d, q_state, t_state), radius, sort_results)


def rows(indptr, flat):
    """The per-row pieces of a CSR array."""
    return np.split(np.asarray(flat), np.asarray(indptr)[1:-1])


def order_key(w):
    """kz_knnr_key (kiez_amd/csrc/kz_order_key.h) in numpy, uint64: NaN takes +inf's pattern and -0.0 that of +0.0; then a value
    with the sign bit set has all its bits flipped, any other gets the sign bit set.  Unsigned keys order like the doubles."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    b = w.view(np.uint64).copy()
    b[np.isnan(w)] = np.uint64(0x7FF0000000000000)
    b[w == 0.0] = np.uint64(0)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(0x8000000000000000))


def radix_passes(values):
    """The 8-bit shifts at which the keys of `values` do not all have the same digit: the passes the radix path of
    kz_radius_sort_kernel runs on a row of these values (it skips the others)."""
    key = order_key(np.ravel(values))
    differ = int(np.bitwise_or.reduce(key) ^ np.bitwise_and.reduce(key))
    return [shift for shift in range(0, 64, 8) if (differ >> shift) & 0xFF]


def byte_values(rng, n, shifts):
    """n float64 values with the bit pattern 0x3FF0000000000000 ^ (b << shift) for every shift of `shifts`, b uniform in [0, 256)
    -- [0, 0x40) at shift 56, which keeps the sign and the top exponent bit clear: every value is finite and >= 0 (what a
    precomputed matrix needs), and their keys differ in exactly the bytes named."""
    bits = np.full(n, 0x3FF0000000000000, dtype=np.uint64)
    for shift in shifts:
        assert shift % 8 == 0 and 0 <= shift < 64, shift
        bits ^= rng.integers(0, 0x40 if shift == 56 else 256, n).astype(np.uint64) << np.uint64(shift)
    return bits.view(np.float64)


# ---- planted precomputed matrices for the row sort (tests/test_gpu_radius_sort.py; checked on the host by tests/test_radius.py) ----
SORT_LDS = 4096          # KZ_RADIUS_SORT_LDS: rows of up to this many entries are sorted in LDS, longer ones by the radix path
PLANT_N_INDEX = 9000     # two chunks of 8192 (KZ_RADIUS_CHUNK)
OUTSIDE = 1e300          # every entry that is not planted: finite, and beyond every radius
# entries <= radius per row, out of order: 0 / 1 (nothing to sort), both sides of every power of two the bitonic network pads to
# from 2 to 4096, 4096 | 4097 (LDS | radix), radix rows with a last tile of 1 (4097, 4353), 255 (4351), 256 (4352, 8192) and 40
# (9000: the whole index) entries -- and short rows behind radix rows at arbitrary offsets.
LENGTHS = (4097, 0, 513, 1, 4096, 2, 1023, 9000, 3, 1024, 255, 4095, 1025, 256, 4352, 2047, 257, 2048, 4353, 511, 2049, 512, 4351, 8192)
BYTE_REGIMES = tuple((s,) for s in range(0, 64, 8)) + ((0, 56), (8, 24, 40))
REGIMES = ("distinct", "grid8", "equal") + BYTE_REGIMES
# the passes of the radix path on a row of 9000 values of the regime
REGIME_PASSES = {"distinct": list(range(0, 56, 8)), "grid8": [48, 56], "equal": [], **{r: list(r) for r in BYTE_REGIMES}}


def regime_id(regime):
    return regime if isinstance(regime, str) else "bytes_" + "_".join(str(s) for s in regime)


def regime_values(rng, regime, n):
    """n values of a key regime: 'distinct' (uniform in [0, 1): all passes below the exponent's top byte), 'grid8' (k / 8, k = 0 .. 8,
    every zero -0.0 or +0.0 at random: mass ties, and the two zeros tie by row), 'equal' (one value: the order is by row alone), or
    a tuple of shifts (byte_values)."""
    if regime == "distinct":
        return rng.random(n)
    if regime == "grid8":
        v = rng.integers(0, 9, n) / 8.0
        return np.where((v == 0.0) & (rng.random(n) < 0.5), -0.0, v)
    if regime == "equal":
        return np.full(n, 0.625)
    return byte_values(rng, n, regime)


_PLANTED = {}


def planted(regime, dtype=np.float64):
    """(D [len(LENGTHS), PLANT_N_INDEX] of `dtype`, radius): row i holds exactly LENGTHS[i] values of `regime` at a random subset of
    its columns, every other entry is OUTSIDE (float32: 1e30, which float32 holds); radius = the largest planted value.  The row
    length 9000 is even, so the 24 value rows of the exact stage start at even elements when the rows view is the query; with the
    columns view as query a value row has 24 entries.  Built once per (regime, dtype) and shared: do not modify."""
    key = (regime, np.dtype(dtype).name)
    if key not in _PLANTED:
        rng = np.random.default_rng([REGIMES.index(regime), 4096])
        outside = OUTSIDE if np.dtype(dtype) == np.float64 else 1e30
        D = np.full((len(LENGTHS), PLANT_N_INDEX), outside, dtype=dtype)
        for i, n in enumerate(LENGTHS):
            cols = np.sort(rng.choice(PLANT_N_INDEX, n, replace=False))
            D[i, cols] = regime_values(rng, regime, n)
        inside = D < outside
        radius = float(D[inside].max())
        D.setflags(write=False)
        _PLANTED[key] = (D, radius)
    return _PLANTED[key]


SIGNED_NAN = (0, 4096, 8999)        # index rows whose potential is NaN: w is NaN, in no row at any radius
SIGNED_TO_MINUS_INF = (1, 4097)     # potential +inf: w = -inf, first in every row, by row
SIGNED_TO_PLUS_INF = (4095, 8191)   # potential -inf: w = +inf, last in every row, by row
SIGNED_RADII = (np.inf, 0.0, -3.0, -4.5, -np.inf)


def signed_case():
    """(D [6, 9000], q_a [6], t_a [9000], w [6, 9000]): a precomputed matrix on the grid k / 128 in [0, 8) under the dual form
    w = (D - q_a) - t_a (KZ_RANK_DUAL) with q_a = 4 and t_a on the grid k / 2 in [-1, 1] -- every difference is exact, so numpy's w
    has the device's bits -- and NaN, +inf and -inf planted into t_a at both ends, around 4096 and at the chunk's last row.  w is
    negative, zero (exactly, many times) and positive, with long ties.  Shared: do not modify."""
    if "signed" not in _PLANTED:
        rng = np.random.default_rng(1)
        D = rng.integers(0, 1024, (6, PLANT_N_INDEX)) / 128.0
        q_a = np.full(6, 4.0)
        t_a = rng.integers(-2, 3, PLANT_N_INDEX) / 2.0
        t_a[list(SIGNED_NAN)] = np.nan
        t_a[list(SIGNED_TO_MINUS_INF)] = np.inf
        t_a[list(SIGNED_TO_PLUS_INF)] = -np.inf
        w = (D - q_a[:, None]) - t_a[None, :]
        for a in (D, q_a, t_a, w):
            a.setflags(write=False)
        _PLANTED["signed"] = (D, q_a, t_a, w)
    return _PLANTED["signed"]


CARRY_N_INDEX = 256 * 8192 + 1      # 257 chunks of KZ_RADIUS_CHUNK: one beyond the 256 a tile of kz_radius_scan_rows_kernel scans
CARRY_ROW0 = (0, 1, 8191, 8192, 255 * 8192 - 1, 255 * 8192, 256 * 8192 - 1, 256 * 8192)


def carry_case():
    """(D float32 [2, CARRY_N_INDEX], radius 1.0): every entry 2.0 except -- row 0: eight values <= 1, descending with the column, at
    both ends of chunks 0, 255 (the last of the scan's first tile) and of the one-entry chunk 256; row 1: 5000 random columns with
    uniform values and 0.0 in the last column, a radix row whose smallest entry lies behind the carry of 256 chunks.  Shared: do
    not modify."""
    if "carry" not in _PLANTED:
        rng = np.random.default_rng(257)
        D = np.full((2, CARRY_N_INDEX), 2.0, dtype=np.float32)
        D[0, list(CARRY_ROW0)] = (8 - np.arange(8)) / 8.0
        D[1, rng.choice(CARRY_N_INDEX - 1, 5000, replace=False)] = rng.random(5000, dtype=np.float32)
        D[1, -1] = 0.0
        D.setflags(write=False)
        _PLANTED["carry"] = (D, 1.0)
    return _PLANTED["carry"]


def gap_radius(w, per_row=20, window=2000):
    """(radius, gap): the midpoint of the widest gap among the `window` sorted values of w around the (per_row n_q)-th smallest, and
    that gap's width: about per_row pairs per row, and no pair closer to the radius than gap / 2, so that a computation of w that
    is off by less than that decides every pair the same way."""
    w = np.asarray(w, dtype=np.float64)
    flat = np.sort(w[~np.isnan(w)], axis=None)
    centre = min(per_row * w.shape[0], flat.size - 1)
    half = min(window // 2, centre // 2)           # (never down into the sparse tail of the smallest values, where the widest gaps are)
    lo, hi = centre - half, min(centre + half + 1, flat.size)
    gaps = np.diff(flat[lo:hi])
    at = int(np.argmax(gaps))
    return float(flat[lo + at] + 0.5 * gaps[at]), float(gaps[at])
