"""Plain Python / numpy restatements of what the kernels of kiez_amd/csrc/kz_analysis.hip compute (TEST INFRASTRUCTURE; numpy and
the standard library only, nothing of kiez_amd).

Integer results are Python ints or int64 arrays and are meant to be compared with ==.  A float sum is math.fsum over its float64
terms -- the correctly rounded sum of exactly the terms the device adds (x - m, d * d, d * d * d and sqrt are single correctly
rounded float64 operations on both sides, the library is built with -ffp-contract=off) -- and comes with the sum of the terms'
magnitudes, which sum_bound turns into the rounding bound of a float64 summation of those terms in ANY order.

tests/test_analysis_restate.py holds this file to the reference's own golden hubness scores before a kernel is judged by it."""
import math

import numpy as np

INT64_MIN = int(np.iinfo(np.int64).min)
INT64_MAX = int(np.iinfo(np.int64).max)
NO_GOLD = INT64_MIN

FLOAT_SUMS = ("abs_dev", "m2s", "m3s", "sqrt_sum")
# the ten doubles of kz_kocc_stats, in its order
STAT_ORDER = ("total", "abs_dev", "m2s", "m3s", "sqrt_sum", "kmax", "n_zero", "hub_sum", "n_hub", "gini_num")


def sum_bound(n_terms, abs_sum):
    """|float64 sum of n terms in any order - exact sum| <= (n - 1) u sum|t| / (1 - (n - 1) u), u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., section 4.2: any order, any tree).  Taken as 2 (n + 4) u sum|t|: the factor n + 4
    leaves three roundings inside a term and fsum's own final rounding, the factor 2 is slack.  Derived, not measured."""
    return 2.0 * (n_terms + 4) * 2.0 ** -53 * abs_sum


def k_occurrence(ind, k, n_bins):
    """np.bincount of the non-negative entries of ind[:, :k], n_bins long; an id >= n_bins is an error."""
    ids = np.asarray(ind, dtype=np.int64)[:, :k].ravel()
    ids = ids[ids >= 0]
    if ids.size and int(ids.max()) >= n_bins:
        raise ValueError(f"neighbour id {int(ids.max())} >= n_bins {n_bins}")
    return np.bincount(ids, minlength=n_bins).astype(np.int64)


def minmax(ind, k=None):
    """(smallest, largest) entry of ind, or of its first k columns."""
    a = np.asarray(ind, dtype=np.int64)
    if k is not None:
        a = a[:, :k]
    return int(a.min()), int(a.max())


def gini_numerator(kocc):
    """sum_i sum_j |x_i - x_j| in the sorted form 2 sum_i (2 i - n + 1) x_(i), in Python ints."""
    xs = sorted(np.asarray(kocc, dtype=np.int64).tolist())        # Python ints
    n = len(xs)
    return 2 * sum((2 * i - n + 1) * x for i, x in enumerate(xs))


def kocc_float_terms(kocc, mean):
    """The float64 terms of the four sums around `mean`, element by element: |d|, d d, (d d) d, sqrt(x) with d = x - mean."""
    x = np.asarray(kocc, dtype=np.int64).astype(np.float64)
    d = x - np.float64(mean)
    return {"abs_dev": np.abs(d), "m2s": d * d, "m3s": d * d * d, "sqrt_sum": np.sqrt(x)}


def kocc_stats(kocc, thr, with_gini=True):
    """The ten values of kz_kocc_stats as a dict (STAT_ORDER): exact ints for sum, max, #zeros, hub sum, hub count and the Gini
    numerator; math.fsum for the four float sums around m = float(sum) / float(n), the mean the library's host code passes to the
    device.  "abs_terms" holds sum|term| of each float sum (for sum_bound), "mean" is m."""
    kocc = np.asarray(kocc, dtype=np.int64)
    n = int(kocc.size)
    vals = kocc.tolist()                                          # Python ints
    total = sum(vals)
    mean = float(total) / float(n)
    hubs = [v for v in vals if float(v) >= thr]
    out = {
        "total": total,
        "kmax": max(max(vals), 0),
        "n_zero": sum(1 for v in vals if v == 0),
        "hub_sum": sum(hubs),
        "n_hub": len(hubs),
        "gini_num": gini_numerator(vals) if with_gini else 0,
        "mean": mean,
        "abs_terms": {},
    }
    for name, t in kocc_float_terms(kocc, mean).items():
        out[name] = math.fsum(t)
        out["abs_terms"][name] = math.fsum(np.abs(t))
    return out


def kocc_select(kocc, mode, thr):
    """Ascending ids with kocc == 0 (mode 0) or float(kocc) >= thr (mode 1)."""
    kocc = np.asarray(kocc, dtype=np.int64)
    return np.flatnonzero(kocc == 0 if mode == 0 else kocc.astype(np.float64) >= thr).astype(np.int64)


def hit_positions(ind, gold):
    """[cols + 1] histogram of the first column of ind[r] that holds gold[r]; bin `cols` counts the rows where it is absent; rows
    whose gold is INT64_MIN are skipped."""
    ind = np.asarray(ind, dtype=np.int64)
    gold = np.asarray(gold, dtype=np.int64)
    cols = ind.shape[1]
    hit = ind == gold[:, None]
    pos = np.where(hit.any(axis=1), hit.argmax(axis=1), cols)
    return np.bincount(pos[gold != NO_GOLD], minlength=cols + 1).astype(np.int64)


def max_abs_diff(a, b):
    """max |a - b| over the entries whose difference is not NaN; 0.0 when none is left."""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0


def rank_stats(rank, ks):
    """kz_rank_stats: ([#(0 <= rank < k) for k in ks], #(rank >= 0), sum(rank + 1) as an int, fsum of 1 / (rank + 1),
    sum|1 / (rank + 1)| (the same number: every term is positive))."""
    r = np.asarray(rank, dtype=np.int64)
    have = r[r >= 0]
    terms = 1.0 / (have + 1).astype(np.float64)
    recip = math.fsum(terms)
    return ([int(np.count_nonzero(have < k)) for k in ks], int(have.size), sum(int(v) + 1 for v in have), recip, recip)


def truncnorm_third_moment(a):
    """scipy.stats.truncnorm(a, +inf).moment(3): m3 = 2 m1 + a^2 phi(a) / Z, m1 = phi(a) / Z, Z = 1 - Phi(a)."""
    phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    z = 0.5 * math.erfc(a / math.sqrt(2.0))
    return 2.0 * (phi / z) + a * a * phi / z


def hubness_measures(kocc, k, n_test, hub_size=2.0):
    """The reference's hubness measures (kiez/analysis/estimation.py) from the k-occurrence histogram, by the closed forms
    kiez_amd/analysis.py uses on kocc_stats' values."""
    kocc = np.asarray(kocc, dtype=np.int64)
    thr = hub_size * k
    st = kocc_stats(kocc, thr)
    n = float(kocc.size)
    total = float(st["total"])
    mean = total / n
    m2, m3 = st["m2s"] / n, st["m3s"] / n
    std1 = math.sqrt(st["m2s"] / (n - 1.0)) if n > 1 else float("nan")
    return {
        "k_skewness": m3 / m2 ** 1.5 if m2 > 0 else float("nan"),
        "k_skewness_truncnorm": truncnorm_third_moment((0.0 - mean) / std1) if std1 and std1 > 0 else float("nan"),
        "atkinson": float(1.0 - 1.0 / mean * (st["sqrt_sum"] / n) ** 2),
        "gini": float(st["gini_num"]) / (2.0 * n * total),
        "robinhood": 0.5 * st["abs_dev"] / total,
        "antihubs": kocc_select(kocc, 0, thr),
        "antihub_occurrence": float(st["n_zero"]) / n,
        "hubs": kocc_select(kocc, 1, thr),
        "hub_occurrence": float(st["hub_sum"]) / k / n_test,
        "groupie_ratio": float(st["kmax"]) / n_test / k,
        "k_occurrence": kocc,
    }
