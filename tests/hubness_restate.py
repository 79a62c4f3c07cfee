"""Plain Python / numpy restatements of what the rescaling kernels of kiez_amd/csrc/kz_hubness.hip compute (TEST INFRASTRUCTURE).

pairwise_sum and the statistics built on it are numpy's summation tree as the device restates it (kz_np_pairwise_sum,
kz_np_pairwise_terms): tests/test_hubness_restate.py checks them against numpy bit for bit on the host, the GPU tests check the
device against numpy, so both ends of "Hubness kernels reproduce numpy's summation order" are pinned.

mp_empiric_rows restates mutual_proximity.py:185-212 in O(K (K + Kt)) per row (the oracle's form builds a K x Kt x K array).

dsl_fit_exact / dsl_transform_exact evaluate DisSimLocal in fractions.Fraction (every float converts exactly), and
dsl_fit_bound / dsl_transform_bound give the per-element rounding bound of the device's float64 evaluation from its operation count.
"""
from fractions import Fraction

import numpy as np


# ---- numpy's pairwise summation ---------------------------------------------------------------------------------------------
def pairwise_sum(a):
    """Sum of the float64 sequence a in the order of numpy's DOUBLE_pairwise_sum (a contiguous run): fewer than 8 elements one
    after the other, up to 128 in eight interleaved accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and then the
    tail, anything longer split at n // 2 rounded down to a multiple of 8."""
    a = [float(x) for x in a]
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res += x
        return res
    if n <= 128:
        r = a[:8]
        i = 8
        while i < n - (n % 8):
            for u in range(8):
                r[u] += a[i + u]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in a[i:]:
            res += x
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def _div(x, y):
    """x / y as IEEE float64 (0 / 0 = NaN, the all-NaN row of the NaN forms)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(x) / np.float64(y))


def mean(a):
    """ndarray.mean of one row: a NaN propagates."""
    return _div(pairwise_sum(a), len(a))


def std(a):
    """ndarray.std (ddof = 0) of one row."""
    m = mean(a)
    return float(np.sqrt(np.float64(_div(pairwise_sum([(float(x) - m) * (float(x) - m) for x in a]), len(a)))))


def nanmean(a):
    """np.nanmean of one row: NaN counts as 0 inside the same full-length tree, the sum is divided by the number of entries that
    are not NaN; a row of NaN only gives NaN."""
    a = [float(x) for x in a]
    cnt = sum(1 for x in a if x == x)
    return _div(pairwise_sum([x if x == x else 0.0 for x in a]), cnt)


def nanstd(a):
    """np.nanstd (ddof = 0) of one row: (x - avg) first, then the NaN positions set to 0, then square and sum."""
    a = [float(x) for x in a]
    cnt = sum(1 for x in a if x == x)
    avg = nanmean(a)
    dev = [(x - avg) if x == x else 0.0 for x in a]
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(_div(pairwise_sum([t * t for t in dev]), cnt))))


def rows(fn, arr):
    """fn over the rows of a 2-D array -> float64 [n]."""
    return np.array([fn(r) for r in np.asarray(arr, dtype=np.float64)], dtype=np.float64)


# ---- MutualProximity empiric ------------------------------------------------------------------------------------------------
def mp_empiric_rows(dist, ind, dist_t2s, ind_t2s):
    """mutual_proximity.py:185-212 row by row.  For query i and candidate j with id c_j:
        T_j[m] = dist_t2s[c_j, p] where ind_t2s[c_j, p] == c_m, else dist_t2s[c_j, Kt - 1] + 1e-6
        out[i, j] = 1 - #{m : d[i, m] > d[i, j] and T_j[m] > d[i, j]} / K
    (a dict from candidate id to position, one vectorised compare per j).  Where a reverse list names one id twice the LAST
    position wins, as in the oracle's fancy assignment; kNN lists hold distinct ids."""
    dist, ind = np.asarray(dist, dtype=np.float64), np.asarray(ind, dtype=np.int64)
    n, K = dist.shape
    out = np.empty((n, K), dtype=np.float64)
    for i in range(n):
        d = dist[i]
        pos = {}
        for m, c in enumerate(ind[i].tolist()):
            pos.setdefault(c, []).append(m)
        for j in range(K):
            cj = int(ind[i, j])
            rd, ri = dist_t2s[cj], ind_t2s[cj]
            T = np.full(K, rd[-1] + 1e-6, dtype=np.float64)
            for p, s in enumerate(ri.tolist()):
                for m in pos.get(s, ()):
                    T[m] = rd[p]
            out[i, j] = 1.0 - np.count_nonzero((d > d[j]) & (T > d[j])) / K
    return out


# ---- DisSimLocal, exact -----------------------------------------------------------------------------------------------------
def _frac_rows(a):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(a)]


def dsl_fit_exact(ind_t2s, source, target_rows):
    """t2c[j] = sum_k (t_jk - (sum_m s[ind[j, m], k]) / Kt)^2 in exact rational arithmetic -> list of Fraction."""
    s, t = _frac_rows(source), _frac_rows(target_rows)
    out = []
    for j, ids in enumerate(np.asarray(ind_t2s).tolist()):
        kt = len(ids)
        acc = Fraction(0)
        for k in range(len(t[j])):
            c = sum((s[m][k] for m in ids), Fraction(0)) / kt
            acc += (t[j][k] - c) ** 2
        out.append(acc)
    return out


def dsl_transform_exact(ind, query_rows, target, t2c):
    """out[i, m] = |q_i - t_c|^2 - |q_i - mean_m t_c|^2 - t2c[c] (c = ind[i, m]) exactly, t2c taken as given (float64)."""
    q, t = _frac_rows(query_rows), _frac_rows(target)
    out = []
    for i, ids in enumerate(np.asarray(ind).tolist()):
        K, d = len(ids), len(q[i])
        s2c = Fraction(0)
        for k in range(d):
            c = sum((t[m][k] for m in ids), Fraction(0)) / K
            s2c += (q[i][k] - c) ** 2
        row = []
        for c_ in ids:
            acc = sum(((q[i][k] - t[c_][k]) ** 2 for k in range(d)), Fraction(0))
            row.append(acc - s2c - Fraction(float(t2c[c_])))
        out.append(row)
    return out


# ---- DisSimLocal, rounding bounds of a float64 evaluation --------------------------------------------------------------------
U = Fraction(1, 2 ** 53)


def gamma(n):
    """gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return n * U / (1 - n * U)


def _sq_bound(x_rows, ids, against, terms):
    """Bound on |computed - exact| of S = sum_k (x_k - c_k)^2, c_k = mean over the rows `ids` of `against`, and the exact S.
    With e_k = gamma_{Kt} mean_m |a_mk| (the centroid: Kt - 1 additions and one division, each (1 + delta); the conversions are
    exact), the computed difference is (x_k - c_k + eps_k)(1 + delta) with |eps_k| <= e_k, so its square differs from the exact
    one by at most 2 |x_k - c_k| e_k + e_k^2 before the roundings of the difference, the product and the sum: a lane adds
    ceil(d / 64) terms and the butterfly six more, the difference counts twice and the product once -> gamma_{terms + 9} of
    the perturbed sum of squares."""
    kt = len(ids)
    S = Fraction(0)
    pert = Fraction(0)
    for k in range(len(x_rows)):
        col = [against[m][k] for m in ids]
        c = sum(col, Fraction(0)) / kt
        e = gamma(kt) * sum((abs(v) for v in col), Fraction(0)) / kt
        df = abs(x_rows[k] - c)
        S += df * df
        pert += 2 * df * e + e * e
    return S, pert + gamma(terms + 9) * (S + pert)


def dsl_fit_bound(ind_t2s, source, target_rows):
    """Per-row bound on |t2c computed in float64 in any of the orders described - exact t2c| -> list of Fraction."""
    s, t = _frac_rows(source), _frac_rows(target_rows)
    d = len(t[0])
    terms = -(-d // 64)
    return [_sq_bound(t[j], ids, s, terms)[1] for j, ids in enumerate(np.asarray(ind_t2s).tolist())]


def dsl_transform_bound(ind, query_rows, target, t2c):
    """Per-element bound for out[i, m]: the bound of |q_i - centroid|^2 as in the fit, gamma_{terms + 9} of |q_i - t_c|^2 (no
    centroid: the difference is one rounding of exact inputs), and u of each of the two subtractions' results, which are at most
    the sum of the magnitudes (1 + u) -> 2 u (A + S + |t2c|)(1 + u) covers both."""
    q, t = _frac_rows(query_rows), _frac_rows(target)
    d = len(q[0])
    terms = -(-d // 64)
    out = []
    for i, ids in enumerate(np.asarray(ind).tolist()):
        S, bS = _sq_bound(q[i], ids, t, terms)
        row = []
        for c_ in ids:
            A = sum(((q[i][k] - t[c_][k]) ** 2 for k in range(d)), Fraction(0))
            bA = gamma(terms + 9) * A
            mag = A + bA + S + bS + abs(Fraction(float(t2c[c_])))
            row.append(bA + bS + 2 * U * (1 + U) * mag)
        out.append(row)
    return out
