"""The minimum-cost assignment over neighbour lists, restated in numpy: the auction rule of kz_assign_lists round by round (the device
must agree with it to the bit), the optimum by scipy's dense solver, the cost of a matching and the certificate that a matching
and a price vector are optimal to within n_q * eps.

Entry (i, c) is a PAIR when 0 <= ind[i, c] < n_target, dist[i, c] widened to float64 is finite and that value is <= u; u is the
price a source row pays for staying unmatched."""
import numpy as np


def pairs(dist, ind, n_target, u):
    """(w float64 [n_q, k], ok bool [n_q, k]): the values widened, and which entries are pairs."""
    w = np.asarray(dist).astype(np.float64)
    ind = np.asarray(ind)
    with np.errstate(invalid="ignore"):
        ok = (ind >= 0) & (ind < n_target) & np.isfinite(w) & (w <= u)
    return w, ok


def value_range(dist, ind, n_target):
    """(smallest, largest) finite value listed with a target id in range; (0.0, 0.0) when there is none."""
    w = np.asarray(dist).astype(np.float64)
    ind = np.asarray(ind)
    w = w[(ind >= 0) & (ind < n_target) & np.isfinite(w)]
    return (float(w.min()), float(w.max())) if w.size else (0.0, 0.0)


def defaults(dist, ind, n_target, u=None, eps=None):
    """u and eps with the defaults of `matching.assignment`: the largest finite listed value, scale / (1000 n_q)."""
    lo, hi = value_range(dist, ind, n_target)
    scale = hi - lo if hi > lo else 1.0
    return (hi if u is None else float(u)), (scale / (1000.0 * max(len(dist), 1)) if eps is None else float(eps))


def auction(dist, ind, n_target, u, eps, max_rounds=1_000_000):
    """The rule: prices start at 0.0, every row FREE.  In a round every FREE row computes v_c = (-w_c) - price[t_c] over its pair
    columns; best = the first column with the largest v (v1); v2 = the largest v among its other pair columns together with -u.
    Not v1 > -u: unmatched for good.  Otherwise it bids (price[t] + (v1 - v2)) + eps on its best target.  A target takes the
    largest bid, among equal bids the smallest row; the bid becomes the price, the winner the owner, the previous owner FREE.
    -> (match int64 [n_q], col int64 [n_q], price float64 [n_target], rounds, converged)"""
    w, ok = pairs(dist, ind, n_target, u)
    ind = np.asarray(ind).astype(np.int64)
    n_q, k = w.shape
    u, eps = np.float64(u), np.float64(eps)
    tgt = np.where(ok, ind, 0)
    price = np.zeros(n_target, dtype=np.float64)
    owner = np.full(n_target, -1, dtype=np.int64)
    match = np.full(n_q, -1, dtype=np.int64)
    col = np.full(n_q, -1, dtype=np.int64)
    free = np.arange(n_q, dtype=np.int64)
    rounds = 0
    while free.size and rounds < max_rounds:
        rounds += 1
        p = price[tgt[free]]
        v = np.where(ok[free], (-w[free]) - p, -np.inf)
        rows = np.arange(free.size)
        best = np.argmax(v, axis=1)                        # (the first column with the largest v)
        v1 = v[rows, best]
        v[rows, best] = -np.inf
        v2 = np.maximum(v.max(axis=1), -u)
        bids = v1 > -u                                     # the others are unmatched for good: they leave `free`
        b_row, b_col = free[bids], best[bids]
        b_t = tgt[b_row, b_col]
        bid = (p[rows, best][bids] + (v1[bids] - v2[bids])) + eps
        order = np.lexsort((b_row, -bid, b_t))             # per target: the largest bid first, then the smallest row
        first = np.ones(order.size, dtype=bool)
        first[1:] = b_t[order][1:] != b_t[order][:-1]
        won = order[first]
        old = owner[b_t[won]]
        old = old[old >= 0]
        match[old] = -1
        col[old] = -1
        price[b_t[won]] = bid[won]
        owner[b_t[won]] = b_row[won]
        match[b_row[won]] = b_t[won]
        col[b_row[won]] = b_col[won]
        free = np.sort(np.concatenate([b_row[order[~first]], old]))
    return match, col, price, rounds, free.size == 0


def cost(dist, ind, n_target, u, match, col):
    """The sum of dist over the matched pairs plus u per unmatched source row (float64); asserts that `match`, `col` is a matching
    over pairs: every matched row names a pair column of its list that holds its target, no target twice."""
    w, ok = pairs(dist, ind, n_target, u)
    match, col = np.asarray(match), np.asarray(col)
    on = match >= 0
    assert ((col >= 0) == on).all()
    rows = np.nonzero(on)[0]
    assert ok[rows, col[rows]].all() and (np.asarray(ind)[rows, col[rows]] == match[rows]).all()
    assert len(np.unique(match[on])) == int(on.sum())
    return float(w[rows, col[rows]].sum() + float(u) * int((~on).sum()))


def optimum(dist, ind, n_target, u):
    """The least cost of any matching: the dense [n_q, n_target + n_q] matrix -- a pair's value (the smallest, where a row lists a
    target twice), +inf where there is no pair, and one private "stay out" column per row at cost u -- solved by scipy."""
    from scipy.optimize import linear_sum_assignment
    w, ok = pairs(dist, ind, n_target, u)
    n_q = w.shape[0]
    dense = np.full((n_q, n_target + n_q), np.inf)
    r, c = np.nonzero(ok)
    np.minimum.at(dense, (r, np.asarray(ind)[r, c]), w[r, c])
    dense[np.arange(n_q), n_target + np.arange(n_q)] = float(u)
    rr, cc = linear_sum_assignment(dense)
    return float(dense[rr, cc].sum())


def slack_violation(dist, ind, n_target, u, eps, match, col, price):
    """The number of rows and targets that break eps-complementary slackness, the certificate of cost <= optimum + n_q eps: a
    matched row has (-w - price[t]) >= max(over its pair columns of v, -u) - eps; an unmatched row has no pair column with
    v > -u; a target that no row holds has price 0.
    The first condition holds with equality in real arithmetic for a row whose second-best column has not changed since its bid:
    the bid is three rounded float64 operations on numbers of magnitude at most M = max |w|, |price|, |u| (their sums: 2 M), each
    v two more, so the compare allows 16 M 2^-52 of rounding on top of eps.  The other two conditions are compares of numbers the
    rule itself compared, and are exact."""
    w, ok = pairs(dist, ind, n_target, u)
    match, col, price = np.asarray(match), np.asarray(col), np.asarray(price, dtype=np.float64)
    big = max([abs(float(u)), float(np.abs(price).max()) if price.size else 0.0, float(np.abs(w[ok]).max()) if ok.any() else 0.0])
    eps = float(eps) + 16.0 * big * 2.0 ** -52
    v = np.where(ok, (-w) - price[np.where(ok, np.asarray(ind), 0)], -np.inf)
    top = np.maximum(v.max(axis=1), -float(u)) if v.shape[1] else np.full(len(v), -float(u))
    on = match >= 0
    rows = np.nonzero(on)[0]
    bad = int(np.count_nonzero(v[rows, col[rows]] < top[rows] - float(eps)))
    bad += int(np.count_nonzero(top[~on] > -float(u)))
    held = np.zeros(n_target, dtype=bool)
    held[match[on]] = True
    return bad + int(np.count_nonzero(price[~held] != 0.0))
