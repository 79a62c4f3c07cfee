"""The one-to-one matching of kz_match_lists restated in numpy / plain Python (no GPU): the ordering rule, a sequential
Gale-Shapley, the greedy assignment and the blocking pairs of a matching.

Lists: dist [n_q, k] floating point, ind [n_q, k] integer.  Entry (i, c) with 0 <= ind[i, c] < n_index is a pair of source row i
and target row ind[i, c] with value dist[i, c]; any other entry is no pair.  A source row prefers its pairs by column, a target row
the sources that list it by (key(value), source row), smaller first."""
import numpy as np


def key(w):
    """The order of values as one uint64 per value (kz_knnr_key on the value widened to double): NaN as +inf, -0.0 as +0.0,
    negative values in order, -inf first."""
    w = np.array(w, dtype=np.float64, copy=True)
    w[np.isnan(w)] = np.inf
    w[w == 0.0] = 0.0
    b = w.view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def _is_pair(ind, n_index):
    return (ind >= 0) & (ind < n_index)


def gale_shapley(dist, ind, n_index, descending=False):
    """Source-proposing deferred acceptance, one proposal at a time; free sources are taken in ascending row order (descending
    with `descending`: the result is the same).  -> (match [n_q], col [n_q]) int64, -1 where a row stays unmatched."""
    dist, ind = np.asarray(dist), np.asarray(ind)
    n_q, k = ind.shape
    keys = key(dist).tolist()
    ids = ind.tolist()
    held = {}                      # target -> (key, source row, column)
    nxt = [0] * n_q
    free = list(range(n_q))
    if not descending:
        free.reverse()             # (a stack: the smallest row on top)
    while free:
        i = free.pop()
        while nxt[i] < k:
            c = nxt[i]
            t = ids[i][c]
            if not 0 <= t < n_index:
                nxt[i] += 1
                continue
            mine = (keys[i][c], i, c)
            cur = held.get(t)
            if cur is None:
                held[t] = mine
                break
            if mine[:2] < cur[:2]:
                held[t] = mine
                nxt[cur[1]] += 1   # the displaced row moves one column on
                free.append(cur[1])
                break
            nxt[i] += 1
    match, col = np.full(n_q, -1, dtype=np.int64), np.full(n_q, -1, dtype=np.int64)
    for t, (_, i, c) in held.items():
        match[i], col[i] = t, c
    return match, col


def greedy(dist, ind, n_index):
    """All pairs sorted by (key, source row, column); a pair is taken when both of its ends are still free.  Equals `gale_shapley`
    where every row of dist is non-decreasing in key order.  -> (match, col)."""
    dist, ind = np.asarray(dist), np.asarray(ind)
    n_q, k = ind.shape
    rows, cols = np.divmod(np.arange(n_q * k, dtype=np.int64), k)
    ok = _is_pair(ind, n_index).ravel()
    rows, cols, tgt, keys = rows[ok], cols[ok], ind.ravel()[ok], key(dist).ravel()[ok]
    order = np.lexsort((cols, rows, keys))
    match, col = np.full(n_q, -1, dtype=np.int64), np.full(n_q, -1, dtype=np.int64)
    taken = np.zeros(n_index, dtype=bool)
    for i, c, t in zip(rows[order].tolist(), cols[order].tolist(), tgt[order].tolist()):
        if match[i] < 0 and not taken[t]:
            match[i], col[i], taken[t] = t, c, True
    return match, col


def blocking_pairs(dist, ind, n_index, match):
    """The listed pairs (i, c) that block the matching `match` = (match, col): source row i is unmatched or prefers column c to its
    own, and the target ind[i, c] is free or prefers (key, i) to its holder."""
    dist, ind = np.asarray(dist), np.asarray(ind)
    m, col = match
    keys = key(dist)
    holder = {int(t): (int(keys[i, col[i]]), i) for i, t in enumerate(m) if t >= 0}
    out = []
    for i in range(ind.shape[0]):
        upto = ind.shape[1] if m[i] < 0 else int(col[i])
        for c in range(upto):
            t = int(ind[i, c])
            if not 0 <= t < n_index:
                continue
            if t not in holder or (int(keys[i, c]), i) < holder[t]:
                out.append((i, c))
    return out
