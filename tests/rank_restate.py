"""numpy restatement of kz_gold_ranks and kz_rank_stats (include/kiez_amd.h): the rank of a known index row is a count over the
float64 value matrix, by (value, row).  Test infrastructure only -- the product path never imports it."""
import numpy as np

NO_GOLD = np.iinfo(np.int64).min


def gold_ranks(vals, gold):
    """vals [n_q, n_i] float64 (the values the search ranks by; NaN ranks as +inf by row), gold [n_q] int64 -> rank [n_q] int64:
    #{ j : v_j < v_g or (v_j == v_g and j < g) }, -1 where gold is outside [0, n_i)."""
    vals = np.asarray(vals, dtype=np.float64)
    gold = np.asarray(gold, dtype=np.int64)
    n_q, n_i = vals.shape
    v = np.where(np.isnan(vals), np.inf, vals)
    ok = (gold >= 0) & (gold < n_i)
    g = np.where(ok, gold, 0)
    vg = v[np.arange(n_q), g][:, None]
    cols = np.arange(n_i)[None, :]
    before = (v < vg) | ((v == vg) & (cols < g[:, None]))
    return np.where(ok, before.sum(axis=1), -1).astype(np.int64)


def full_order(vals):
    """[n_q, n_i] index rows in the order kz_knn returns them for k = n_i: by value (NaN as +inf), ties by smaller row."""
    v = np.where(np.isnan(vals), np.inf, np.asarray(vals, dtype=np.float64))
    return np.argsort(v, axis=1, kind="stable")


def positions(ind, gold):
    """Position of gold[r] in the list ind[r, :] (-1: absent or no gold)."""
    ind = np.asarray(ind)
    gold = np.asarray(gold, dtype=np.int64)
    hit = ind == gold[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int64)


def rank_stats(ranks, ks):
    """kz_rank_stats: ([#(0 <= rank < k) for k in ks], #(rank >= 0), sum(rank + 1), sum 1 / (rank + 1))."""
    r = np.asarray(ranks, dtype=np.int64)
    have = r[r >= 0]
    return ([int(np.count_nonzero(have < k)) for k in ks], int(have.size), float((have + 1).sum()),
            float((1.0 / (have + 1)).sum()))
