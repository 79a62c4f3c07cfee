"""numpy restatement of kz_gold_ranks_reduced (include/kiez_amd.h): the rank of a known index row under a pointwise hubness
reduction is the count of tests/rank_restate.py over the reduced distances w = f(d, state of the query row, state of the index
row), by (w, row), NaN as +inf.  The formulas are the reference's, operation by operation (csls.py:90-93, local_scaling.py:135-147,
mutual_proximity.py:177-183).  Test infrastructure only -- the product path never imports it."""
import numpy as np
from scipy.special import ndtr

from tests import rank_restate as RR

NO_GOLD = RR.NO_GOLD
KINDS = ("csls", "ls", "nicdm", "mp_normal")          # kz_gold_ranks_reduced's kind = position + 1


def kind_id(kind):
    return KINDS.index(kind) + 1


def lists(d, K):
    """The K smallest distances of every row of d, ascending: the distances of a neighbour list of K."""
    return np.sort(np.asarray(d, dtype=np.float64), axis=1)[:, :K]


def state(kind, neigh_dist):
    """The state vectors one side contributes, from its [n, K] neighbour distances: (mean,) for csls / nicdm, (last,) for ls,
    (nanmean, nanstd) for mp_normal."""
    neigh_dist = np.asarray(neigh_dist, dtype=np.float64)
    if kind in ("csls", "nicdm"):
        return (neigh_dist.mean(axis=1),)
    if kind == "ls":
        return (neigh_dist[:, -1].copy(),)
    assert kind == "mp_normal"
    return (np.nanmean(neigh_dist, axis=1), np.nanstd(neigh_dist, axis=1))


def reduce(kind, d, q_state, t_state):
    """w [n_q, n_i] of the distances d [n_q, n_i]; q_state entries [n_q], t_state entries [n_i]."""
    d = np.asarray(d, dtype=np.float64)
    qa, ta = np.asarray(q_state[0])[:, None], np.asarray(t_state[0])[None, :]
    with np.errstate(all="ignore"):
        if kind == "csls":
            return 2.0 * d - qa - ta
        if kind == "ls":
            return 1.0 - np.exp(-1.0 * (d * d) / (qa * ta))
        if kind == "nicdm":
            return d / np.sqrt(qa * ta)
        assert kind == "mp_normal"
        qb, tb = np.asarray(q_state[1])[:, None], np.asarray(t_state[1])[None, :]
        return 1.0 - ndtr(-((d - qa) / qb)) * ndtr(-((d - ta) / tb))


def ranks(kind, d, q_state, t_state, gold):
    return RR.gold_ranks(reduce(kind, d, q_state, t_state), gold)


def bracket(w, gold, tol):
    """(lo, hi) per row: lo = #{w < w_g - tol}, hi = #{w <= w_g + tol} - 1 -- every rank a computation of w that is off by less
    than tol / 2 per entry can give.  NaN as +inf; rows without gold: (-1, -1)."""
    w = np.where(np.isnan(w), np.inf, np.asarray(w, dtype=np.float64))
    gold = np.asarray(gold, dtype=np.int64)
    ok = (gold >= 0) & (gold < w.shape[1])
    wg = w[np.arange(w.shape[0]), np.where(ok, gold, 0)][:, None]
    lo = (w < wg - tol).sum(axis=1)
    hi = (w <= wg + tol).sum(axis=1) - 1
    return np.where(ok, lo, -1), np.where(ok, hi, -1)
