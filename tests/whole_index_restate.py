"""numpy restatement of kz_knn_reduced (include/kiez_amd.h): the k index rows with the smallest hubness-reduced distance over the whole
index are the first k of a stable sort of the reduced distances of tests/reduced_rank_restate.py by (w, row), NaN as +inf -- the
order whose positions kz_gold_ranks_reduced counts.  Test infrastructure only -- the product path never imports it."""
import numpy as np

from tests import reduced_rank_restate as RD


def topk(w, k):
    """w [n_q, n_i] -> (w [n_q, k] with NaN kept, index rows [n_q, k] int64): ascending by (w with NaN as +inf, row).  A stable sort
    keeps equal values in row order, and -0.0 == +0.0 to it."""
    w = np.asarray(w, dtype=np.float64)
    order = np.argsort(np.where(np.isnan(w), np.inf, w), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(w, order, axis=1), order.astype(np.int64)


def knn_reduced(kind, d, q_state, t_state, k):
    """topk of the reduced distances of the distances d [n_q, n_i] (RD.reduce)."""
    return topk(RD.reduce(kind, d, q_state, t_state), k)


def non_decreasing(w):
    """Every row of w ascends under NaN-as-+inf."""
    v = np.where(np.isnan(w), np.inf, np.asarray(w, dtype=np.float64))
    return bool((v[:, 1:] >= v[:, :-1]).all())
