"""numpy restatement of kz_radius_neighbors / kz_radius_neighbors_reduced (include/kiez_amd.h): every pair within a threshold is the
full matrix of the values w -- the distances themselves, or their reduced distances of tests/reduced_rank_restate.py -- thresholded
by w <= radius (NaN: never) and each row ordered by (w, row), the order of tests/whole_index_restate.py, or by row alone.  Test
infrastructure only -- the product path never imports it."""
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
