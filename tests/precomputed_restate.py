"""numpy restatement of a search on a precomputed distance matrix (metric='precomputed'): nothing is computed, the lists ARE the rows
of the matrix in order.  Used by tests/test_precomputed.py (against scikit-learn) and tests/test_gpu_precomputed.py (against the
device).  The order among equal values is by index row (column of the row searched), as everywhere in the library."""
import numpy as np


def knn_rows(D: np.ndarray, k: int):
    """(dist [n, k] float64, ind [n, k] int64): the k smallest entries of every ROW of D by (value, column) -- a stable argsort."""
    D = np.asarray(D)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, order, axis=1).astype(np.float64), order.astype(np.int64)


def knn(D: np.ndarray, k: int, s_to_t: bool = True):
    """The search in either direction: source rows against the target side (rows of D), or target rows against the source side (rows
    of D.T)."""
    return knn_rows(D if s_to_t else np.ascontiguousarray(np.asarray(D).T), k)


def ranks(D: np.ndarray, gold: np.ndarray, s_to_t: bool = True) -> np.ndarray:
    """0-based position of column gold[i] in the full sorted row i (by (value, column)); -1 where gold[i] < 0."""
    M = np.asarray(D) if s_to_t else np.asarray(D).T
    order = np.argsort(M, axis=1, kind="stable")
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(M.shape[1]), M.shape), axis=1)
    gold = np.asarray(gold, dtype=np.int64)
    out = np.full(M.shape[0], -1, dtype=np.int64)
    has = gold >= 0
    out[has] = pos[np.nonzero(has)[0], gold[has]]
    return out


def grid_rows(rng, n_rows: int, n_cols: int, dtype) -> np.ndarray:
    """A matrix whose every row is a permutation of the grid 0, 1/8, 2/8, ...: distinct within a row by construction, and exact in
    float32 (multiples of 1/8 below 2^21)."""
    base = np.arange(n_cols, dtype=np.float64) / 8.0
    return np.stack([rng.permutation(base) for _ in range(n_rows)]).astype(dtype)
