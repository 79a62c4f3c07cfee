"""numpy restatement of the Sinkhorn / inverted-softmax potentials on neighbour lists (kz_lists_transpose, kz_softmin_list_rows,
kz_softmin_list_cols, kz_sinkhorn_lists; Sinkhorn / InvertedSoftmax with support="candidates"), float64 throughout.

dist / ind [n_q, k]: entry (i, c) is a PAIR of source row i and target row ind[i, c] when 0 <= ind[i, c] < n_t; any other id is none.
The potentials are those of tests/sinkhorn_restate.py with every value outside the pairs at +inf -- a dropped pair carries no mass --
except that a row or a column with no pair at all has NO value: NaN where the masked matrix gives +inf.

Two forms, asserted against each other in tests/test_sinkhorn_lists.py:
  * the MASKED MATRIX: D [n_q, n_t] with +inf outside the pairs, fed to SR.softmin / SR.sinkhorn_potentials (lists without a target
    repeated inside a row only: a matrix holds one value per pair);
  * the LIST / CSC form: rows reduced over their own entries, columns over the entries of the transposed view.
The transposition is a stable argsort of (target id | n_t for a non-pair) over the flat positions i k + c."""
import numpy as np

from tests import sinkhorn_restate as SR


def pairs(ind, n_t):
    """Boolean [n_q, k]: which entries are pairs."""
    ind = np.asarray(ind)
    return (ind >= 0) & (ind < n_t)


def masked_matrix(dist, ind, n_t):
    """D [n_q, n_t]: dist at the pairs, +inf elsewhere.  A target listed twice by one row has no place in a matrix: refused."""
    dist, ind = np.asarray(dist, dtype=np.float64), np.asarray(ind)
    ok = pairs(ind, n_t)
    rows = np.nonzero(ok)[0]
    flat = rows * n_t + ind[ok]
    assert np.unique(flat).size == flat.size, "a row lists a target twice: use the list form"
    D = np.full((dist.shape[0], n_t), np.inf)
    D[rows, ind[ok]] = dist[ok]
    return D


def transpose(dist, ind, n_t):
    """(colptr int64 [n_t + 1], col_row int32 [nnz], col_val float64 [nnz]): the entries of column j are colptr[j] .. colptr[j + 1] - 1,
    in ascending flat position i k + c."""
    dist, ind = np.asarray(dist, dtype=np.float64), np.asarray(ind)
    k = ind.shape[1]
    key = np.where(pairs(ind, n_t), ind, n_t).ravel()
    order = np.argsort(key, kind="stable")
    colptr = np.searchsorted(key[order], np.arange(n_t + 1), side="left").astype(np.int64)
    order = order[:colptr[n_t]]
    return colptr, (order // k).astype(np.int32), dist.ravel()[order]


def softmin_rows(dist, ind, n_t, eps, off=None, shift=0.0):
    """[n_q]: per row the soft-min over its pairs of dist - off[ind], plus shift; NaN for a row without a pair."""
    dist, ind = np.asarray(dist, dtype=np.float64), np.asarray(ind)
    ok = pairs(ind, n_t)
    x = dist if off is None else dist - np.asarray(off)[np.where(ok, ind, 0)]
    out = SR.softmin(np.where(ok, x, np.inf), eps, axis=1) + shift
    return np.where(ok.any(axis=1), out, np.nan)


def softmin_cols(colptr, col_row, col_val, eps, off=None, shift=0.0):
    """[n_t]: per column the soft-min over its entries of col_val - off[col_row], plus shift; NaN for a column without an entry."""
    x = col_val if off is None else col_val - np.asarray(off)[col_row]
    out = np.full(colptr.size - 1, np.nan)
    for j in np.nonzero(np.diff(colptr))[0]:
        out[j] = SR.softmin(x[colptr[j]:colptr[j + 1]], eps) + shift
    return out


def max_abs_diff(a, b):
    """kz_max_abs_diff: the largest |a - b| with NaN differences ignored, 0.0 when none is left."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0


def sinkhorn_potentials(dist, ind, n_t, eps, L, tol=None):
    """The list / CSC form -> (f [n_q], g [n_t], iterations done, last measured change of g or None).  Sinkhorn._potentials' loop:
    stop after the column step whose change is <= tol, the row step behind it still taken."""
    n_q = np.asarray(ind).shape[0]
    colptr, col_row, col_val = transpose(dist, ind, n_t)
    shift = eps * np.log(n_q / n_t)
    f = g = change = None
    done = 0
    for it in range(1, L + 1):
        g_new = softmin_cols(colptr, col_row, col_val, eps, off=f, shift=shift)
        if g is not None:
            change = max_abs_diff(g_new, g)
        g = g_new
        f = softmin_rows(dist, ind, n_t, eps, off=g)
        done = it
        if tol is not None and change is not None and change <= tol:
            break
    return f, g, done, change


def sinkhorn_potentials_masked(dist, ind, n_t, eps, L):
    """The masked-matrix form -> (f, g): SR.sinkhorn_potentials on the masked matrix, the +inf of an empty row / column turned into NaN."""
    D = masked_matrix(dist, ind, n_t)
    with np.errstate(invalid="ignore"):
        f, g = SR.sinkhorn_potentials(D, eps, L)
    f, g = f.copy(), g.copy()
    f[np.isinf(D).all(axis=1)] = np.nan
    g[np.isinf(D).all(axis=0)] = np.nan
    return f, g


def inverted_softmax_potential(dist, ind, n_t, eps):
    """g [n_t]: one column step from f = 0 without the constant."""
    return softmin_cols(*transpose(dist, ind, n_t), eps)


def candidate_lists(D, K):
    """The K nearest columns of every row of D by (value, column): what the forward search returns -> (dist, ind)."""
    ind = np.argsort(D, axis=1, kind="stable")[:, :K].astype(np.int64)
    return np.take_along_axis(D, ind, axis=1), ind


def list_w(dist, ind, f, g):
    """(dist - f_i) - g[ind]: kz_dual_shift over lists whose ids are all target rows."""
    return (dist - f[:, None]) - g[ind]


def topk_lists(w, ind, k):
    """The k best entries of every row by a stable sort of w (NaN last): what kneighbors(k) returns -> (w, ind)."""
    order = np.argsort(w, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(w, order, axis=1), np.take_along_axis(ind, order, axis=1)
