"""numpy restatement of the neighbour-pair calls (kz_lists_combine, kz_pairs_values): the set step over two
list arrays and "the value of a pair is the table entry".  Python sets and loops, nothing shared with the device code or with
the dense boolean matrices tests/test_neighbor_pairs.py checks it against."""
import numpy as np

MODES = ("forward", "reverse", "union", "mutual")


def pair_sets(fwd_ind, rev_ind, n_source, n_target):
    """(F, R): per source row the set of target rows its forward list names, and the set of target rows whose reverse list names it.
    An id outside its range (-1, INT_MAX padding, >= n) is no pair; a repeated id counts once (a set)."""
    F = [set() for _ in range(n_source)]
    R = [set() for _ in range(n_source)]
    if fwd_ind is not None:
        for i, row in enumerate(np.asarray(fwd_ind)):
            F[i] = {int(j) for j in row if 0 <= j < n_target}
    if rev_ind is not None:
        for j, row in enumerate(np.asarray(rev_ind)):
            for i in row:
                if 0 <= i < n_source:
                    R[int(i)].add(j)
    return F, R


def combine(fwd_ind, rev_ind, mode, n_source=None, n_target=None):
    """-> (indptr int64 [n_source + 1], ind int64 [total]): the pairs of `mode` as a CSR over the source rows, a row ascending by
    target id."""
    assert mode in MODES
    n_source = np.asarray(fwd_ind).shape[0] if n_source is None else n_source
    n_target = np.asarray(rev_ind).shape[0] if n_target is None else n_target
    F, R = pair_sets(fwd_ind if mode != "reverse" else None, rev_ind if mode != "forward" else None, n_source, n_target)
    rows = []
    for f, r in zip(F, R):
        keep = f if mode == "forward" else r if mode == "reverse" else f | r if mode == "union" else f & r
        rows.append(sorted(keep))
    indptr = np.zeros(n_source + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    ind = np.array([j for r in rows for j in r], dtype=np.int64)
    return indptr, ind


def row_of(indptr):
    """The source row of every entry of a CSR."""
    return np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))


def values(indptr, ind, table):
    """The value of every entry: table[i, j] -- `table` a dense [n_source, n_target] array of pair values."""
    return np.asarray(table)[row_of(indptr), ind]


def sort_rows(indptr, ind, val):
    """Rows ascending by (value, target row) in kz_knnr_key's order: NaN as +inf, -0.0 equal to +0.0, ties by target row."""
    key = np.where(np.isnan(val), np.inf, val) + 0.0   # (-0.0 + 0.0 = +0.0)
    order = np.lexsort((ind, key, row_of(indptr)))
    return ind[order], val[order]


def table_from_csr(indptr, ind, val, n_target):
    """The CSR of `radius_neighbors(inf)` (every pair whose value is no NaN, any order inside a row) as the dense table of pair
    values: a pair the CSR does not hold has the value NaN."""
    n_source = indptr.shape[0] - 1
    table = np.full((n_source, n_target), np.nan, dtype=val.dtype)
    table[row_of(indptr), ind] = val
    return table
