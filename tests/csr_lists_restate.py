"""Helpers of the CSR pair-list tests (kz_match_csr, kz_assign_csr, kz_softmin_csr_rows, kz_sinkhorn_csr), numpy only.

A CSR pair list (indptr [n_q + 1], ind [nnz], dist [nnz]) holds the same pairs as the fixed-width lists it pads to: `pad` gives
those lists, and the numpy restatements of the fixed-width calls (tests/match_restate.py, tests/assignment_restate.py,
tests/sinkhorn_lists_restate.py) -- which have no limit on the number of columns -- are the reference of the CSR calls: the position
of an entry inside its row is its column."""
import numpy as np

# include/kiez_amd.h: KZ_CSR_LONG_ROW
LONG_ROW = 256
# the row lengths at which the kernels take another path: empty, one entry, around a wave, around the long-row switch, around one
# and two soft-min chunks, and past the 4 096 columns of the fixed-width calls
LENGTHS = (0, 1, 63, 64, 65, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 512, 513, 1025, 4100)


def pad(indptr, ind, dist):
    """[n_q, max_len] lists of a CSR: row i holds its entries in order, then ind = -1 / dist = NaN (no pair).  -> (dist, ind)"""
    indptr, ind, dist = np.asarray(indptr), np.asarray(ind), np.asarray(dist)
    n_q = indptr.size - 1
    lens = np.diff(indptr)
    width = max(int(lens.max()) if n_q else 0, 1)
    p_ind = np.full((n_q, width), -1, dtype=np.int64)
    p_dist = np.full((n_q, width), np.nan, dtype=dist.dtype)
    rows = np.repeat(np.arange(n_q), lens)
    cols = np.arange(ind.size) - np.repeat(indptr[:-1], lens)
    p_ind[rows, cols] = ind
    p_dist[rows, cols] = dist
    return p_dist, p_ind


def random_csr(rng, n_q, n_index, lengths, plain=False, dtype=np.float64):
    """A CSR with the row lengths `lengths` ({row: length}; the other rows get 0 .. 40 entries).  Values on a grid of 1 / 128 (ties
    between rows and inside a row), unsorted: a row's order is its own preference.  Target 0 is listed by every row that has an
    entry, target n_index - 1 by none; a row of at least two entries repeats a target.  Unless `plain`, rows of at least five
    entries get the ids -1 and n_index (no pair) somewhere behind their first two entries.  -> (indptr, ind, dist)"""
    lens = rng.integers(0, 41, size=n_q)
    for row, length in lengths.items():
        lens[row] = length
    indptr = np.zeros(n_q + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    ind = rng.integers(1, n_index - 1, size=int(indptr[-1])).astype(np.int64)
    dist = (rng.integers(0, 129, size=ind.size) / 128.0).astype(dtype)
    for i in range(n_q):
        a, n = int(indptr[i]), int(lens[i])
        if n == 0:
            continue
        if n <= 2:
            ind[a:a + n] = 0
        else:
            ind[a + 1] = ind[a]
            where = a + 2 + rng.choice(n - 2, size=min(n - 2, 3), replace=False)
            ind[where[0]] = 0
            if where.size == 3 and not plain:
                ind[where[1]], ind[where[2]] = -1, n_index
    return indptr, ind, dist


def cases():
    """[(name, n_index, {row: length})]: every length of LENGTHS once as the first and once as the last row of a CSR of 300 rows;
    n_index 600, or 5 000 where a row has 4 100 entries."""
    out = []
    for j, first in enumerate(LENGTHS):
        last = LENGTHS[len(LENGTHS) - 1 - j]
        out.append((f"first{first}_last{last}", 5000 if max(first, last) > 4096 else 600, {0: first, 299: last, 150: LONG_ROW + 44}))
    return out
