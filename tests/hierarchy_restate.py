"""numpy restatement of kz_forest_csr / kz_forest_lists and the weighted pair lists its tests share.

The minimum spanning forest of the weighted pair graph: source row i is node i, target row j node n_q + j, entry p an edge when
0 <= ind[p] < n_t and its value is not NaN.  A SEQUENTIAL Kruskal that takes the edges in the order (order key of the value, p) --
the key makes -0.0 equal +0.0 and puts -inf first -- so the forest is the unique one under that strict total order.  A cut is
tests/components_restate.py on the entries with value <= t.  tests/test_hierarchy.py checks both against scipy;
tests/test_gpu_hierarchy.py checks the device against them bit for bit."""
import numpy as np

from tests import components_restate as CR

INT_MAX = CR.INT_MAX


def order_key(w):
    """kz_knnr_key of float64 values: uint64 keys that order like the values, -0.0 == +0.0, -inf first (NaN as +inf: never an edge)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    b = w.view(np.uint64).copy()
    b[np.isnan(w)] = np.uint64(0x7ff0000000000000)
    b[w == 0.0] = np.uint64(0)
    neg = (b >> np.uint64(63)) == np.uint64(1)
    return np.where(neg, ~b, b | np.uint64(0x8000000000000000))


def forest(indptr, ind, dist, n_t):
    """-> (source int64 [m], target int64 [m], value float64 [m], entry int64 [m], C)."""
    indptr, ind = np.asarray(indptr, dtype=np.int64), np.asarray(ind, dtype=np.int64)
    w = np.asarray(dist).astype(np.float64)   # (float32 widens exactly)
    n_q = len(indptr) - 1
    n = n_q + n_t
    rows = np.repeat(np.arange(n_q, dtype=np.int64), np.diff(indptr))
    p = np.flatnonzero((ind >= 0) & (ind < n_t) & ~np.isnan(w))
    p = p[np.lexsort((p, order_key(w[p])))]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    taken = []
    for e, a, b in zip(p.tolist(), rows[p].tolist(), (ind[p] + n_q).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            taken.append(e)
    e = np.array(taken, dtype=np.int64)
    return rows[e], ind[e], w[e], e, n - e.shape[0]


def forest_lists(dist, ind, n_t):
    ind = np.asarray(ind, dtype=np.int64)
    return forest(ind.shape[1] * np.arange(ind.shape[0] + 1, dtype=np.int64), ind.reshape(-1), np.asarray(dist).reshape(-1), n_t)


def restrict(indptr, ind, dist, t):
    """The CSR of the entries with value <= t (IEEE comparison: a NaN value goes), rows and order kept -> (indptr, ind)."""
    indptr, ind = np.asarray(indptr, dtype=np.int64), np.asarray(ind, dtype=np.int64)
    keep = np.asarray(dist).astype(np.float64) <= t
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    new_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(indptr) - 1))]).astype(np.int64)
    return new_ptr, ind[keep]


def cut(indptr, ind, dist, n_t, t):
    """What a cut at t must equal: CR.components of the restricted CSR -> (source_label, target_label, n_source_in, n_target_in, C)."""
    return CR.components(*restrict(indptr, ind, dist, t), n_t)


def thresholds(value, limit=18):
    """The distinct forest values (-0.0 and +0.0 are one); more than `limit`: 16 evenly spaced ones plus the two ends."""
    d = np.unique(np.asarray(value, dtype=np.float64))
    if d.size <= limit:
        return d
    return d[np.unique(np.round(np.linspace(0, d.size - 1, 18)).astype(np.int64))]   # (the two ends and 16 between them)


# ---- the weighted pair lists (each -> indptr, ind, dist, n_t) ------------------------------------------------------------------------
def random_ties(seed=11, n_q=300, n_t=280, per_row=3, dtype=np.float64, positive=False):
    """About `per_row` entries a row, weights in eighths: ties everywhere, and duplicate pairs with different values."""
    rng = np.random.default_rng(seed)
    n = n_q * per_row
    rows, cols = rng.integers(0, n_q, n), rng.integers(0, n_t, n)
    dup = rng.integers(0, n, n // 10)   # a tenth of the pairs once more, with a value of their own
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    w = rng.integers(1 if positive else 0, 17, rows.shape[0]) / 8.0
    order = np.argsort(rows, kind="stable")
    indptr, ind = CR.csr_of(rows, cols, n_q)
    return indptr, ind, w[order].astype(dtype), n_t


def all_equal():
    """Every weight the same: every pick is decided by the position, mutual picks are everywhere."""
    indptr, ind, w, n_t = random_ties(12)
    return indptr, ind, np.full_like(w, 0.5), n_t


def weighted_path(seed, increasing):
    """A shuffled path of 4 000 nodes; weights increasing along the path (every node picks the edge towards the start: one round
    hooks a chain of 4 000) or random."""
    rng = np.random.default_rng(seed)
    half = 2000
    s, t = rng.permutation(half), rng.permutation(half)
    rows, cols = np.concatenate([s, s[1:]]), np.concatenate([t, t[:-1]])   # s_i - t_i (step 2 i), t_i - s_(i+1) (step 2 i + 1)
    step = np.concatenate([2 * np.arange(half), 2 * np.arange(half - 1) + 1]).astype(np.float64)
    w = step if increasing else rng.random(rows.shape[0])
    order = rng.permutation(rows.shape[0])
    rows, cols, w = rows[order], cols[order], w[order]
    indptr, ind = CR.csr_of(rows, cols, half)
    return indptr, ind, w[np.argsort(rows, kind="stable")], half


def hubs():
    indptr, ind, n_t = CR.hub()
    return indptr, ind, np.random.default_rng(13).integers(0, 40, ind.shape[0]) / 4.0, n_t


def mixed_values():
    """Negative values, -inf, +inf, -0.0 and +0.0; NaN values, -1, INT_MAX and ids >= n_t among the entries; row 3 has no entry and
    target 9 nobody lists."""
    rng = np.random.default_rng(14)
    n_q, n_t, n = 40, 30, 240
    rows = rng.integers(0, n_q, n)
    rows[rows == 3] = 4
    cols = rng.integers(0, n_t, n)
    cols[cols == 9] = 10
    w = rng.choice(np.array([-np.inf, -2.5, -1.0, -0.0, 0.0, 0.75, 3.0, np.inf, np.nan]), n)
    bad = rng.random(n) < 0.15
    cols = np.where(bad, rng.choice(np.array([-1, INT_MAX, n_t, n_t + 5, 2 ** 40]), n), cols)
    order = np.argsort(rows, kind="stable")
    indptr, ind = CR.csr_of(rows, cols, n_q)
    return indptr, ind, w[order], n_t


def degenerate():
    z, f = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
    return {
        "n_q = 0": (np.zeros(1, dtype=np.int64), z, f, 6),
        "nnz = 0": (np.zeros(6, dtype=np.int64), z, f, 4),
        "one entry": (np.array([0, 0, 1], dtype=np.int64), np.array([2], dtype=np.int64), np.array([-1.5]), 3),
        "one entry, NaN": (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([np.nan]), 1),
    }


def fixed_lists(k):
    """[300, k] lists with padding (CR.fixed_lists) and weights in quarters -> (dist, ind, n_t)."""
    ind, n_t = CR.fixed_lists(k)
    return np.random.default_rng(15 + k).integers(-4, 9, ind.shape) / 4.0, ind, n_t


def csr_cases():
    """name -> (indptr, ind, dist, n_t): every small CSR the GPU tests run."""
    out = {"random ties": random_ties(), "random ties f32": random_ties(dtype=np.float32), "all equal": all_equal(),
           "path increasing": weighted_path(16, True), "path random": weighted_path(17, False), "hubs": hubs(), "mixed values": mixed_values()}
    out.update(degenerate())
    return out
