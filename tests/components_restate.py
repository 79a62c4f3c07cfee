"""numpy restatement of kz_components_csr / kz_components_lists and the graphs its tests share.

The connected components of the bipartite graph of a pair list: source row i is node i, target row j node n_q + j, every entry
(i, ind[p]) with 0 <= ind[p] < n_t an edge.  A SEQUENTIAL min-root union-find (the smaller root becomes the parent), then the rank of
the roots: components numbered in the order of their smallest node.  tests/test_components.py checks it against scipy's
connected_components on every graph below; tests/test_gpu_components.py checks the device against it bit for bit."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def _edges(indptr, ind, n_t):
    indptr, ind = np.asarray(indptr, dtype=np.int64), np.asarray(ind, dtype=np.int64)
    rows = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    ok = (ind >= 0) & (ind < n_t)
    return rows[ok], ind[ok]


def components(indptr, ind, n_t):
    """-> (source_label [n_q], target_label [n_t], n_source_in [C], n_target_in [C], C), all int64."""
    n_q = len(indptr) - 1
    n = n_q + n_t
    rows, cols = _edges(indptr, ind, n_t)
    parent = np.arange(n).tolist()

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in zip(rows.tolist(), (cols + n_q).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.arange(n, dtype=np.int64)
    touched = np.unique(np.concatenate([rows, cols + n_q]))   # (every other node is its own root)
    root[touched] = [find(v) for v in touched.tolist()]
    is_root = (root == np.arange(n)).astype(np.int64)
    rank = np.cumsum(is_root) - is_root
    label = rank[root]
    c = int(is_root.sum())
    return (label[:n_q], label[n_q:], np.bincount(label[:n_q], minlength=c).astype(np.int64),
            np.bincount(label[n_q:], minlength=c).astype(np.int64), c)


def components_lists(ind, n_t):
    ind = np.asarray(ind, dtype=np.int64)
    return components(ind.shape[1] * np.arange(ind.shape[0] + 1, dtype=np.int64), ind.reshape(-1), n_t)


def scipy_components(indptr, ind, n_t):
    """scipy.sparse.csgraph.connected_components on A = [[0, B], [B.T, 0]] -> (C, labels [n_q + n_t])."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n_q = len(indptr) - 1
    rows, cols = _edges(indptr, ind, n_t)
    B = sp.coo_matrix((np.ones(rows.shape[0], dtype=np.int8), (rows, cols)), shape=(n_q, n_t)).tocsr()
    A = sp.bmat([[None, B], [B.T, None]], format="csr") if n_q else sp.csr_matrix((n_t, n_t), dtype=np.int8)
    return connected_components(A, directed=False)


def csr_of(rows, cols, n_q):
    """The CSR of the pairs (rows[p], cols[p]), the entries of a row in the order they come in."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_q))]).astype(np.int64)
    return indptr, cols[order]


def component_sizes(indptr, ind, n_t):
    """The number of nodes of every component."""
    _, _, ns, nt, _ = components(indptr, ind, n_t)
    return ns + nt


# ---- the graphs (each -> indptr, ind, n_t) ----------------------------------------------------------------------------------------
def random_graph(seed, n_q, n_t, n_entries):
    rng = np.random.default_rng(seed)
    return csr_of(rng.integers(0, n_q, n_entries), rng.integers(0, n_t, n_entries), n_q) + (n_t,)


def mixed():
    """Near the threshold of the random graph: one large component, many small ones, many singletons."""
    return random_graph(0, 3000, 2500, 2800)


def near_giant():
    return random_graph(1, 2000, 2000, 3999)


def hub():
    """5000 rows list one of 7 targets each (about 700 listers per target: heavy contention on a few roots), and one more row lists
    5000 entries: longer than any fixed-width list."""
    rng = np.random.default_rng(2)
    rows = np.concatenate([np.arange(5000), np.full(5000, 5000)])
    cols = np.concatenate([rng.integers(0, 7, 5000), rng.integers(0, 7, 5000)])
    return csr_of(rows, cols, 5001) + (7,)


def chains(seed, n_chains, nodes_per_chain):
    """n_chains paths s - t - s - t - ... of nodes_per_chain nodes (even), source ids and target ids shuffled independently, the
    entries in random order."""
    rng = np.random.default_rng(seed)
    half = nodes_per_chain // 2
    n = n_chains * half
    perm_s, perm_t = rng.permutation(n), rng.permutation(n)
    rows, cols = [], []
    for c in range(n_chains):
        s, t = perm_s[c * half:(c + 1) * half], perm_t[c * half:(c + 1) * half]
        rows += [s, s[1:]]          # s_i - t_i, then t_i - s_(i+1)
        cols += [t, t[:-1]]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = rng.permutation(rows.shape[0])
    return csr_of(rows[order], cols[order], n) + (n,)


def path(seed):
    return chains(seed, 1, 4000)


def many_chains():
    return chains(5, 100, 40)


def degenerate():
    """name -> (indptr, ind, n_t)"""
    z = np.zeros(0, dtype=np.int64)
    return {
        "nnz = 0": (np.zeros(6, dtype=np.int64), z, 4),
        "n_q = 0": (np.zeros(1, dtype=np.int64), z, 6),
        "1 x 1 with the edge": (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64), 1),
        "1 x 1 without": (np.array([0, 0], dtype=np.int64), z, 1),
        "every entry out of range": (np.array([0, 2, 2, 5], dtype=np.int64), np.array([-1, 3, INT_MAX, -7, 2 ** 40], dtype=np.int64), 3),
        "duplicates": (np.array([0, 3, 5, 6], dtype=np.int64), np.array([1, 1, 0, 0, 0, 2], dtype=np.int64), 4),
    }


def fixed_lists(k, n_q=300, n_t=200, seed=7):
    """[n_q, k] lists with -1 and n_t as padding: about one valid entry per row (k = 1: in 7 rows of 10)."""
    rng = np.random.default_rng(seed + k)
    ind = rng.integers(0, n_t, (n_q, k))
    keep = rng.random((n_q, k)) < min(0.7, 1.0 / k)
    pad = np.where(rng.random((n_q, k)) < 0.5, -1, n_t)
    return np.where(keep, ind, pad).astype(np.int64), n_t


def all_graphs():
    """name -> (indptr, ind, n_t): every CSR the GPU tests run."""
    out = {"mixed": mixed(), "near giant": near_giant(), "hub": hub(), "path a": path(3), "path b": path(4), "many chains": many_chains()}
    out.update(degenerate())
    for k in (1, 3, 64):
        ind, n_t = fixed_lists(k)
        out[f"lists k={k}"] = (k * np.arange(ind.shape[0] + 1, dtype=np.int64), ind.reshape(-1), n_t)
    return out
