"""One-to-one alignment over neighbour lists, on the device: the source-proposing stable matching (`kz_match_lists`) and the
minimum-cost assignment (`kz_assign_lists`).

Every neighbour list lets many source rows claim one target row.  Entity alignment is a matching task -- a target entity belongs
to at most one source entity -- and the CSLS-style pipelines end with a one-to-one step.  `one_to_one` is that step for any lists
this library (or anything else) produced, `assignment` the same step with the total value of the pairs minimised instead of pairs
taken greedily; `Kiez.match` runs either on the lists of a fitted instance without taking them out of HBM.  `sinkhorn_lists` is the soft form over the
same lists: the Sinkhorn potentials with the transport plan restricted to the listed pairs (`kz_sinkhorn_lists`)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native as N


def _checked_dtypes(dist, ind):
    """The dtype half of `_checked`, shared by the two layouts."""
    if not np.issubdtype(ind.dtype, np.integer):
        raise ValueError(f"ind must hold integer row ids, got {ind.dtype}")
    if not np.issubdtype(dist.dtype, np.floating):
        raise ValueError(f"dist must be floating point, got {dist.dtype}")
    if isinstance(dist, N.DeviceArray):
        if dist.dtype not in (np.float32, np.float64):
            raise ValueError(f"a device dist must be float32 or float64, got {dist.dtype}")
    elif dist.dtype not in (np.float32, np.float64):
        dist = dist.astype(np.float64)   # (float16, longdouble: matched and returned as float64)
    if isinstance(ind, N.DeviceArray):
        if ind.dtype != np.int64:
            raise ValueError(f"a device ind must be int64, got {ind.dtype}")
    elif ind.dtype != np.int64:
        if ind.dtype == np.uint64 and ind.size and ind.max() > np.iinfo(np.int64).max:
            raise ValueError("ind holds ids beyond int64")
        ind = ind.astype(np.int64)
    return dist, ind


def _checked(dist, ind, indptr, n_target):
    """The argument checks of every function here that takes a pair list, all before the device is touched -> (dist, ind, indptr) as
    `_uploaded` takes them.  `indptr` None: fixed-width lists [n_q, k]; else a CSR, whose host `indptr` is checked in full here (one
    on the device is checked there, by the native call).  `dist` None (`components`: a list without values): the same checks of the
    rest, and None comes back for it."""
    if isinstance(n_target, (bool, np.bool_)) or not isinstance(n_target, (int, np.integer)) or n_target < 1:
        raise ValueError(f"n_target must be a positive integer, got {n_target!r}")
    dist, ind, indptr = (a if a is None or isinstance(a, N.DeviceArray) else np.asarray(a) for a in (dist, ind, indptr))
    if indptr is None:
        if dist is None:
            return None, _checked_ids("ind", ind), None
        if len(dist.shape) != 2 or len(ind.shape) != 2 or tuple(dist.shape) != tuple(ind.shape):
            raise ValueError(f"dist and ind must be 2-D neighbour lists of one shape, got {tuple(dist.shape)} and {tuple(ind.shape)}")
        return _checked_dtypes(dist, ind) + (None,)
    if dist is None:
        if len(ind.shape) != 1:
            raise ValueError(f"ind must be a 1-D array (the entries of a CSR), got shape {tuple(ind.shape)}")
    elif len(dist.shape) != 1 or len(ind.shape) != 1 or tuple(dist.shape) != tuple(ind.shape):
        raise ValueError(f"dist and ind must be 1-D arrays of one length (the entries of a CSR), got {tuple(dist.shape)} "
                         f"and {tuple(ind.shape)}")
    if len(indptr.shape) != 1 or indptr.shape[0] < 1:
        raise ValueError(f"indptr must be a 1-D array of n_source + 1 row starts, got shape {tuple(indptr.shape)}")
    if not np.issubdtype(indptr.dtype, np.integer) or indptr.dtype == np.bool_:
        raise ValueError(f"indptr must hold integer row starts, got {indptr.dtype}")
    if dist is None:
        ind = _checked_ids("ind", ind, ndim=1)
    else:
        dist, ind = _checked_dtypes(dist, ind)
    if isinstance(indptr, N.DeviceArray):
        if indptr.dtype != np.int64:
            raise ValueError(f"a device indptr must be int64, got {indptr.dtype}")
    else:
        nnz = ind.shape[0]
        if indptr[0] != 0 or indptr[-1] != nnz or (indptr.shape[0] > 1 and bool((indptr[1:] < indptr[:-1]).any())):
            raise ValueError(f"indptr must start at 0, never decrease and end at the number of entries {nnz}, got {indptr[0]} .. {indptr[-1]}")
        indptr = indptr.astype(np.int64, copy=False)
    return dist, ind, indptr


def _uploaded(checked, n_target, ctx):
    """(dist | None, ind, indptr | None) as `_checked` returns them -> (the `PairList` on the device -- the one object that knows the
    layout from here on --, whether the results stay on the device: they do if `dist`, or `ind` where there is no `dist`, is a
    `DeviceArray`)."""
    on_device = isinstance(checked[1] if checked[0] is None else checked[0], N.DeviceArray)
    if ctx is None:
        ctx = next((a.ctx for a in checked if isinstance(a, N.DeviceArray)), None) or N.Context.get()
    dist, ind, indptr = (None if a is None else ctx.as_device(a) for a in checked)
    if indptr is None:
        return N.PairList.lists(ctx, dist, ind, int(n_target)), on_device
    return N.PairList.csr(ctx, indptr, ind, dist, int(n_target)), on_device


def from_sparse(S):
    """A scipy sparse matrix [n_source, n_target] whose STORED entries are the pairs (an explicit zero is a pair of value 0) ->
    `(indptr, ind, dist)`, the CSR `one_to_one_csr`, `assignment_csr` and `sinkhorn_csr` take: every row sorted by
    (value, target row), the order every list of this library has.  scipy orders a row by column id, and `one_to_one` reads a row's
    order as the source's preference.  Host-side: one lexsort over the entries.  Duplicate entries are summed first, as scipy does."""
    if not hasattr(S, "tocsr"):
        raise ValueError(f"from_sparse takes a scipy sparse matrix, got {type(S).__name__}")
    S = S.tocsr(copy=True)
    S.sum_duplicates()
    indptr = np.asarray(S.indptr, dtype=np.int64)
    ind = np.asarray(S.indices, dtype=np.int64)
    dist = np.asarray(S.data)
    if not np.issubdtype(dist.dtype, np.floating) or dist.dtype not in (np.float32, np.float64):
        dist = dist.astype(np.float64)
    rows = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((ind, dist, rows))   # (row, then value, then target row; NaN values sort last in their row)
    return indptr, ind[order], dist[order]


def one_to_one(dist, ind, n_target: int, *, return_distance: bool = True, ctx: Optional[N.Context] = None):
    """The one-to-one assignment of source rows to target rows from neighbour lists: the source-proposing stable matching.

    `dist`, `ind` [n_q, k]: neighbour lists as `kneighbors` / `kneighbors_whole_index` return them (numpy arrays, or the
    `DeviceArray`s of `kneighbors_device` / `kneighbors_whole_index_device`); `n_target`: the number of target rows.  An entry with
    `ind` outside [0, n_target) is no pair.  A source row prefers its pairs by column; a target row prefers the sources that list it
    by (value, source row), smaller first, with NaN counted as +inf and -0.0 equal to +0.0.  The matching is the unique
    source-optimal stable one; for lists sorted by value -- every list this library returns -- it is the greedy assignment over all
    pairs in the order (value, source row, column), a pair being taken when both its ends are still free.

    Returns `(match_dist, match_ind)`, each [n_q], or `match_ind` alone with `return_distance=False`: `match_ind[i]` is the target
    row of source row i or -1, `match_dist[i]` the value of that pair in `dist`'s dtype or NaN.  numpy lists give numpy arrays; if
    `dist` is a `DeviceArray`, so are the results.  `evaluate.hits(match_ind[:, None], gold, k=[1])` is the matching's precision.
    Ragged lists (a CSR): `one_to_one_csr`."""
    return _one_to_one(dist, ind, None, n_target, return_distance, ctx)


def _one_to_one(dist, ind, indptr, n_target, return_distance, ctx):
    pairs, on_device = _uploaded(_checked(dist, ind, indptr, n_target), n_target, ctx)
    match, col, _ = pairs.match()
    if not return_distance:
        return match if on_device else match.numpy()
    match_dist = pairs.values(col)
    return (match_dist, match) if on_device else (match_dist.numpy(), match.numpy())


def _assignment_options(unmatched_cost, eps, max_rounds):
    """The checks of `assignment`'s options that need no data -> (unmatched_cost | None, eps | None, max_rounds)."""
    def real(name, x):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a real number, got {x!r}")
        return float(x)
    if unmatched_cost is not None:
        unmatched_cost = real("unmatched_cost", unmatched_cost)
        if not np.isfinite(unmatched_cost):
            raise ValueError(f"unmatched_cost must be finite, got {unmatched_cost!r}")
    if eps is not None:
        eps = real("eps", eps)
        if not (np.isfinite(eps) and eps > 0.0):
            raise ValueError(f"eps must be positive and finite, got {eps!r}")
    if isinstance(max_rounds, (bool, np.bool_)) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1:
        raise ValueError(f"max_rounds must be a positive integer, got {max_rounds!r}")
    return unmatched_cost, eps, int(max_rounds)


def _host_value_range(dist, ind, n_target):
    """What kz_assign_range returns, for lists on the host: (smallest, largest) finite value listed with 0 <= ind < n_target, as
    float64, or None."""
    w = dist.astype(np.float64)[(ind >= 0) & (ind < n_target)]
    w = w[np.isfinite(w)]
    return (float(w.min()), float(w.max())) if w.size else None


def _assignment_defaults(value_range, n_q, unmatched_cost, eps):
    """`unmatched_cost` and `eps` with their defaults filled in from the range of the listed values; the lower bound of eps."""
    lo, hi = value_range if value_range is not None else (0.0, 0.0)
    scale = hi - lo if hi > lo and np.isfinite(hi - lo) else 1.0
    if unmatched_cost is None:
        unmatched_cost = hi
    if eps is None:
        eps = scale / (1000.0 * max(n_q, 1))
    if eps < scale * 2.0 ** -40:
        raise ValueError(f"eps = {eps!r} is below 2**-40 of the lists' value spread {scale!r}: a bid may fail to raise a price")
    return unmatched_cost, eps


def _assignment_of(pairs, unmatched_cost, eps, max_rounds=1_000_000, return_distance=True, return_prices=False, defaults=True):
    """The auction over a `PairList` -> the tuple ([match_dist,] match_ind[, prices]) of `DeviceArray`s.  `defaults`: unmatched_cost
    and eps are completed and checked here, from the value range taken on the device (False: the caller did, from lists on the host)."""
    if defaults:
        unmatched_cost, eps = _assignment_defaults(pairs.value_range(), pairs.n_q, unmatched_cost, eps)
    match, col, prices, rounds, converged = pairs.assign(unmatched_cost, eps, max_rounds, want_prices=return_prices)
    if not converged:
        raise RuntimeError(f"assignment: rows are still free after {rounds} rounds (max_rounds) with eps = {eps!r} and "
                           f"unmatched_cost = {unmatched_cost!r}; a larger eps or a smaller unmatched_cost shortens the run")
    out = (pairs.values(col), match) if return_distance else (match,)
    return out + (prices,) if return_prices else out


def _assignment(dist, ind, indptr, n_target, unmatched_cost, eps, max_rounds, return_distance, return_prices, ctx):
    dist, ind, indptr = _checked(dist, ind, indptr, n_target)
    unmatched_cost, eps, max_rounds = _assignment_options(unmatched_cost, eps, max_rounds)
    host = not isinstance(dist, N.DeviceArray) and not isinstance(ind, N.DeviceArray)
    if host:   # (host lists: the eps check comes before the device is touched)
        n_q = dist.shape[0] if indptr is None else indptr.shape[0] - 1
        unmatched_cost, eps = _assignment_defaults(_host_value_range(dist, ind, n_target), n_q, unmatched_cost, eps)
    pairs, on_device = _uploaded((dist, ind, indptr), n_target, ctx)
    out = _assignment_of(pairs, unmatched_cost, eps, max_rounds, return_distance, return_prices, defaults=not host)
    if not on_device:
        out = tuple(x.numpy() for x in out)
    return out if len(out) > 1 else out[0]


def assignment(dist, ind, n_target: int, *, unmatched_cost: Optional[float] = None, eps: Optional[float] = None,
               max_rounds: int = 1_000_000, return_distance: bool = True, return_prices: bool = False, ctx: Optional[N.Context] = None):
    """The minimum-cost one-to-one assignment of source rows to target rows from neighbour lists, on the device (`kz_assign_lists`):
    the hard form of what `Sinkhorn` computes softly, where `one_to_one` takes pairs greedily.

    `dist`, `ind`, `n_target` as `one_to_one` takes them.  An entry is a pair when `ind` is in [0, n_target), the value widened
    to float64 is finite, and it is at most `unmatched_cost`.  A matching uses each source and each target row at most once; its
    cost is the sum of the matched pairs' values plus `unmatched_cost` for every unmatched source row, so a row is matched only
    where that is strictly better than staying out.  `unmatched_cost` defaults to the largest finite listed value.  The result
    costs at most `n_q * eps` more than the optimum; `eps` defaults to a thousandth of the lists' value spread divided by n_q,
    and for integer values `eps < 1 / (n_q + 1)` gives the exact optimum.  Values may be negative; all arithmetic is float64.
    The solver is a forward auction with synchronous rounds: every run returns the same arrays.

    Returns `(match_dist, match_ind)`, or `match_ind` alone with `return_distance=False`, as `one_to_one` does, with the float64
    target prices [n_target] appended when `return_prices=True`.  More than `max_rounds` rounds raise RuntimeError.
    Ragged lists (a CSR): `assignment_csr`."""
    return _assignment(dist, ind, None, n_target, unmatched_cost, eps, max_rounds, return_distance, return_prices, ctx)


def _sinkhorn_options(temperature, n_iter, tol):
    """The checks of the Sinkhorn options that need no data."""
    if (isinstance(temperature, (bool, np.bool_)) or not isinstance(temperature, (int, float, np.integer, np.floating))
            or not np.isfinite(temperature) or temperature <= 0):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if isinstance(n_iter, (bool, np.bool_)) or not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ValueError(f"n_iter must be an integer >= 1, got {n_iter!r}")
    if tol is not None and (isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0):
        raise ValueError(f"tol must be None or a number >= 0, got {tol!r}")


def sinkhorn_lists(dist, ind, n_target: int, *, temperature: float = 0.05, n_iter: int = 10, tol: Optional[float] = None,
                   ctx: Optional[N.Context] = None, return_info: bool = False):
    """The Sinkhorn potentials of neighbour lists, on the device (`kz_sinkhorn_lists`): entropic optimal transport between the source
    rows and `n_target` target rows with the plan restricted to the LISTED pairs -- what `Sinkhorn(support="candidates")` fits, for
    any caller's lists.

    `dist`, `ind`, `n_target` as `one_to_one` takes them (numpy arrays or `DeviceArray`s; an entry with `ind` outside [0, n_target)
    is no pair, so the padded lists of `kneighbors_whole_index` are fine); values are taken as float64.  From f = 0, `n_iter` times:
    g_j = softmin_eps over the rows i that list j of (d_ij - f_i) + eps log(n_q / n_target), then f_i = softmin_eps over the pairs of
    row i of (d_ij - g_j), softmin_eps(x) = m - eps log sum exp(-(x - m) / eps), m = min x; `temperature` is eps, in the units of
    `dist`.  `tol`: stop after the column step that moves g by at most tol (None: exactly `n_iter` iterations).  The pairs outside
    the lists are dropped, so the potentials depend on how long the lists are.  A target row that no row lists, and a row without a
    pair, get NaN.  Every run returns the same bits.

    Returns `(f, g)`, float64 [n_q] and [n_target] -- numpy arrays for numpy lists, `DeviceArray`s if `dist` is one -- and with
    `return_info=True` a third item, the dict {"n_iter": iterations done, "potential_change": the last measured change of g or None}.
    `(dist - f[:, None]) - g[ind]` is the reduced distance of the listed pairs (`Sinkhorn.transform`).  Ragged lists (a CSR):
    `sinkhorn_csr`."""
    return _sinkhorn(dist, ind, None, n_target, temperature, n_iter, tol, ctx, return_info)


def _sinkhorn(dist, ind, indptr, n_target, temperature, n_iter, tol, ctx, return_info):
    dist, ind, indptr = _checked(dist, ind, indptr, n_target)
    _sinkhorn_options(temperature, n_iter, tol)
    if not isinstance(dist, N.DeviceArray):
        dist = dist.astype(np.float64, copy=False)
    elif dist.dtype != np.float64:
        raise ValueError(f"a device dist must be float64 here, got {dist.dtype}")
    pairs, on_device = _uploaded((dist, ind, indptr), n_target, ctx)
    f, g, done, change = pairs.sinkhorn(float(temperature), int(n_iter), tol)
    out = (f, g) if on_device else (f.numpy(), g.numpy())
    return out + ({"n_iter": done, "potential_change": change},) if return_info else out


# ---- the same three steps on RAGGED lists: a CSR (indptr, ind, dist) as `radius_neighbors` or `from_sparse` return it ----------------
def one_to_one_csr(indptr, ind, dist, n_target: int, *, return_distance: bool = True, ctx: Optional[N.Context] = None):
    """`one_to_one` over ragged lists (kz_match_csr).  `indptr` [n_q + 1], `ind` and `dist` 1-D arrays of one length: row i lists the
    targets `ind[indptr[i]:indptr[i + 1]]` with the values `dist[...]`, in its order of preference (`radius_neighbors` and
    `from_sparse` order a row by (value, target row)).  Rows may be empty and have NO length limit (`one_to_one` stops at 4 096
    columns); an entry with `ind` outside [0, n_target) is no pair, a target may repeat inside a row.  numpy arrays or `DeviceArray`s,
    with `one_to_one`'s rule for where the result lives.  An `indptr` that does not start at 0, decreases or does not end at the
    number of entries raises ValueError -- a host one before the device is touched, a device one on the device before anything
    reads through it.  Returns what `one_to_one` returns."""
    return _one_to_one(dist, ind, indptr, n_target, return_distance, ctx)


def assignment_csr(indptr, ind, dist, n_target: int, *, unmatched_cost: Optional[float] = None, eps: Optional[float] = None,
                   max_rounds: int = 1_000_000, return_distance: bool = True, return_prices: bool = False,
                   ctx: Optional[N.Context] = None):
    """`assignment` over ragged lists (kz_assign_csr): the CSR as `one_to_one_csr` takes it, every option, default (from the range
    of the listed values), error and result as `assignment`."""
    return _assignment(dist, ind, indptr, n_target, unmatched_cost, eps, max_rounds, return_distance, return_prices, ctx)


def sinkhorn_csr(indptr, ind, dist, n_target: int, *, temperature: float = 0.05, n_iter: int = 10, tol: Optional[float] = None,
                 ctx: Optional[N.Context] = None, return_info: bool = False):
    """`sinkhorn_lists` over ragged lists (kz_sinkhorn_csr): the CSR as `one_to_one_csr` takes it (values taken as float64), every
    option and result as `sinkhorn_lists`; f has one entry per row of `indptr`."""
    return _sinkhorn(dist, ind, indptr, n_target, temperature, n_iter, tol, ctx, return_info)


# ---- the producer of such a CSR from two list arrays: forward, reverse, union, mutual --------------------------------------------
def _checked_ids(what, ind, ndim=2):
    """One list array of `combine_lists` or `components` -> a 2-D int64 array (numpy or `DeviceArray`), before the device is touched.
    (`ndim` 1: the entries of a CSR, whose shape `_checked` has checked.)"""
    if not isinstance(ind, N.DeviceArray):
        ind = np.asarray(ind)
    if ndim == 2 and (len(ind.shape) != 2 or ind.shape[1] < 1):
        raise ValueError(f"{what} must be a 2-D array of ids with at least one column, got shape {tuple(ind.shape)}")
    if not np.issubdtype(ind.dtype, np.integer) or ind.dtype == np.bool_:
        raise ValueError(f"{what} must hold integer row ids, got {ind.dtype}")
    if isinstance(ind, N.DeviceArray):
        if ind.dtype != np.int64:
            raise ValueError(f"a device {what} must be int64, got {ind.dtype}")
    elif ind.dtype != np.int64:
        if ind.dtype == np.uint64 and ind.size and ind.max() > np.iinfo(np.int64).max:
            raise ValueError(f"{what} holds ids beyond int64")
        ind = ind.astype(np.int64)
    return ind


def combine_lists(fwd_ind, rev_ind, *, mode: str, n_source: Optional[int] = None, n_target: Optional[int] = None,
                  ctx: Optional[N.Context] = None):
    """The set combination of a forward and a reverse list array into a CSR over the source rows (kz_lists_combine), for lists from
    anywhere.  `fwd_ind` [n_source, k_f]: target ids per source row; `rev_ind` [n_target, k_r]: source ids per target row; k_f != k_r
    is fine.  With F = {(i, fwd_ind[i, c])} and R = {(rev_ind[j, c], j)}, `mode` "forward" gives F, "reverse" R grouped by source row
    (the transposed reverse lists), "union" F | R and "mutual" F & R -- every pair once.  An id outside its range is no pair,
    `one_to_one`'s rule: -1, the INT_MAX padding of `kneighbors_whole_index`, an id >= n.  An id repeated inside a row counts once.
    "forward" ignores `rev_ind` and "reverse" `fwd_ind` (None is fine); `n_source` / `n_target` default to the row counts of the arrays
    and must be named where the one array read does not say them.

    Returns `(indptr int64 [n_source + 1], ind int64 [total])`: the targets of source row i are `ind[indptr[i]:indptr[i + 1]]`,
    ascending by target id.  numpy arrays give numpy arrays; if the array read first is a `DeviceArray`, so are the results.  The
    same bytes from every call.  Values for the pairs: `Kiez.neighbor_pairs` computes them for a fitted instance."""
    mode = N.pair_mode(mode, "combine_lists")
    use_f, use_r = mode != "reverse", mode != "forward"
    fwd = _checked_ids("fwd_ind", fwd_ind) if use_f else None
    rev = _checked_ids("rev_ind", rev_ind) if use_r else None
    for what, n in (("n_source", n_source), ("n_target", n_target)):
        if n is not None and (isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < (what == "n_target")):
            raise ValueError(f"{what} must be a {'positive' if what == 'n_target' else 'non-negative'} integer, got {n!r}")
    # (the array a one-sided mode does not read still says how many rows its side has, where it is given)
    if n_source is None and (use_f or fwd_ind is not None):
        n_source = fwd.shape[0] if use_f else _checked_ids("fwd_ind", fwd_ind).shape[0]
    if n_target is None and (use_r or rev_ind is not None):
        n_target = rev.shape[0] if use_r else _checked_ids("rev_ind", rev_ind).shape[0]
    if n_source is None or n_target is None:
        raise ValueError(f"combine_lists(mode={mode!r}) reads one list array: name n_source and n_target")
    if (use_f and fwd.shape[0] != n_source) or (use_r and rev.shape[0] != n_target):
        raise ValueError(f"fwd_ind has one row per source row and rev_ind one per target row: got n_source = {n_source}, n_target = "
                         f"{n_target} and shapes {tuple(fwd.shape) if use_f else None}, {tuple(rev.shape) if use_r else None}")
    first = fwd if use_f else rev
    on_device = isinstance(first, N.DeviceArray)
    if ctx is None:
        ctx = next((a.ctx for a in (fwd, rev) if isinstance(a, N.DeviceArray)), None) or N.Context.get()
    indptr, ind, _ = N.lists_combine(ctx, ctx.as_device(fwd) if use_f else None, ctx.as_device(rev) if use_r else None, mode,
                                     int(n_source), int(n_target))
    return (indptr, ind) if on_device else (indptr.numpy(), ind.numpy())


# ---- the transitive closure of a pair list: entity clusters (kz_components_csr, kz_components_lists) ------------------------------
def _checked_node_count(n_source, n_target):
    if n_source + n_target > N.COMPONENTS_MAX_NODES:
        raise ValueError(f"n_source + n_target = {n_source + n_target} rows, the limit is {N.COMPONENTS_MAX_NODES} (2**31 - 2)")


def _components_of(pairs, return_sizes):
    """The labels (and sizes) of a `PairList`'s components -> a tuple of `DeviceArray`s."""
    res = pairs.components(bool(return_sizes))
    return tuple(res[:4] if return_sizes else res[:2])


def _components(ind, indptr, n_target, return_sizes, ctx):
    _, ind, indptr = _checked(None, ind, indptr, n_target)
    _checked_node_count(ind.shape[0] if indptr is None else indptr.shape[0] - 1, int(n_target))
    if indptr is None and ind.shape[0] * ind.shape[1] > 2 ** 31 - 2:
        raise ValueError(f"ind has {ind.shape[0] * ind.shape[1]} entries, the limit is 2**31 - 2")
    pairs, on_device = _uploaded((None, ind, indptr), n_target, ctx)
    out = _components_of(pairs, return_sizes)
    return out if on_device else tuple(x.numpy() for x in out)


def components_csr(indptr, ind, n_target: int, *, return_sizes: bool = False, ctx: Optional[N.Context] = None):
    """Entity clusters: the connected components of the bipartite graph of a pair list, on the device (kz_components_csr) -- the
    transitive closure "everything connected by accepted pairs is one entity", the third way to resolve a many-to-many pair list
    beside `one_to_one_csr` / `assignment_csr` and `sinkhorn_csr`.

    `indptr` [n_source + 1] and `ind`: a CSR as `one_to_one_csr` takes it, without values -- of `Kiez.radius_neighbors`,
    `Kiez.neighbor_pairs`, `from_sparse`, `combine_lists` or anything else; numpy arrays or `DeviceArray`s.  Source row i and target row
    j are joined by every entry `j = ind[p]` of row i with 0 <= j < n_target; any other entry is no pair, a pair may repeat.  EVERY
    row belongs to a cluster: a source row without a pair and a target row nobody lists are clusters of one row.  Clusters are numbered
    0 .. C - 1 in the order of their smallest node, source rows before target rows -- what
    `scipy.sparse.csgraph.connected_components([[0, B], [B.T, 0]], directed=False)` returns, bit for bit, from every run.

    Returns `(source_label int64 [n_source], target_label int64 [n_target])`; with `return_sizes=True` also
    `(n_source_in, n_target_in)`, int64 [C]: the source and target rows of every cluster.  `(n_source_in == 1) & (n_target_in == 1)`
    are the unambiguous alignments, a giant cluster says the threshold is too loose.  numpy arrays in give numpy arrays, if `ind` is a
    `DeviceArray` so are the results.  `evaluate.cluster_metrics` scores the pairs the clustering implies.  Argument errors are raised
    before the device is touched; an `indptr` on the device that does not start at 0, decreases or does not end at the number of
    entries raises ValueError there, before anything reads through it.  Fixed-width lists: `components`."""
    return _components(ind, indptr, n_target, return_sizes, ctx)


def components(ind, n_target: int, *, return_sizes: bool = False, ctx: Optional[N.Context] = None):
    """`components_csr` over fixed-width lists (kz_components_lists): `ind` [n_source, k] as `kneighbors` returns it, any k >= 1; an
    entry outside [0, n_target) -- a -1, the INT_MAX padding of `kneighbors_whole_index` -- is no pair.  Every result and error as
    `components_csr`."""
    return _components(ind, None, n_target, return_sizes, ctx)


# ---- the single-linkage hierarchy of a weighted pair list: clusters at every threshold (kz_forest_csr, kz_forest_lists) -----------
def _checked_threshold(t) -> float:
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
        raise ValueError(f"the threshold must be a real number, got {t!r}")
    t = float(t)
    if t != t:
        raise ValueError("the threshold must not be NaN (+inf and -inf are fine)")
    return t


class Hierarchy:
    """The single-linkage hierarchy of a weighted pair list: its minimum spanning forest, which holds the clusters of the pairs with
    value <= t for EVERY threshold t (`single_linkage_csr`, `single_linkage`, `Kiez.hierarchy_radius`, `Kiez.hierarchy_pairs`).

    `n_source`, `n_target`; `n_components`: the clusters of all pairs; `source`, `target` (int64), `value` (float64), `entry` (int64)
    [m], m = n_source + n_target - n_components: the forest's edges as numpy arrays, ascending by (value, `entry`) with -0.0 equal to
    +0.0 -- `entry` is the position of the edge in the pair list it came from (the CSR position, or i * k + c).  `rounds`: the rounds
    the device took (None for a hierarchy built from arrays).  The device copies of `source` / `target` are kept for the cuts."""

    def __init__(self, n_source, n_target, n_components, source, target, value, entry, *, rounds=None, device=None, ctx=None):
        self.n_source, self.n_target, self.n_components = int(n_source), int(n_target), int(n_components)
        self.source, self.target = np.asarray(source, dtype=np.int64), np.asarray(target, dtype=np.int64)
        self.value, self.entry = np.asarray(value, dtype=np.float64), np.asarray(entry, dtype=np.int64)
        m = self.value.shape[0]
        if not (self.source.shape == self.target.shape == self.entry.shape == self.value.shape == (m,)):
            raise ValueError("source, target, value and entry must be 1-D arrays of one length")
        if m != self.n_source + self.n_target - self.n_components:
            raise ValueError(f"a forest of {self.n_source + self.n_target} nodes and {self.n_components} components has "
                             f"{self.n_source + self.n_target - self.n_components} edges, got {m}")
        if m and (np.isnan(self.value).any() or bool((self.value[1:] < self.value[:-1]).any())):
            raise ValueError("value must be ascending and hold no NaN")
        self.rounds = rounds
        self._device, self._ctx = device, ctx   # (source, target) as DeviceArrays, uploaded by the first cut when not given

    def n_edges(self, t) -> int:
        """The forest edges with value <= t: the length of the prefix a cut at t uses."""
        return int(np.searchsorted(self.value, _checked_threshold(t), side="right"))

    def n_clusters(self, t) -> int:
        """The number of clusters of the pairs with value <= t: every forest edge joins two.  Host arithmetic."""
        return self.n_source + self.n_target - self.n_edges(t)

    def cut_device(self, t, return_sizes: bool = False):
        """Like `cut` but the label (and size) arrays stay in HBM as DeviceArrays."""
        count = self.n_edges(t)
        if self._device is None:
            ctx = self._ctx or N.Context.get()
            self._device, self._ctx = (ctx.to_device(self.source), ctx.to_device(self.target)), ctx
        source, target = self._device
        res = N.components_edges(source.ctx, source, target, self.n_source, self.n_target, bool(return_sizes), count=count)
        return tuple(res[:4] if return_sizes else res[:2])

    def cut(self, t, return_sizes: bool = False):
        """The clusters of the pairs with value <= t (IEEE comparison; t = +-inf is fine, NaN raises ValueError before the device is
        touched): what `components_csr` returns for the pair list restricted to those entries, bit for bit -- `(source_label,
        target_label)`, with `return_sizes=True` also `(n_source_in, n_target_in)` -- from a components call over the forest's prefix
        (kz_components_edges), at most n_source + n_target - 1 edges however many pairs the list held."""
        return tuple(x.numpy() for x in self.cut_device(t, return_sizes))


def _single_linkage(dist, ind, indptr, n_target, ctx):
    if dist is None:
        raise ValueError("single linkage needs the values of the pairs: dist is None")
    dist, ind, indptr = _checked(dist, ind, indptr, n_target)
    n_source = ind.shape[0] if indptr is None else indptr.shape[0] - 1
    _checked_node_count(n_source, int(n_target))
    if indptr is None and ind.shape[0] * ind.shape[1] > 2 ** 31 - 2:
        raise ValueError(f"ind has {ind.shape[0] * ind.shape[1]} entries, the limit is 2**31 - 2")
    pairs, _ = _uploaded((dist, ind, indptr), n_target, ctx)
    return _hierarchy_of(pairs)


def _hierarchy_of(pairs):
    """The forest of a `PairList` with values -> a `Hierarchy` (numpy copies for the host side, the device edges for the cuts)."""
    source, target, value, entry, n_components, rounds = pairs.forest()
    return Hierarchy(pairs.n_q, pairs.n_target, n_components, source.numpy(), target.numpy(), value.numpy(), entry.numpy(), rounds=rounds,
                     device=(source, target), ctx=pairs.ctx)


def single_linkage_csr(indptr, ind, dist, n_target: int, *, ctx: Optional[N.Context] = None) -> Hierarchy:
    """The single-linkage hierarchy of a weighted pair list, on the device (kz_forest_csr): ONE call that answers "which clusters do the
    pairs with value <= t form" for every t, where `components_csr` answers it for the one threshold the list was produced with.

    `indptr`, `ind`, `dist`: a CSR as `one_to_one_csr` takes it (numpy arrays or `DeviceArray`s; float32 or float64 values).  An entry
    is an edge when 0 <= ind < n_target and its value is not NaN; -inf, +inf, -0.0 and negative values are legal; a pair stored twice
    counts with its smaller value.  The result is the minimum spanning forest under the order (value, position of the entry), -0.0
    equal to +0.0: unique, the same bytes from every run.  Returns a `Hierarchy`; `Hierarchy.cut(t)` equals `components_csr` of the
    entries with value <= t bit for bit, `evaluate.cluster_curve` scores a sweep of thresholds against gold.  Argument errors are
    raised before the device is touched.  Fixed-width lists: `single_linkage`."""
    return _single_linkage(dist, ind, indptr, n_target, ctx)


def single_linkage(dist, ind, n_target: int, *, ctx: Optional[N.Context] = None) -> Hierarchy:
    """`single_linkage_csr` over fixed-width lists `dist`, `ind` [n_source, k] (kz_forest_lists), any k >= 1; `Hierarchy.entry` is
    i * k + c.  An entry outside [0, n_target) -- a -1, the INT_MAX padding of `kneighbors_whole_index` -- is no pair."""
    return _single_linkage(dist, ind, None, n_target, ctx)
