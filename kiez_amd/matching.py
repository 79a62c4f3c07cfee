"""One-to-one alignment: the source-proposing stable matching over neighbour lists, on the device (`kz_match_lists`).

Every neighbour list lets many source rows claim one target row.  Entity alignment is a matching task -- a target entity belongs
to at most one source entity -- and the CSLS-style pipelines end with a one-to-one step.  `one_to_one` is that step for any lists
this library (or anything else) produced; `Kiez.match` runs it on the lists of a fitted instance without taking them out of HBM."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native as N


def _checked_lists(dist, ind, n_target):
    """The argument checks of `one_to_one`, all before the device is touched -> (dist, ind) as the native call takes them."""
    if isinstance(n_target, (bool, np.bool_)) or not isinstance(n_target, (int, np.integer)) or n_target < 1:
        raise ValueError(f"n_target must be a positive integer, got {n_target!r}")
    if not isinstance(dist, N.DeviceArray):
        dist = np.asarray(dist)
    if not isinstance(ind, N.DeviceArray):
        ind = np.asarray(ind)
    if len(dist.shape) != 2 or len(ind.shape) != 2 or tuple(dist.shape) != tuple(ind.shape):
        raise ValueError(f"dist and ind must be 2-D neighbour lists of one shape, got {tuple(dist.shape)} and {tuple(ind.shape)}")
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
    `dist` is a `DeviceArray`, so are the results.  `evaluate.hits(match_ind[:, None], gold, k=[1])` is the matching's precision."""
    dist, ind = _checked_lists(dist, ind, n_target)
    on_device = isinstance(dist, N.DeviceArray)
    if ctx is None:
        ctx = dist.ctx if on_device else ind.ctx if isinstance(ind, N.DeviceArray) else N.Context.get()
    dist_dev, ind_dev = ctx.as_device(dist), ctx.as_device(ind)
    match, col, _ = N.match_lists(ctx, dist_dev, ind_dev, int(n_target))
    if not return_distance:
        return match if on_device else match.numpy()
    match_dist = N.match_values(ctx, dist_dev, col)
    return (match_dist, match) if on_device else (match_dist.numpy(), match.numpy())
