"""hits@k — `kiez.evaluate.hits` (kiez/evaluate/eval_metrics.py:23-61) with the row scan on the GPU.

For array input the neighbour matrix may live on the device (`Kiez.kneighbors_device`).  Dict input with arbitrary
labels is first encoded to integer ids on the host (data preparation); the matching itself runs in `kz_hit_positions`."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Union

import numpy as np

from . import _native as N

_NO_GOLD = np.iinfo(np.int64).min


def _as_row_number(x):
    """x as an integer if the reference's `==` would match it against an integer row number / neighbour id (ints, and floats with an
    integral value: 4.0 == 4 and hash(4.0) == hash(4), so `i in gold` and `gold[i] in nn_ind[i][:k]` both accept them), else None.
    Values that no int64 row number or neighbour id can equal -- beyond [-2**63, 2**63), e.g. 1e20 -- are None as well (the
    reference's `in` simply finds no hit for them; such pairs count in the denominator only).  bools stay what they are to
    Python's `==` and `hash`: True is 1 and False is 0 -- `1 in {True: t}` holds in the reference, too."""
    if isinstance(x, (bool, np.bool_)):
        return int(bool(x))
    if isinstance(x, (int, np.integer)):
        v = int(x)
    elif isinstance(x, (float, np.floating)) and np.isfinite(x) and float(x) == int(x):
        v = int(x)
    else:
        return None
    return v if -(1 << 63) <= v < (1 << 63) else None


def _gold_vector(gold: Dict[Any, Any], n_rows: int) -> np.ndarray:
    """gold target per source row (or _NO_GOLD): one vectorised scatter instead of a Python loop over all rows."""
    out = np.full(n_rows, _NO_GOLD, dtype=np.int64)
    # (array input: the reference tests `i in gold and gold[i] in nn_ind[i][:k]` with integer row numbers i, so only keys and
    #  targets that compare equal to an integer can ever hit -- ints and integral floats, e.g. gold read with np.loadtxt or from
    #  a pandas column; everything still counts in the denominator len(gold))
    pairs = [(a, b) for a, b in ((_as_row_number(k_), _as_row_number(v)) for k_, v in gold.items()) if a is not None and b is not None]
    if pairs:
        keys = np.fromiter((p[0] for p in pairs), dtype=np.int64, count=len(pairs))
        vals = np.fromiter((p[1] for p in pairs), dtype=np.int64, count=len(pairs))
        ok = (keys >= 0) & (keys < n_rows)
        out[keys[ok]] = vals[ok]
    return out


def _gold_rows(gold, n_rows: int) -> np.ndarray:
    """What every `gold_ranks` takes -- the dict of `hits`, or an integer array with one gold id per query row and -1 for none --
    as the int64 vector the native calls read: _NO_GOLD where a row has no gold id."""
    if isinstance(gold, dict):
        return _gold_vector(gold, n_rows)
    gold_arr = np.asarray(gold)
    if gold_arr.shape != (n_rows,) or not np.issubdtype(gold_arr.dtype, np.integer):
        raise ValueError(f"gold must be a dict or an integer array with one gold id per query row ({n_rows},), -1 for none")
    gold_arr = gold_arr.astype(np.int64)
    gold_arr[gold_arr < 0] = _NO_GOLD
    return gold_arr


def _rank_stats(ranks, ks: List[int], ctx: Optional[N.Context]):
    """([#(0 <= rank < k) for k in ks], #(rank >= 0), sum(rank + 1), sum 1 / (rank + 1)) of a rank vector, reduced on the device."""
    if isinstance(ranks, N.DeviceArray):
        if ranks.dtype != np.int64 or len(ranks.shape) != 1:
            raise ValueError("ranks must be a one-dimensional int64 vector")
        ctx, rank_dev = ranks.ctx, ranks
    else:
        arr = np.asarray(ranks)
        if arr.ndim != 1 or not (np.issubdtype(arr.dtype, np.integer) or arr.size == 0):
            raise ValueError("ranks must be a one-dimensional integer vector")
        if arr.size == 0:
            return [0] * len(ks), 0, 0.0, 0.0
        ctx = ctx or N.Context.get()
        rank_dev = ctx.to_device(arr.astype(np.int64))
    if rank_dev.shape[0] == 0:
        return [0] * len(ks), 0, 0.0, 0.0
    return N.rank_stats(ctx, rank_dev, ks)


def rank_metrics(ranks: Union[np.ndarray, list, "N.DeviceArray"], gold, k=None, ctx: Optional[N.Context] = None) -> Dict[str, Any]:
    """hits@k, mean rank and mean reciprocal rank from the exact ranks of the gold targets (`Kiez.gold_ranks`,
    `SklearnNN.gold_ranks_device`: 0-based, -1 = the row has no rank), for every k in `k` (default [1, 5, 10]) -- any k, also
    beyond the longest neighbour list a search returns.

    `gold` is what `gold_ranks` was given: the dict of `hits` (every pair counts, also one whose key is no query row) or the array
    with -1 for rows without gold.  Returns {"hits": {k: #(0 <= rank < k) / n_gold}, "mr": mean(rank + 1), "mrr": mean(1 / (rank + 1)),
    "n_ranked": ..., "n_gold": ...}: `hits` has the denominator of `evaluate.hits`, len(gold), so the two agree wherever a list is
    long enough to hold the answer; `mr` and `mrr` average over the n_ranked pairs that have a rank (nan when there is none).
    The rank vector is reduced on the device (kz_rank_stats); only the scalars come to the host."""
    if k is None:
        k = [1, 5, 10]
    k = sorted(k)
    n_gold = len(gold) if isinstance(gold, dict) else int(np.count_nonzero(np.asarray(gold) >= 0))
    int64_max = int(np.iinfo(np.int64).max)
    counts, n_ranked, sum_pos, sum_rec = _rank_stats(ranks, [min(max(int(kk), 0), int64_max) for kk in k], ctx)
    return {"hits": {kk: (c / n_gold if n_gold else 0.0) for kk, c in zip(k, counts)},
            "mr": sum_pos / n_ranked if n_ranked else float("nan"),
            "mrr": sum_rec / n_ranked if n_ranked else float("nan"),
            "n_ranked": n_ranked, "n_gold": n_gold}


def hits(nn_ind: Union[np.ndarray, list, Dict[Any, List], "N.DeviceArray"], gold: Dict[Any, Any], k=None,
         ctx: Optional[N.Context] = None) -> Dict[int, float]:
    """Relative hits@k for every k in `k` (default [1, 5, 10]); same semantics as the reference."""
    if k is None:
        k = [1, 5, 10]
    k = sorted(k)
    if isinstance(nn_ind, dict):
        # encode labels: neighbour labels and gold targets share one code table; rows follow the dict order
        codes: Dict[Any, int] = {}

        def code(x):
            return codes.setdefault(x, len(codes))
        keys = list(nn_ind.keys())
        width = max((len(v) for v in nn_ind.values()), default=0)
        mat = np.full((len(keys), max(width, 1)), -1, dtype=np.int64)
        for r, key in enumerate(keys):
            row = [code(x) for x in nn_ind[key]]
            mat[r, : len(row)] = row
        gold_arr = np.array([code(gold[key]) if key in gold else _NO_GOLD for key in keys], dtype=np.int64)
        ind_host = mat
    elif isinstance(nn_ind, N.DeviceArray):
        ind_host = None
        n_rows = nn_ind.shape[0]
        gold_arr = _gold_vector(gold, n_rows)
    else:
        ind_host = np.ascontiguousarray(np.asarray(nn_ind), dtype=np.int64)
        if ind_host.ndim != 2:
            raise ValueError("nn_ind must be a 2D neighbour index matrix")
        gold_arr = _gold_vector(gold, ind_host.shape[0])
    if isinstance(nn_ind, N.DeviceArray):
        ctx = nn_ind.ctx
        ind_dev = nn_ind
    else:
        ctx = ctx or N.Context.get()
        ind_dev = ctx.to_device(ind_host)
    cols = ind_dev.shape[1]
    hist = N.hit_positions(ctx, ind_dev, ctx.to_device(gold_arr))   # (the uploaded gold vector is held until the call returns)
    cum = np.cumsum(hist.numpy()[:cols])
    return {kk: (float(cum[min(kk, cols) - 1]) / len(gold) if kk >= 1 else 0.0) for kk in k}


def _labels(what: str, label) -> np.ndarray:
    """One label vector of a clustering on the host: a 1-D array of integers >= 0."""
    arr = label.numpy() if isinstance(label, N.DeviceArray) else np.asarray(label)
    if arr.ndim != 1 or not (np.issubdtype(arr.dtype, np.integer) or arr.size == 0) or arr.dtype == np.bool_:
        raise ValueError(f"{what} must be a one-dimensional integer vector of cluster ids")
    arr = arr.astype(np.int64, copy=False)
    if arr.size and arr.min() < 0:
        raise ValueError(f"{what} holds a negative cluster id")
    return arr


def cluster_metrics(source_label, target_label, gold) -> Dict[str, Any]:
    """Precision, recall and F1 of the pairs a clustering of source and target rows IMPLIES -- every (i, j) with
    `source_label[i] == target_label[j]` -- against the gold pairs: the score of `matching.components_csr`, `Kiez.components_radius`
    and `Kiez.components_pairs` (numpy arrays or `DeviceArray`s, which are brought to the host).

    `gold`: the dict of `hits`, or the integer array with one gold target per source row and -1 for none.  Returns {"precision":
    n_true / n_pairs (0.0 without a pair), "recall": n_true / n_gold, "f1", "n_pairs": the sum over the clusters of (source rows x
    target rows), a Python int, "n_true": the gold pairs (i, gold[i]) with gold[i] a target row and both ends in one cluster,
    "n_gold": as `rank_metrics` counts it, "n_components"}.  A gold id that is no target row counts in n_gold only.  O(n) integer
    work on the host, the sizes by one bincount per side."""
    src, tgt = _labels("source_label", source_label), _labels("target_label", target_label)
    gold_arr = _gold_rows(gold, src.shape[0])
    n_gold = len(gold) if isinstance(gold, dict) else int(np.count_nonzero(gold_arr != _NO_GOLD))
    n_components = int(max(src.max(initial=-1), tgt.max(initial=-1))) + 1
    n_source_in = np.bincount(src, minlength=n_components)
    n_target_in = np.bincount(tgt, minlength=n_components)
    # (at most n_source x n_target: exact in int64 for every row count the library takes, and beyond in float-free Python ints)
    if src.shape[0] * tgt.shape[0] < 2 ** 63:
        n_pairs = int(np.dot(n_source_in.astype(np.int64), n_target_in.astype(np.int64)))
    else:
        n_pairs = sum(int(a) * int(b) for a, b in zip(n_source_in, n_target_in))
    rows = np.flatnonzero((gold_arr >= 0) & (gold_arr < tgt.shape[0]))
    n_true = int(np.count_nonzero(src[rows] == tgt[gold_arr[rows]]))
    precision = n_true / n_pairs if n_pairs else 0.0
    recall = n_true / n_gold if n_gold else 0.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return {"precision": precision, "recall": recall, "f1": f1, "n_pairs": n_pairs, "n_true": n_true, "n_gold": n_gold,
            "n_components": n_components}


def cluster_curve(hierarchy, gold, thresholds=None, max_points: int = 64) -> Dict[str, Any]:
    """Precision, recall and F1 of the clustering at a sweep of thresholds, from one single-linkage hierarchy
    (`matching.single_linkage_csr`, `Kiez.hierarchy_radius`, `Kiez.hierarchy_pairs`): every point is `hierarchy.cut(t)` scored by
    `cluster_metrics` -- a components call over at most n_source + n_target - 1 edges, no join.

    `thresholds`: the values of t (any order, no NaN); None: at most `max_points` of the DISTINCT forest values at evenly spaced
    positions, the largest one included -- the thresholds at which the clustering changes.  Returns {"threshold", "precision",
    "recall", "f1" (float64 arrays), "n_components", "n_pairs" (int64 arrays; n_pairs as Python ints in an object array where it
    exceeds int64), "best": the first index of the largest F1 (None for an empty sweep)}."""
    if thresholds is None:
        if isinstance(max_points, (bool, np.bool_)) or not isinstance(max_points, (int, np.integer)) or max_points < 1:
            raise ValueError(f"max_points must be a positive integer, got {max_points!r}")
        distinct = np.unique(hierarchy.value)   # (ascending; -0.0 and +0.0 are one value)
        if distinct.size > max_points:
            # evenly spaced positions that end at the last one (one point: the last)
            pos = np.round(np.linspace(0 if max_points > 1 else distinct.size - 1, distinct.size - 1, max_points)).astype(np.int64)
            distinct = distinct[np.unique(pos)]
        ts = distinct
    else:
        ts = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if np.isnan(ts).any():
            raise ValueError("thresholds must not hold NaN")
    points = [cluster_metrics(*hierarchy.cut(float(t)), gold) for t in ts]
    n_pairs = [p["n_pairs"] for p in points]
    f1 = np.array([p["f1"] for p in points], dtype=np.float64)
    return {"threshold": np.asarray(ts, dtype=np.float64),
            "precision": np.array([p["precision"] for p in points], dtype=np.float64),
            "recall": np.array([p["recall"] for p in points], dtype=np.float64),
            "f1": f1,
            "n_components": np.array([p["n_components"] for p in points], dtype=np.int64),
            "n_pairs": np.array(n_pairs, dtype=np.int64 if all(n < 2 ** 63 for n in n_pairs) else object),
            "best": int(np.argmax(f1)) if f1.size else None}
