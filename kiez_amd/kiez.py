"""The `Kiez` facade over the MI355X exact backend.

Drop-in for the reference's `kiez.Kiez` (kiez/kiez.py:18-223): same constructor arguments, methods, properties, error
types and message texts; everything between `fit` and the returned `(dist, ind)` runs on the GPU through the C ABI.
The facade itself is three small pieces: argument validation (`_candidate_count`), the two name resolvers, and thin
delegation to the resolved `HubnessReduction` object, which owns the `NNAlgorithm`.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import numpy as np

from . import _native as N
from .hubness_reduction import (CSLS, DisSimLocal, HubnessReduction, LocalScaling, MutualProximity,
                                NoHubnessReduction)
from .neighbors import NNAlgorithm, SklearnNN, available_nn_algorithms
from .resolver import Resolver

# kiez/neighbors/__init__.py:20-26 (default SklearnNN) and kiez/hubness_reduction/__init__.py:9-12 (default "no")
nn_algorithm_resolver = Resolver([SklearnNN], base=NNAlgorithm, default=SklearnNN,
                                 synonyms={"exact": SklearnNN, "hip": SklearnNN, "mi355x": SklearnNN})
hubness_reduction_resolver = Resolver([NoHubnessReduction, CSLS, LocalScaling, MutualProximity, DisSimLocal],
                                      base=HubnessReduction, default=NoHubnessReduction)


def _candidate_count(value) -> int:
    """The reference's checks on `n_candidates` (kiez.py:106-113): integer type first, then positivity."""
    if not np.issubdtype(type(value), np.integer):
        raise TypeError(f"n_neighbors does not take {type(value)} value, enter integer value")
    if value <= 0:
        raise ValueError(f"Expected n_candidates > 0. Got {value}")
    return value


class Kiez:
    """Hubness reduced nearest neighbor search for entity alignment on MI355X.

    Parameters are the reference's: `n_candidates` (candidates fetched per query before hubness reduction), `algorithm`
    / `algorithm_kwargs` (an `NNAlgorithm` instance, class or name; only the exact backend exists here and it is the
    default), `hubness` / `hubness_kwargs` (a `HubnessReduction` instance, class or name; default: none).

    >>> from kiez_amd import Kiez
    >>> import numpy as np
    >>> rng = np.random.RandomState(0)
    >>> source, target = rng.rand(100, 50), rng.rand(100, 50)
    >>> k_inst = Kiez(n_candidates=10, algorithm="SklearnNN", hubness="CSLS")
    >>> nn_dist, nn_ind = k_inst.fit(source, target).kneighbors(5)
    """

    def __init__(self, n_candidates: int = 10, algorithm=None, algorithm_kwargs: Optional[Dict[str, Any]] = None,
                 hubness=None, hubness_kwargs: Optional[Dict[str, Any]] = None):
        n_candidates = _candidate_count(n_candidates)
        # the NN backend learns the candidate count unless its own kwargs already name one (kiez.py:114-117)
        nn_kwargs = {"n_candidates": n_candidates} if algorithm_kwargs is None else algorithm_kwargs
        nn_kwargs.setdefault("n_candidates", n_candidates)
        # (the reference tries Faiss first and falls back to SklearnNN, kiez.py:118-122; the default here IS the exact one)
        nn_algo = nn_algorithm_resolver.make(algorithm, nn_kwargs)
        assert nn_algo
        hub_kwargs = {} if hubness_kwargs is None else hubness_kwargs
        hub_kwargs["nn_algo"] = nn_algo
        self.hubness = hubness_reduction_resolver.make(hubness, hub_kwargs)

    # ---- introspection ------------------------------------------------------------------------------
    @staticmethod
    def show_algorithm_options() -> List[str]:
        return available_nn_algorithms(as_string=True)

    @staticmethod
    def show_hubness_options() -> List[str]:
        return list(hubness_reduction_resolver.options)

    @property
    def algorithm(self):
        return self.hubness.nn_algo

    @algorithm.setter
    def algorithm(self, value):
        self.hubness.nn_algo = value

    def __repr__(self):
        fitted = self.algorithm._describe_source_target_fitted()
        return f"Kiez(algorithm: {self.algorithm}, hubness: {self.hubness}) {fitted}"

    @classmethod
    def from_path(cls, path: Union[str, Path]) -> "Kiez":
        """A Kiez instance from a JSON file of constructor arguments (kiez.py:154-158)."""
        return cls(**json.loads(Path(path).read_text()))

    # ---- the hot path -------------------------------------------------------------------------------
    def fit(self, source, target=None) -> "Kiez":
        self.hubness.fit(source, target)
        return self

    def kneighbors_device(self, k: Optional[int] = None):
        """Like `kneighbors` but the (dist, ind) result stays in HBM as DeviceArrays (no PCIe copy)."""
        return self.hubness.kneighbors_device(k)

    def kneighbors(self, k: Optional[int] = None, return_distance: bool = True):
        dist, ind = self.hubness.kneighbors(k)
        return (dist, ind) if return_distance else ind

    def kneighbors_whole_index_device(self, k: int):
        """Like `kneighbors_whole_index` but the (dist, ind) result stays in HBM as DeviceArrays."""
        return self.hubness.kneighbors_whole_index_device(k)

    def kneighbors_whole_index(self, k: int, return_distance: bool = True):
        """The k nearest targets of every source row by the hubness-reduced distance over the WHOLE target index
        (`HubnessReduction.kneighbors_whole_index`: CSLS, LocalScaling 'standard' / 'nicdm', MutualProximity 'normal'; none: the plain
        `kneighbors(k)`), where `kneighbors(k)` rescales the `n_candidates` nearest targets only.  The lists `gold_ranks(gold,
        reduced=True)` ranks in: hits@k of the two agree.  `k` is required, at most min(n_target, 512), and not clamped to
        `n_candidates`.  MutualProximity 'empiric' and DisSimLocal raise NotImplementedError."""
        dist, ind = self.hubness.kneighbors_whole_index(k)
        return (dist, ind) if return_distance else ind

    def radius_neighbors(self, radius, reduced: bool = False, return_distance: bool = True, sort_results: bool = True,
                         ragged: bool = False):
        """Every target row within `radius` of every source row, over the whole target index: the similarity join by threshold, the
        abstain rule for dangling entities (an empty row: no target is close enough) -- `radius_neighbors` of scikit-learn's
        `NearestNeighbors`, without an n_source x n_target matrix and without `kneighbors_whole_index`'s fixed width.

        `reduced` has the meaning it has in `gold_ranks`.  False: pair (i, j) is in the result exactly when d_ij <= radius under the
        SEARCH METRIC, whatever the hubness setting (`SklearnNN.radius_neighbors`).  True: when w_ij <= radius under the
        hubness-reduced distances of the fitted reduction (`HubnessReduction.radius_neighbors`: CSLS, LocalScaling 'standard' /
        'nicdm', MutualProximity 'normal' -- there w is a probability --; none: the plain result); MutualProximity 'empiric' and
        DisSimLocal raise NotImplementedError.  `radius` is a real number -- negative values and infinities are legal, NaN raises
        ValueError, a bool TypeError.  A NaN value is never in the result.  A single-source fit raises NotImplementedError.

        Returns the CSR `(indptr int64 [n_source + 1], ind int64 [total], dist [total])`, or `(indptr, ind)` with
        `return_distance=False`: the targets of source row i are `ind[indptr[i]:indptr[i + 1]]`, ascending by (value, target row) or,
        with `sort_results=False`, by target row.  numpy arrays, or tensors when fitted on tensors.  `dist` is in the dtype
        `kneighbors` returns; for float32 cosine / precomputed input the float64 value is rounded to float32 AFTER it was compared, so
        a float32 distance may round to just above `radius`.  `ragged=True` gives scikit-learn's layout instead -- `(dist, ind)` or
        `ind`, numpy object arrays of one array per source row -- by one split on the host."""
        algo = self.hubness if reduced else self.algorithm
        res = algo.radius_neighbors(radius, return_distance=return_distance, sort_results=sort_results)
        if not ragged:
            return res
        host = [r.cpu().numpy() if hasattr(r, "cpu") else r for r in res]
        cuts = host[0][1:-1]

        def rows(flat):
            out = np.empty(len(host[0]) - 1, dtype=object)
            out[:] = np.split(flat, cuts)
            return out
        return (rows(host[2]), rows(host[1])) if return_distance else rows(host[1])

    def radius_counts(self, radius, reduced: bool = False):
        """The number of target rows within `radius` of every source row (`radius_neighbors`' rule and `reduced`): int64 [n_source],
        the per-row density count -- no pair is stored."""
        return (self.hubness if reduced else self.algorithm).radius_counts(radius)

    def _lists_for_matching(self, k, whole_index):
        """The device lists a one-to-one step runs on -> a `PairList`."""
        nn = self.algorithm
        cached = getattr(nn, "_forward", None)
        dist, ind = self.kneighbors_whole_index_device(k) if whole_index else self.kneighbors_device(k)
        if cached is not None and nn._forward is None:
            nn._forward = cached   # (the shared sweep's forward lists stay cached for the kneighbors() that follows, as after gold_ranks)
        return N.PairList.lists(dist.ctx, dist, ind, nn.target_.shape[0])

    # the three consumers of a `PairList`, whichever producer made it and whichever layout it has
    @staticmethod
    def _match_of(pairs):
        match, col, _ = pairs.match()
        return pairs.values(col), match

    @staticmethod
    def _assign_of(make_pairs, unmatched_cost, eps):
        from . import matching
        unmatched_cost, eps, _ = matching._assignment_options(unmatched_cost, eps, 1)   # (checked before the search runs)
        return matching._assignment_of(make_pairs(), unmatched_cost, eps)

    @staticmethod
    def _components_of(pairs, return_sizes):
        from . import matching
        return matching._components_of(pairs, return_sizes)

    def match_device(self, k: Optional[int] = None, whole_index: bool = False):
        """Like `match` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._match_of(self._lists_for_matching(k, whole_index))

    def match(self, k: Optional[int] = None, whole_index: bool = False, return_distance: bool = True):
        """One-to-one alignment of the fitted source and target rows: the source-proposing stable matching (`matching.one_to_one`)
        over the neighbour lists of `kneighbors(k)` or, with `whole_index=True`, of `kneighbors_whole_index(k)`.  Both kinds of
        list are sorted by value, so the matching is the greedy assignment over all listed pairs in the order (value, source row,
        column).  `k`, its warnings and every error are those of the list call.  The lists never leave HBM; the matching runs on the
        device (kz_match_lists).

        Returns `(match_dist, match_ind)` or, with `return_distance=False`, `match_ind`: per source row the matched target row
        (-1: none) and the value of that pair in the lists' dtype (NaN: none).  No target row appears twice.  The result is numpy
        arrays also after a fit on tensors: tensor output is out of scope.  `evaluate.hits(match_ind[:, None], gold, k=[1])` is the
        precision of the matching."""
        match_dist, match_ind = self.match_device(k, whole_index)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    def assign_device(self, k: Optional[int] = None, whole_index: bool = False, unmatched_cost: Optional[float] = None,
                      eps: Optional[float] = None):
        """Like `assign` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._assign_of(lambda: self._lists_for_matching(k, whole_index), unmatched_cost, eps)

    def assign(self, k: Optional[int] = None, whole_index: bool = False, return_distance: bool = True,
               unmatched_cost: Optional[float] = None, eps: Optional[float] = None):
        """One-to-one alignment of the fitted source and target rows by the minimum-cost assignment (`matching.assignment`) over
        the lists `match` runs on: the total value of the matched pairs plus `unmatched_cost` per unmatched source row is within
        `n_q * eps` of the smallest any one-to-one matching over these lists reaches, where `match` takes pairs greedily.
        `unmatched_cost` (default: the largest listed value) is also the threshold above which a pair is never taken; `eps`
        defaults to a thousandth of the lists' value spread divided by the number of source rows.  The lists never leave HBM; the
        auction runs on the device (kz_assign_lists).  Returns what `match` returns."""
        match_dist, match_ind = self.assign_device(k, whole_index, unmatched_cost, eps)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    # ---- threshold, then one-to-one: the same two steps on the pairs within a radius (a CSR, rows of any length) ----------------
    def _pairs_within_radius(self, radius, reduced):
        """The device CSR of `radius_neighbors(radius, reduced=reduced)`, rows by (value, target row) -> a `PairList`."""
        algo = self.hubness if reduced else self.algorithm
        indptr, ind, dist = algo.radius_neighbors_device(radius, sort_results=True)
        return N.PairList.csr(dist.ctx, indptr, ind, dist, self.algorithm.target_.shape[0])

    def match_radius_device(self, radius, reduced: bool = False):
        """Like `match_radius` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._match_of(self._pairs_within_radius(radius, reduced))

    def match_radius(self, radius, reduced: bool = False, return_distance: bool = True):
        """Threshold, then one-to-one: `match` over the pairs of `radius_neighbors(radius, reduced=reduced)` instead of neighbour lists
        -- every check and error of that call applies, `reduced` has its meaning there.  Each row lists its targets by (value, target
        row), so a pair above the threshold takes NO PART in the matching: the dangling-aware pipeline, which filtering the result
        of `match(k)` is not.  The CSR never leaves HBM and its rows have no length limit -- a hub row of more than 4 096 targets
        is fine (kz_match_csr).  Returns what `match` returns."""
        match_dist, match_ind = self.match_radius_device(radius, reduced)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    def assign_radius_device(self, radius, reduced: bool = False, unmatched_cost: Optional[float] = None, eps: Optional[float] = None):
        """Like `assign_radius` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._assign_of(lambda: self._pairs_within_radius(radius, reduced), unmatched_cost, eps)

    def assign_radius(self, radius, reduced: bool = False, return_distance: bool = True, unmatched_cost: Optional[float] = None,
                      eps: Optional[float] = None):
        """`assign` over the pairs of `radius_neighbors(radius, reduced=reduced)`, as `match_radius` takes them: the minimum-cost
        one-to-one matching among the pairs within the threshold (kz_assign_csr); `unmatched_cost` and `eps` as in `assign`.
        Returns what `match` returns."""
        match_dist, match_ind = self.assign_radius_device(radius, reduced, unmatched_cost, eps)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    # ---- both directions, then one-to-one: the same two steps on the neighbour pairs of both searches (a CSR, rows of any length) --
    def neighbor_pairs_device(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_distance: bool = True,
                              sort_results: bool = True):
        """Like `neighbor_pairs` but the CSR stays in HBM as DeviceArrays."""
        algo = self.hubness if reduced else self.algorithm
        return algo.neighbor_pairs_device(k, mode, sort_results, return_distance)

    def neighbor_pairs(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_distance: bool = True,
                       sort_results: bool = True):
        """The neighbour pairs of BOTH search directions as one CSR over the source rows: F = (i, j) with target j among the k nearest
        targets of source i, R = (i, j) with source i among the k nearest sources of target j, and `mode` "forward" (F), "reverse" (R,
        grouped by source row), "union" (F | R: bidirectional candidate generation -- a target that no source lists still takes
        part) or "mutual" (F & R: mutual nearest neighbours, the high-precision filter of bootstrapping alignment).  Membership is
        always decided by the raw lists of the two searches under the search metric, ties included; every pair appears once.

        `reduced` has the meaning it has in `radius_neighbors`: False values a pair by the distance `kneighbors` computes from source
        i to target j -- also a pair only R holds --, True by the hubness-reduced distance of the fitted reduction
        (`HubnessReduction.neighbor_pairs`; none: the plain values; MutualProximity 'empiric' and DisSimLocal raise
        NotImplementedError).  Either way the value has the bits `radius_neighbors(inf, reduced=...)` returns for the pair.  A NaN
        value stays in the result and sorts last.  `k`: None means `n_candidates`, else an int >= 1 that is NOT clamped to
        `n_candidates`.

        Returns the CSR `(indptr int64 [n_source + 1], ind int64 [total], dist [total])`, or `(indptr, ind)` with
        `return_distance=False`, rows ascending by (value, target row) or, with `sort_results=False`, by target row; numpy arrays, or
        tensors when fitted on tensors.  ValueError for another `mode` or a k that is no positive int, NotFittedError before `fit`,
        NotImplementedError after a single-source fit."""
        algo = self.hubness if reduced else self.algorithm
        return algo.neighbor_pairs(k, mode, return_distance, sort_results)

    def _pairs_of_both_directions(self, k, mode, reduced):
        """The device CSR of `neighbor_pairs(k, mode, reduced)`, rows by (value, target row) -> a `PairList`."""
        indptr, ind, dist = self.neighbor_pairs_device(k, mode, reduced)
        return N.PairList.csr(dist.ctx, indptr, ind, dist, self.algorithm.target_.shape[0])

    def match_pairs_device(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False):
        """Like `match_pairs` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._match_of(self._pairs_of_both_directions(k, mode, reduced))

    def match_pairs(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_distance: bool = True):
        """Both directions, then one-to-one: `match` over the pairs of `neighbor_pairs(k, mode, reduced)` instead of the forward lists
        -- every check and error of that call applies.  "mutual" matches among mutual nearest neighbours only; "union" lets a source
        propose to a target that lists it although it does not list the target.  The CSR never leaves HBM and its rows have no length
        limit (kz_match_csr).  Returns what `match` returns."""
        match_dist, match_ind = self.match_pairs_device(k, mode, reduced)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    def assign_pairs_device(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, unmatched_cost: Optional[float] = None,
                            eps: Optional[float] = None):
        """Like `assign_pairs` but the (match_dist, match_ind) result stays in HBM as DeviceArrays."""
        return self._assign_of(lambda: self._pairs_of_both_directions(k, mode, reduced), unmatched_cost, eps)

    def assign_pairs(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_distance: bool = True,
                     unmatched_cost: Optional[float] = None, eps: Optional[float] = None):
        """`assign` over the pairs of `neighbor_pairs(k, mode, reduced)`, as `match_pairs` takes them: the minimum-cost one-to-one
        matching among the pairs of both directions (kz_assign_csr); `unmatched_cost` and `eps` as in `assign`.  Returns what `match`
        returns."""
        match_dist, match_ind = self.assign_pairs_device(k, mode, reduced, unmatched_cost, eps)
        return (match_dist.numpy(), match_ind.numpy()) if return_distance else match_ind.numpy()

    # ---- threshold or both directions, then the transitive closure: entity clusters of the same two CSRs ------------------------
    def components_radius_device(self, radius, reduced: bool = False, return_sizes: bool = False):
        """Like `components_radius` but the label (and size) arrays stay in HBM as DeviceArrays."""
        return self._components_of(self._pairs_within_radius(radius, reduced), return_sizes)

    def components_radius(self, radius, reduced: bool = False, return_sizes: bool = False):
        """Threshold, then the transitive closure: the entity clusters of the pairs of `radius_neighbors(radius, reduced=reduced)` --
        every source and target row connected through accepted pairs is one cluster (`matching.components_csr`), where `match_radius`
        forces a one-to-one answer.  Every check and error of the radius call applies, `reduced` has its meaning there.  The CSR
        never leaves HBM (kz_components_csr).

        Returns `(source_label int64 [n_source], target_label int64 [n_target])`, clusters numbered in the order of their smallest
        node, source rows before target rows; with `return_sizes=True` also `(n_source_in, n_target_in)`, the rows of every cluster
        per side: `(n_source_in == 1) & (n_target_in == 1)` are the unambiguous alignments, 1:n and n:m clusters the non-bijective
        ones, one giant cluster the sign of a threshold that is too loose.  numpy arrays, also after a fit on tensors.
        `evaluate.cluster_metrics(source_label, target_label, gold)` scores the implied pairs."""
        return tuple(x.numpy() for x in self.components_radius_device(radius, reduced, return_sizes))

    def components_pairs_device(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_sizes: bool = False):
        """Like `components_pairs` but the label (and size) arrays stay in HBM as DeviceArrays."""
        return self._components_of(self._pairs_of_both_directions(k, mode, reduced), return_sizes)

    def components_pairs(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False, return_sizes: bool = False):
        """Both directions, then the transitive closure: the entity clusters of the pairs of `neighbor_pairs(k, mode, reduced)` --
        every check and error of that call applies.  With "mutual" and k = 1 every cluster has at most one row per side, and the
        (1, 1) clusters are the pairs `match_pairs(1, "mutual")` returns.  The CSR never leaves HBM (kz_components_csr).  Returns what
        `components_radius` returns."""
        return tuple(x.numpy() for x in self.components_pairs_device(k, mode, reduced, return_sizes))

    # ---- the same two CSRs, then the single-linkage hierarchy: the clusters at EVERY tighter threshold from one join ------------
    def hierarchy_radius(self, radius, reduced: bool = False):
        """One loose join, every tighter threshold: the single-linkage hierarchy (`matching.Hierarchy`) of the pairs of
        `radius_neighbors(radius, reduced=reduced)` -- every check and error of that call applies.  `h.cut(t)` for t <= radius equals
        `components_radius(t, reduced=reduced)` without walking the index again, `h.n_clusters(t)` is host arithmetic and
        `evaluate.cluster_curve(h, gold)` scores a sweep of thresholds.  The CSR never leaves HBM (kz_forest_csr)."""
        from . import matching
        return matching._hierarchy_of(self._pairs_within_radius(radius, reduced))

    def hierarchy_pairs(self, k: Optional[int] = None, mode: str = "union", reduced: bool = False):
        """`hierarchy_radius` over the pairs of `neighbor_pairs(k, mode, reduced)` -- every check and error of that call applies:
        `h.cut(t)` are the clusters of those pairs with value <= t.  The CSR never leaves HBM (kz_forest_csr)."""
        from . import matching
        return matching._hierarchy_of(self._pairs_of_both_directions(k, mode, reduced))

    def gold_ranks(self, gold, s_to_t: bool = True, reduced: bool = False):
        """Exact 0-based rank of every source row's gold target against the whole target index (`evaluate.rank_metrics` turns the
        ranks into hits@k, mean rank and mean reciprocal rank).

        `reduced=False`: under the SEARCH METRIC, whatever the hubness setting (`SklearnNN.gold_ranks`).  `reduced=True`: under the
        hubness-reduced distances of the fitted reduction (`HubnessReduction.gold_ranks`: CSLS, LocalScaling 'standard' / 'nicdm',
        MutualProximity 'normal'; none: the plain ranks) -- every target row is ranked by its reduced distance, with the state taken
        from the `n_candidates` neighbours as `fit` / `kneighbors` use them, so a gold row outside the candidate list has a rank too.
        MutualProximity 'empiric' and DisSimLocal raise NotImplementedError.  The fit state exists for the source -> target
        direction: `reduced=True` with `s_to_t=False` raises ValueError."""
        if not reduced:
            return self.algorithm.gold_ranks(gold, s_to_t=s_to_t)
        if not s_to_t:
            raise ValueError("gold_ranks(reduced=True) ranks source rows against the target index only (s_to_t=True): the hubness "
                             "reduction is fitted for that direction")
        return self.hubness.gold_ranks(gold)
