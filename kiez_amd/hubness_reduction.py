"""Hubness reduction: the reference's `HubnessReduction` plugin interface with GPU implementations.

Mirrors kiez/hubness_reduction/{base,csls,mutual_proximity,local_scaling,dis_sim}.py: same class names,
constructor arguments, fitted attributes, errors and warnings.  `_fit` / `transform` accept what the
reference's do (numpy arrays from any `NNAlgorithm`) and additionally device arrays; when the NN backend is
the MI355X `SklearnNN`, `fit` / `kneighbors` keep every intermediate in HBM and only the final [n, k]
result crosses PCIe.
"""
from __future__ import annotations

import warnings
from abc import ABC, abstractmethod
from typing import Optional, Tuple

import numpy as np

from . import _native as N
from .neighbors import NNAlgorithm, SklearnNN, check_is_fitted


def _is_dev(x):
    return isinstance(x, N.DeviceArray)


def _is_precomputed(nn_algo) -> bool:
    """The MI355X backend fitted on a distance matrix (metric='precomputed'): `fit(D)` alone is a two-sided fit."""
    return isinstance(nn_algo, SklearnNN) and nn_algo._metric_c == "precomputed"


class HubnessReduction(ABC):
    """Base class for hubness reduction (kiez/hubness_reduction/base.py:17-105)."""

    def __init__(self, nn_algo: NNAlgorithm, verbose: int = 0, **kwargs):
        self.nn_algo = nn_algo
        self.verbose = verbose
        self._use_torch = False
        if "native_fit" in kwargs:
            self._native_fit = bool(kwargs["native_fit"])
        self._fitted = None
        if nn_algo.n_candidates == 1:
            raise ValueError("Cannot perform hubness reduction with a single candidate per query!")
        # known at construction, so say it at construction (not after a long fit): the device transforms and the final
        # sort take up to KZ_MAX_CANDIDATES = 4096 candidates per query (the NN backend itself stops at 4095 neighbours)
        if (self._device_native and type(self).__name__ != "NoHubnessReduction" and isinstance(nn_algo.n_candidates, (int, np.integer))
                and nn_algo.n_candidates > N.MAX_HUBNESS_CANDIDATES):
            raise NotImplementedError(f"n_candidates={nn_algo.n_candidates}: the MI355X hubness reductions support up to "
                                      f"{N.MAX_HUBNESS_CANDIDATES} candidates per query")

    # Subclasses shipped here consume device arrays; a user-written subclass (docs/source/using_your_own.rst:11-19)
    # gets numpy arrays exactly as in the reference.
    _device_native = False
    # fit() takes its reverse search and the forward search of the kneighbors() that follows out of ONE sweep of the
    # distance matrix where the native library can (kz_knn_dual; results identical to the two searches).  Set to False on
    # an instance to search twice, as the reference does.
    _shared_sweep = True
    # Opt-in (`hubness_kwargs={"native_fit": True}`): fit() and kneighbors() are ONE native call each (kz_fit / kz_kneighbors: the
    # searches, the fit state, the fused rescale + sort + cast) for the reductions that name a `_native_kind` -- CSLS, LocalScaling,
    # MutualProximity -- on the MI355X backend with an embedding metric.  Same results, bit for bit.  Where the library's plan refuses
    # the fit (a k that would be clamped, a precomputed matrix) and for every other reduction the pipeline below runs as ever.
    _native_fit = False

    def _native_kind(self) -> Optional[int]:
        """The KZ_HUB_* kind `_native.fit` takes for this reduction; None: no native fit."""
        return None

    def _set_native_state(self, fitted: "N.Fitted"):
        """The fitted attributes `_fit` sets, as views into the fitted object."""
        raise NotImplementedError  # pragma: no cover

    def _fit_native(self, source, target) -> bool:
        """fit() through kz_fit.  False -- nothing changed -- where the flag is off, the reduction or the backend has no native fit, or
        the plan refuses (the present pipeline then produces the clamp, the warning or the error)."""
        self._fitted = None
        kind = self._native_kind() if self._native_fit and self._gpu_nn else None
        nn = self.nn_algo
        K = nn.n_candidates
        if kind is None or _is_precomputed(nn) or isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)):
            return False
        try:
            fitted = N.fit(self.ctx, nn.source_index, None if nn.source_equals_target else nn.target_index, kind, int(K), self._shared_sweep)
        except (ValueError, NotImplementedError):
            return False
        self._fitted = fitted
        self._set_native_state(fitted)
        self._native_stats()
        return True

    def _native_stats(self):
        """`last_stats` / `last_stats_reverse` of the backend from the fitted object's record of its searches."""
        info = self._fitted.info
        nn = self.nn_algo
        if info["forward_ready"]:
            nn.last_stats = info["stats_forward"]
        nn.last_stats_reverse = info["stats_reverse"] if info["search"] in (N.FIT_SEARCH_DUAL, N.FIT_SEARCH_REVERSE) else None

    # ---- device helpers ---------------------------------------------------------------------------
    @property
    def _gpu_nn(self) -> bool:
        return self._device_native and isinstance(self.nn_algo, SklearnNN)

    @property
    def ctx(self) -> N.Context:
        if self._gpu_nn:
            return self.nn_algo.ctx
        if getattr(self, "_ctx", None) is None:
            self._ctx = N.Context.get()
        return self._ctx

    def _out_dtype(self, like):
        """dtype of the distances the reference would return for this input."""
        if _is_dev(like):
            return np.float64
        return np.float32 if np.asarray(like).dtype == np.float32 else np.float64

    @abstractmethod
    def _fit(self, neigh_dist, neigh_ind, source, target):
        pass  # pragma: no cover

    def fit(self, source, target=None):
        """base.py:33-50: index both sides, run the reverse (target -> source) kNN, hand it to `_fit`."""
        self.nn_algo.fit(source, target)
        if target is None:
            # (a precomputed distance matrix is two-sided by itself: its target side is the backend's `target_`, a distinct object
            #  that the backend resolves to the matrix' COLUMNS view -- `source` again would resolve to the rows view)
            target = self.nn_algo.target_ if _is_precomputed(self.nn_algo) else source
        if self._fit_native(source, target):
            return
        if self._gpu_nn:
            # one sweep of the distance matrix serves this reverse search AND the forward search of kneighbors()
            # (kz_knn_dual); where that does not apply, the reverse search alone
            both = self.nn_algo.kneighbors_device_both(k=self.nn_algo.n_candidates) if self._shared_sweep else None
            if both is not None:
                neigh_dist_t_to_s, neigh_ind_t_to_s = both
            else:
                neigh_dist_t_to_s, neigh_ind_t_to_s = self.nn_algo.kneighbors_device(
                    k=self.nn_algo.n_candidates, query=target, s_to_t=False)
        else:
            neigh_dist_t_to_s, neigh_ind_t_to_s = self.nn_algo.kneighbors(
                k=self.nn_algo.n_candidates, query=target, s_to_t=False, return_distance=True)
        self._fit(neigh_dist_t_to_s, neigh_ind_t_to_s, source, target)

    @abstractmethod
    def transform(self, neigh_dist, neigh_ind, query) -> Tuple:
        pass  # pragma: no cover

    def _set_k_if_needed(self, k: Optional[int] = None) -> int:
        if k is None:
            warnings.warn(f"No k supplied, setting to n_candidates = {self.nn_algo.n_candidates}", stacklevel=2)
            return self.nn_algo.n_candidates
        if k > self.nn_algo.n_candidates:
            warnings.warn(f"k > n_candidates supplied! Setting to n_candidates = {self.nn_algo.n_candidates}", stacklevel=2)
            return self.nn_algo.n_candidates
        return k

    @staticmethod
    def _sort(hubness_reduced_query_dist, query_ind, n_neighbors: int, ctx: Optional[N.Context] = None):
        """base.py:72-87 (numpy branch) on the GPU: kz_select_topk.  numpy in -> numpy out; device in -> device out."""
        dev_in = _is_dev(hubness_reduced_query_dist)
        if ctx is None:
            ctx = hubness_reduced_query_dist.ctx if dev_in else N.Context.get()
        out_dtype = np.float64 if dev_in else np.asarray(hubness_reduced_query_dist).dtype
        d = ctx.as_device(hubness_reduced_query_dist, np.float64) if not dev_in else hubness_reduced_query_dist
        i = ctx.as_device(query_ind, np.int64)
        n_neighbors = min(int(n_neighbors), d.shape[1])
        od, oi = N.select_topk(ctx, d, i, n_neighbors)
        if dev_in:
            return od, oi
        od_h = od.numpy()
        if out_dtype == np.float32:
            od_h = od_h.astype(np.float32)
        return od_h, oi.numpy()

    def kneighbors_device(self, k: Optional[int] = None):
        """`kneighbors` with the result left in HBM (MI355X NN backend only): (dist, ind) DeviceArrays."""
        if not self._gpu_nn:
            raise TypeError("kneighbors_device needs the MI355X SklearnNN backend")
        n_neighbors = self._set_k_if_needed(k)
        nn = self.nn_algo
        if self._fitted is not None:   # (native_fit: the forward search if the fit left it, rescale + sort + cast, one call)
            od, oi = self._fitted.kneighbors(n_neighbors, nn._out_dtype(nn.target_index))
            self._native_stats()
            return od, oi
        query_dist, query_ind = nn.kneighbors_device(query=None, k=nn.n_candidates)
        hub_dist, query_ind = self.transform(query_dist, query_ind, nn.source_)
        od, oi = HubnessReduction._sort(hub_dist, query_ind, n_neighbors, ctx=self.ctx)
        if nn._out_dtype(nn.target_index) == np.float32:
            od = N.cast_f32(self.ctx, od)
        return od, oi

    def kneighbors(self, k: Optional[int] = None):
        """base.py:89-105: forward candidates, rescale, final top-k."""
        if self._gpu_nn:
            od, oi = self.kneighbors_device(k)
            return self._to_host(od, oi)
        n_neighbors = self._set_k_if_needed(k)
        query_dist, query_ind = self.nn_algo.kneighbors(query=None, k=self.nn_algo.n_candidates, return_distance=True)
        hub_dist, query_ind = self.transform(query_dist, query_ind, self.nn_algo.source_)
        return HubnessReduction._sort(hub_dist, query_ind, n_neighbors, ctx=self.ctx)

    # ---- ranks of gold targets under the reduced distances -------------------------------------------
    # why gold_ranks cannot rank under this reduction (None: it can, and `_rank_state` says how)
    _no_rank_reason: Optional[str] = ("this reduction has no rank over the whole index: gold_ranks needs a reduction that is a function "
                                      "of a pair's distance and one state per side (CSLS, LocalScaling, MutualProximity 'normal')")

    def _rank_state(self, query_dist):
        """(kind, query-side state vectors of the forward lists `query_dist`, index-side fit state) for kz_gold_ranks_reduced."""
        raise NotImplementedError(self._no_rank_reason)

    def _forward_rank_state(self):
        """`_rank_state` of the forward lists of kneighbors().  When they are the shared sweep's cached result, the cache is left as it
        was found, so the kneighbors() that follows is served as it would have been."""
        nn = self.nn_algo
        cached = nn._forward
        query_dist, _ = nn.kneighbors_device(query=None, k=nn.n_candidates)
        if cached is not None and cached[1] is query_dist:
            nn._forward = cached
        return self._rank_state(query_dist)

    def gold_ranks_device(self, gold) -> N.DeviceArray:
        """`gold_ranks` that leaves the int64 rank vector in HBM (evaluate.rank_metrics reduces it there)."""
        if not self._gpu_nn:
            raise NotImplementedError("gold_ranks under a hubness reduction needs one of the device-native reductions on the "
                                      "MI355X SklearnNN backend")
        nn = self.nn_algo
        query, index, gold_dev = nn._gold_rank_operands(gold)   # (NotFittedError, single-source fit: as the plain call)
        if self._no_rank_reason:
            raise NotImplementedError(f"{type(self).__name__}: {self._no_rank_reason}")
        kind, q_state, t_state = self._forward_rank_state()
        return N.gold_ranks_reduced(self.ctx, query, index, gold_dev, kind, q_state, t_state)

    def gold_ranks(self, gold) -> np.ndarray:
        """Exact 0-based rank of every source row's gold target against the WHOLE target index under the HUBNESS-REDUCED distances
        (`SklearnNN.gold_ranks`: under the search metric; same `gold`, same result vector, -1 = no gold id).

        CSLS, LocalScaling ('standard', 'nicdm') and MutualProximity 'normal' rescale a pair's distance d with one state of the
        source row and one of the target row: w = f(d, a_i, b_j) is defined for every target row, as CSLS was defined.  The state
        is what `fit` / `kneighbors` use -- statistics of the K = n_candidates forward and reverse neighbours -- d is the distance the
        search returns for the pair, and rank_i = #{j : w_ij < w_ig or (w_ij == w_ig and j < g)}, NaN ranked as +inf by row.
        * With lists over the whole index (n_candidates = n_target) this is the position of g in `transform`'s output row ordered
          by (value, target row), bit for bit.
        * With K < n_target, a gold row inside the candidate list need not have rank == its position in `kneighbors(k)`: a row
          outside the list can have a smaller reduced distance.  Ranking all targets is the point.
        * MutualProximity 'normal' is exactly 1.0 for pairs far beyond both lists (the product of two survival functions falls
          below 2^-53): with small K most pairs tie there and are ordered by target row.
        MutualProximity 'empiric' (its value depends on list membership) and DisSimLocal (its values come from its own gather of
        the embeddings, not from the search's distances) raise NotImplementedError, as does a user-written reduction."""
        return self.gold_ranks_device(gold).numpy()

    # ---- neighbour lists by the reduced distance over the whole index ----------------------------------
    def _whole_index_k(self, k) -> int:
        """The k of `kneighbors_whole_index`: a positive int; never clamped to n_candidates (the list is not cut from the candidates)."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"kneighbors_whole_index needs a positive integer k, got {k!r}")
        return int(k)

    def kneighbors_whole_index_device(self, k: int):
        """`kneighbors_whole_index` with the result left in HBM: (dist, ind) DeviceArrays."""
        k = self._whole_index_k(k)
        if not self._gpu_nn:
            raise NotImplementedError("kneighbors_whole_index needs one of the device-native reductions on the MI355X SklearnNN backend")
        nn = self.nn_algo
        query, index = nn._two_sided_operands("kneighbors_whole_index")   # (NotFittedError, single-source fit: as gold_ranks)
        if self._no_rank_reason:
            raise NotImplementedError(f"{type(self).__name__}: {self._no_rank_reason}")
        if k > index.shape[0]:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {index.shape[0]}")
        if k > N.KNN_REDUCED_MAX_K:
            raise NotImplementedError(f"kneighbors_whole_index returns up to {N.KNN_REDUCED_MAX_K} neighbours per query, got k = {k}: "
                                      "beyond that, gold_ranks ranks any target row against the whole index")
        kind, q_state, t_state = self._forward_rank_state()
        od, oi = N.knn_reduced(self.ctx, query, index, k, kind, q_state, t_state)
        if nn._out_dtype(nn.target_index) == np.float32:
            od = N.cast_f32(self.ctx, od)
        return od, oi

    def kneighbors_whole_index(self, k: int):
        """The k nearest target rows of every source row by the HUBNESS-REDUCED distance over the WHOLE target index: the exact
        CSLS / LocalScaling / NICDM / MutualProximity-'normal' neighbour list, as CSLS was defined over the full similarity matrix.

        `kneighbors(k)` rescales the `n_candidates` nearest targets by raw distance and returns the k best of THOSE; a target
        outside the candidates can have a smaller reduced distance.  Here every target row is a candidate: w = f(d, a_i, b_j)
        with the state `fit` / `kneighbors` use (statistics of the `n_candidates` forward and reverse neighbours) is evaluated for
        every pair, and row i of the result holds the k targets with the smallest w, ascending by (w, target row), NaN last (as
        +inf, by row).  These are the lists `gold_ranks` ranks in: `gold_ranks(gold)[i] == c` exactly when `ind[i, c] == gold[i]`,
        so hits@k from either agree.  `k` is required, at most min(n_target, 512), and is NOT clamped to `n_candidates`.

        Returns (dist, ind) like `kneighbors`: numpy arrays, or tensors when fitted on tensors; dist in the dtype `kneighbors`
        returns.  NoHubnessReduction returns the plain `kneighbors(k)`.  MutualProximity 'empiric', DisSimLocal and user-written
        reductions raise NotImplementedError (no value outside the list), a single-source fit too (two-sided data only)."""
        od, oi = self.kneighbors_whole_index_device(k)
        return self._to_host(od, oi)

    # ---- every pair within a threshold of the reduced distance, whole index -----------------------------
    def _radius_operands(self, what, s_to_t):
        """(query matrix, index matrix, kind, q_state, t_state) of a radius call under the reduced distances, after its checks."""
        if not s_to_t:
            raise ValueError(f"{what} under a hubness reduction takes source rows against the target index only (s_to_t=True): the "
                             "hubness reduction is fitted for that direction")
        if not self._gpu_nn:
            raise NotImplementedError(f"{what} needs one of the device-native reductions on the MI355X SklearnNN backend")
        query, index = self.nn_algo._two_sided_operands(what)   # (NotFittedError, single-source fit: as gold_ranks)
        if self._no_rank_reason:
            raise NotImplementedError(f"{type(self).__name__}: {self._no_rank_reason}")
        return (query, index) + tuple(self._forward_rank_state())

    def radius_neighbors_device(self, radius, s_to_t=True, sort_results=True):
        """`radius_neighbors` with the CSR left in HBM: (indptr, ind, dist) DeviceArrays."""
        radius = N.radius_value(radius)
        query, index, kind, q_state, t_state = self._radius_operands("radius_neighbors", s_to_t)
        indptr, ind, dist, _ = N.radius_neighbors(self.ctx, query, index, radius, kind, q_state, t_state, sort_results)
        return indptr, ind, self.nn_algo._radius_distances(dist, self.nn_algo.target_index)

    def radius_neighbors(self, radius, s_to_t=True, return_distance=True, sort_results=True):
        """Every target row whose HUBNESS-REDUCED distance to a source row is <= `radius`, over the whole target index
        (`SklearnNN.radius_neighbors`: under the search metric; same result layout, same `radius` checks).  w = f(d, a_i, b_j) is
        the value `kneighbors_whole_index` returns for the pair, with the state `fit` / `kneighbors` use; under MutualProximity
        'normal' it is a probability, so `radius=0.05` asks for all pairs with MP <= 0.05.  CSLS values are routinely negative and
        so may `radius` be.  A NaN w is never in the result.  Rows ascend by (w, target row) in `kneighbors_whole_index`'s order:
        a row with at most 512 entries IS the head of that list.  MutualProximity 'empiric', DisSimLocal and user-written reductions
        raise NotImplementedError, `s_to_t=False` ValueError; the shared sweep's cached forward lists are left as found."""
        nn = self.nn_algo
        indptr, ind, dist = self.radius_neighbors_device(radius, s_to_t, sort_results)
        return nn._results_to_host(indptr, ind, dist) if return_distance else nn._results_to_host(indptr, ind)

    def radius_counts(self, radius, s_to_t=True):
        """The number of target rows within `radius` of every source row under the reduced distances: int64 [n_source]."""
        radius = N.radius_value(radius, "radius_counts")
        query, index, kind, q_state, t_state = self._radius_operands("radius_counts", s_to_t)
        indptr, _ = N.radius_counts(self.ctx, query, index, radius, kind, q_state, t_state)
        indptr, = self.nn_algo._results_to_host(indptr)
        return indptr[1:] - indptr[:-1]

    # ---- the neighbour pairs of both directions, valued by the reduced distance -------------------------
    def neighbor_pairs_device(self, k=None, mode="union", sort_results=True, return_distance=True):
        """`neighbor_pairs` with the CSR left in HBM: (indptr, ind, dist) DeviceArrays, or (indptr, ind)."""
        nn = self.nn_algo
        if not self._gpu_nn:
            N.pair_mode(mode)
            raise NotImplementedError("neighbor_pairs needs one of the device-native reductions on the MI355X SklearnNN backend")
        k, mode = nn._pairs_args(k, mode)
        nn._two_sided_operands("neighbor_pairs")   # (NotFittedError, single-source fit: as gold_ranks)
        if self._no_rank_reason:
            raise NotImplementedError(f"{type(self).__name__}: {self._no_rank_reason}")
        kind, q_state, t_state = self._forward_rank_state()
        indptr, ind, dist, _ = nn._neighbor_pairs(k, mode, sort_results, return_distance, kind, q_state, t_state)
        return (indptr, ind, dist) if return_distance else (indptr, ind)

    def neighbor_pairs(self, k=None, mode="union", return_distance=True, sort_results=True):
        """`SklearnNN.neighbor_pairs` with every pair valued by its HUBNESS-REDUCED distance: the same pairs -- membership is decided
        by the raw lists of the two searches, also here: the reduction is fitted one way, and with k = `n_candidates` these are
        exactly the two candidate sets its state is built from -- and w = f(d, a_i, b_j) with the state `fit` / `kneighbors` use, the
        value `radius_neighbors(inf)` and `kneighbors_whole_index` return for the pair; for a pair of the forward lists that is
        `transform`'s output.  A pair only the reverse lists hold is valued all the same (CSLS, LocalScaling 'standard' / 'nicdm',
        MutualProximity 'normal', Sinkhorn / InvertedSoftmax: functions of the pair's distance and one state per side).
        MutualProximity 'empiric', DisSimLocal and user-written reductions raise NotImplementedError; NoHubnessReduction returns the
        plain result.  Rows ascend by (w, target row), a NaN w last.  The shared sweep's cached forward lists are left as found."""
        return self.nn_algo._results_to_host(*self.neighbor_pairs_device(k, mode, sort_results, return_distance))

    def _to_host(self, od: N.DeviceArray, oi: N.DeviceArray):
        """A device result as `kneighbors` hands it out: tensors in -> tensors out on the source's device, else numpy."""
        src = self.nn_algo.source_
        from .neighbors import _is_tensor, _torch_if_loaded
        if _is_tensor(src):
            torch = _torch_if_loaded()
            self.ctx.sync()
            out = (torch.as_tensor(od, device="cuda").clone().to(src.device),
                   torch.as_tensor(oi, device="cuda").clone().to(src.device))
            torch.cuda.current_stream().synchronize()   # before od / oi go back to our stream-ordered pool
            return out
        return od.numpy(), oi.numpy()

    # ---- shared plumbing for the transform kernels -------------------------------------------------
    def _device_inputs(self, neigh_dist, neigh_ind):
        ctx = self.ctx
        return ctx.as_device(neigh_dist, np.float64), ctx.as_device(neigh_ind, np.int64)

    def _finish(self, out: N.DeviceArray, neigh_dist, neigh_ind):
        """device in -> device out; numpy in -> numpy out in the reference's dtype."""
        if _is_dev(neigh_dist):
            return out, neigh_ind
        res = out.numpy()
        dt = self._out_dtype(neigh_dist)
        if dt != np.float64:
            res = res.astype(dt)
        return res, neigh_ind


class NoHubnessReduction(HubnessReduction):
    """kiez/hubness_reduction/base.py:108-122: no reverse pass, the NN result is returned directly."""

    _device_native = True

    def _fit(self, neigh_dist, neigh_ind, source, target):
        pass  # pragma: no cover

    def fit(self, source, target=None):
        self.nn_algo.fit(source, target, only_fit_target=True)

    def transform(self, neigh_dist, neigh_ind, query):
        return neigh_dist, neigh_ind

    def kneighbors_device(self, k: Optional[int] = None):
        n_neighbors = self._set_k_if_needed(k)
        nn = self.nn_algo
        od, oi = nn.kneighbors_device(query=None, k=n_neighbors)
        if nn._out_dtype(nn.target_index) == np.float32:
            od = N.cast_f32(self.ctx, od)
        return od, oi

    def kneighbors(self, k: Optional[int] = None):
        n_neighbors = self._set_k_if_needed(k)
        return self.nn_algo.kneighbors(query=None, k=n_neighbors, return_distance=True)

    def gold_ranks_device(self, gold) -> N.DeviceArray:
        return self.nn_algo.gold_ranks_device(gold)   # (nothing is rescaled: the ranks under the search metric)

    # (nothing is rescaled: the search's own lists ARE over the whole index)
    def kneighbors_whole_index_device(self, k: int):
        return self.kneighbors_device(self._whole_index_k(k))

    def kneighbors_whole_index(self, k: int):
        return self.kneighbors(self._whole_index_k(k))

    # (nothing is rescaled: the pairs within a threshold of the search metric)
    def radius_neighbors_device(self, radius, s_to_t=True, sort_results=True):
        return self.nn_algo.radius_neighbors_device(radius, s_to_t, sort_results)

    def radius_neighbors(self, radius, s_to_t=True, return_distance=True, sort_results=True):
        return self.nn_algo.radius_neighbors(radius, s_to_t, return_distance, sort_results)

    def radius_counts(self, radius, s_to_t=True):
        return self.nn_algo.radius_counts(radius, s_to_t)

    # (nothing is rescaled: the pairs with the search's own distances)
    def neighbor_pairs_device(self, k=None, mode="union", sort_results=True, return_distance=True):
        return self.nn_algo.neighbor_pairs_device(k, mode, sort_results, return_distance)

    def neighbor_pairs(self, k=None, mode="union", return_distance=True, sort_results=True):
        return self.nn_algo.neighbor_pairs(k, mode, return_distance, sort_results)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class CSLS(HubnessReduction):
    """Cross-domain similarity local scaling (kiez/hubness_reduction/csls.py)."""

    _device_native = True

    def __repr__(self):
        return f"{self.__class__.__name__}(verbose = {self.verbose})"

    def _fit(self, neigh_dist, neigh_ind, source=None, target=None) -> "CSLS":
        self.r_dist_train_ = neigh_dist            # csls.py:53
        self.r_ind_train_ = neigh_ind              # csls.py:54
        d = self.ctx.as_device(neigh_dist, np.float64)
        self._r_train_dev, _, _ = N.row_stats(self.ctx, d, mean=True)   # csls.py:90, hoisted into fit
        return self

    def _native_kind(self):
        return N.HUB_CSLS

    def _set_native_state(self, fitted):
        self.r_dist_train_ = fitted.state("reverse_dist")
        self.r_ind_train_ = fitted.state("reverse_ind")
        self._r_train_dev = fitted.state("state_a")

    _no_rank_reason = None

    def _rank_state(self, query_dist):
        check_is_fitted(self, "r_dist_train_")
        r_test, _, _ = N.row_stats(self.ctx, query_dist, mean=True)
        return N.RANK_CSLS, r_test, self._r_train_dev

    def transform(self, neigh_dist, neigh_ind, query):
        check_is_fitted(self, "r_dist_train_")
        d, i = self._device_inputs(neigh_dist, neigh_ind)
        return self._finish(N.csls(self.ctx, d, i, self._r_train_dev), neigh_dist, neigh_ind)


class LocalScaling(HubnessReduction):
    """Local scaling / NICDM (kiez/hubness_reduction/local_scaling.py)."""

    _device_native = True

    def __init__(self, method: str = "standard", **kwargs):
        super().__init__(**kwargs)
        self.method = method.lower()
        if self.method not in ["ls", "standard", "nicdm"]:
            raise ValueError(f"Internal: Invalid method {self.method}. Try 'ls' or 'nicdm'.")

    def __repr__(self):
        return f"{self.__class__.__name__}(method = {self.method}, verbose = {self.verbose})"

    def _fit(self, neigh_dist, neigh_ind, source, target) -> "LocalScaling":
        self.r_dist_t_to_s_ = neigh_dist           # local_scaling.py:82
        self.r_ind_t_to_s_ = neigh_ind             # local_scaling.py:83
        d = self.ctx.as_device(neigh_dist, np.float64)
        if self.method == "nicdm":
            self._r_t_dev, _, _ = N.row_stats(self.ctx, d, mean=True)       # :143
        else:
            _, _, self._r_t_dev = N.row_stats(self.ctx, d, last=True)       # :136
        return self

    def _native_kind(self):
        return N.HUB_NICDM if self.method == "nicdm" else N.HUB_LS

    def _set_native_state(self, fitted):
        self.r_dist_t_to_s_ = fitted.state("reverse_dist")
        self.r_ind_t_to_s_ = fitted.state("reverse_ind")
        self._r_t_dev = fitted.state("state_a")

    _no_rank_reason = None

    def _rank_state(self, query_dist):
        check_is_fitted(self, "r_dist_t_to_s_")
        nicdm = self.method == "nicdm"
        r_s, _, last = N.row_stats(self.ctx, query_dist, mean=nicdm, last=not nicdm)
        return (N.RANK_NICDM, r_s, self._r_t_dev) if nicdm else (N.RANK_LS, last, self._r_t_dev)

    def transform(self, neigh_dist, neigh_ind, query=None):
        check_is_fitted(self, "r_dist_t_to_s_")
        d, i = self._device_inputs(neigh_dist, neigh_ind)
        return self._finish(N.local_scaling(self.ctx, d, i, self._r_t_dev, self.method == "nicdm"), neigh_dist, neigh_ind)


class MutualProximity(HubnessReduction):
    """Mutual proximity, 'normal' and 'empiric' (kiez/hubness_reduction/mutual_proximity.py)."""

    _device_native = True

    def __init__(self, method: str = "normal", **kwargs):
        super().__init__(**kwargs)
        if method not in ["exact", "empiric", "normal", "gaussi"]:
            raise ValueError(f'Mutual proximity method "{method}" not recognized. Try "normal" or "empiric".')
        if method in ["exact", "empiric"]:
            self.method = "empiric"
        elif method in ["normal", "gaussi"]:
            self.method = "normal"

    def __repr__(self):
        return f"{self.__class__.__name__}(method = {self.method}, verbose = {self.verbose})"

    def _fit(self, neigh_dist, neigh_ind, source, target) -> "MutualProximity":
        self.n_train = neigh_dist.shape[0]
        d = self.ctx.as_device(neigh_dist, np.float64)
        if self.method == "empiric":
            self.neigh_dist_t_to_s_ = neigh_dist       # mutual_proximity.py:95
            self.neigh_ind_t_to_s_ = neigh_ind         # :96
            self._dist_t2s_dev = d
            self._ind_t2s_dev = self.ctx.as_device(neigh_ind, np.int64)
        else:
            mu, sd = N.row_nanstats(self.ctx, d)       # :102-103 (np.nanmean / np.nanstd)
            self._mu_dev, self._sd_dev = mu, sd
            self.mu_t_to_s_ = mu
            self.sd_t_to_s_ = sd
        return self

    def _native_kind(self):
        return N.HUB_MP_EMPIRIC if self.method == "empiric" else N.HUB_MP_NORMAL

    def _set_native_state(self, fitted):
        self.n_train = fitted.info["n_target"]
        if self.method == "empiric":
            self.neigh_dist_t_to_s_ = self._dist_t2s_dev = fitted.state("reverse_dist")
            self.neigh_ind_t_to_s_ = self._ind_t2s_dev = fitted.state("reverse_ind")
        else:
            self.mu_t_to_s_ = self._mu_dev = fitted.state("state_a")
            self.sd_t_to_s_ = self._sd_dev = fitted.state("state_b")

    @property
    def _no_rank_reason(self):
        if self.method == "empiric":
            return ("MutualProximity 'empiric' counts over the members of the two candidate lists: a target row outside the list "
                    "has no value, so there is no rank over the whole index (use method='normal')")
        return None

    def _rank_state(self, query_dist):
        check_is_fitted(self, ["mu_t_to_s_", "sd_t_to_s_"])
        return N.RANK_MP_NORMAL, N.row_nanstats(self.ctx, query_dist), (self._mu_dev, self._sd_dev)

    def transform(self, neigh_dist, neigh_ind, query):
        check_is_fitted(self, ["mu_t_to_s_", "sd_t_to_s_", "neigh_dist_t_to_s_", "neigh_ind_t_to_s_"], all_or_any=any)
        d, i = self._device_inputs(neigh_dist, neigh_ind)
        out = (N.mp_normal(self.ctx, d, i, self._mu_dev, self._sd_dev) if self.method == "normal"
               else N.mp_empiric(self.ctx, d, i, self._dist_t2s_dev, self._ind_t2s_dev))
        return self._finish(out, neigh_dist, neigh_ind)


class _DualPotentials(HubnessReduction):
    """What Sinkhorn and InvertedSoftmax share: the reduced distance w_ij = (d_ij - f_i) - g_j with one soft-min potential per source
    row (f) and per target row (g) -- CSLS's 2 d - r_i - r_j with soft-min potentials over the WHOLE index in place of k-NN means.
    The state does not come from reverse neighbour lists, so `fit` runs no reverse search: it iterates `_native.softmin_rows`
    (kz_softmin_rows) between the two fitted sides.  Everything that ranks -- `kneighbors`, `kneighbors_whole_index`,
    `gold_ranks(reduced=True)`, `Kiez.match` and their device variants -- is the base class's, fed by `transform` (kz_dual_shift) and
    the whole-index kind RANK_DUAL.

    `support`: which pairs the potentials are taken over.  "index" (the default): every pair of the two sides -- each soft-min
    recomputes n_source x n_target distances.  "candidates": the pairs of the forward candidate lists only (`n_candidates` nearest
    targets per source row; kz_sinkhorn_lists / kz_softmin_list_cols): a pair outside a row's list would carry exp(-(d - m) / eps) of
    mass and is dropped, a step reads n_source x n_candidates values, and the lists stay cached for the `kneighbors` that follows --
    `fit` + `kneighbors` run ONE search.  The result is an approximation whose quality depends on `n_candidates` (on the 300 x 300
    test case at eps = 0.02: hits@1 0.803 with 10 candidates as over the whole index, 0.780 with 5; raw distance 0.723).  A target
    row that no source row lists has no potential: its `target_potential_` is NaN, and it ranks last (by row) in
    `kneighbors_whole_index` and `gold_ranks(reduced=True)`.  "union": the pairs of the forward AND the reverse candidate lists
    (`SklearnNN.neighbor_pairs(n_candidates, mode="union")`, a CSR; kz_sinkhorn_csr): every target row lists `n_candidates` sources, so
    every target row has pairs and `target_potential_` holds no NaN; a step reads at most n_source x n_candidates + n_target x
    n_candidates values, `fit` takes both directions from one shared sweep where that applies, and the forward lists stay cached for
    the `kneighbors` that follows."""

    _device_native = True
    _no_rank_reason = None
    _SUPPORTS = ("index", "candidates", "union")

    def __init__(self, temperature: float = 0.05, support: str = "index", **kwargs):
        if (isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating))
                or not np.isfinite(temperature) or temperature <= 0):
            raise ValueError(f"temperature must be a finite number > 0 (in the units of the search's distance), got {temperature!r}")
        if not isinstance(support, str) or support not in self._SUPPORTS:
            raise ValueError(f"support must be one of {self._SUPPORTS}, got {support!r}")
        super().__init__(**kwargs)
        self.temperature = float(temperature)
        self.support = support

    def _fit(self, neigh_dist, neigh_ind, source, target):
        raise NotImplementedError(f"{type(self).__name__} has no fit state in neighbour lists: `fit` iterates over the whole index")

    @abstractmethod
    def _potentials(self, source_m, target_m):
        """(f [n_s], g [n_t]) as float64 DeviceArrays from the two fitted device matrices; sets n_iter_ / potential_change_."""

    @abstractmethod
    def _potentials_pairs(self, pairs):
        """The same from a `PairList` over the source rows (float64 values): the forward candidate lists, or a CSR of pairs."""

    def fit(self, source, target=None):
        if target is None and not _is_precomputed(self.nn_algo):   # (a precomputed distance matrix IS two-sided)
            raise ValueError(f"{type(self).__name__} normalises between two sides: two-sided data only (fit(source, target))")
        if not self._gpu_nn:
            raise NotImplementedError(f"{type(self).__name__} needs the MI355X SklearnNN backend (the soft-min runs over the whole index)")
        nn = self.nn_algo
        nn.fit(source, target)
        source_m, target_m = nn._two_sided_operands(type(self).__name__)
        for attr in ("_f_dev", "_g_dev"):
            self.__dict__.pop(attr, None)
        if self.support == "candidates":
            # the forward search of kneighbors(), taken here; handed back to the backend's one-shot cache (the shared sweep's), so
            # that the kneighbors() that follows runs no second search
            dist, ind = nn.kneighbors_device(query=None, k=nn.n_candidates)
            self._f_dev, self._g_dev = self._potentials_pairs(N.PairList.lists(self.ctx, dist, ind, target_m.shape[0]))
            nn._forward = (dist.shape[1], dist, ind)
        elif self.support == "union":
            # the raw lists of BOTH directions at n_candidates (one shared sweep where it applies), their union as a CSR with the plain
            # float64 distances, rows by (value, target row): `neighbor_pairs(n_candidates, mode="union")` before its output cast.
            # Every target row lists n_candidates sources, so every column has pairs.  The forward lists go back into the one-shot cache.
            k, _ = nn._pairs_args(None, "union", type(self).__name__)
            indptr, ind, dist, fwd = nn._neighbor_pairs(k, "union", True, True, cast=False)
            self._f_dev, self._g_dev = self._potentials_pairs(N.PairList.csr(self.ctx, indptr, ind, dist, target_m.shape[0]))
            nn._forward = (fwd[0].shape[1],) + tuple(fwd)
        else:
            self._f_dev, self._g_dev = self._potentials(source_m, target_m)

    @property
    def source_potential_(self) -> np.ndarray:
        check_is_fitted(self, "_f_dev")
        return self._f_dev.numpy()

    @property
    def target_potential_(self) -> np.ndarray:
        check_is_fitted(self, "_g_dev")
        return self._g_dev.numpy()

    def _forward_rank_state(self):
        """The potentials ARE the state of both sides: no forward search."""
        check_is_fitted(self, ["_f_dev", "_g_dev"])
        return N.RANK_DUAL, self._f_dev, self._g_dev

    def transform(self, neigh_dist, neigh_ind, query=None):
        check_is_fitted(self, ["_f_dev", "_g_dev"])
        d, i = self._device_inputs(neigh_dist, neigh_ind)
        if len(d.shape) != 2 or d.shape[0] != self._f_dev.shape[0]:
            raise ValueError(f"{type(self).__name__}.transform takes the candidate lists of the fitted source rows "
                             f"({self._f_dev.shape[0]} rows), got shape {d.shape}: a potential belongs to a fitted row")
        if d.shape[0] and d.shape[1]:
            # (the native call trusts the ids, and this method takes any caller's lists: an id that is no target row would read past g)
            lo, hi = N.index_range(self.ctx, i)
            if lo < 0 or hi >= self._g_dev.shape[0]:
                raise ValueError(f"{type(self).__name__}.transform: neigh_ind holds ids in [{lo}, {hi}], the fitted target has "
                                 f"{self._g_dev.shape[0]} rows")
        return self._finish(N.dual_shift(self.ctx, d, i, self._f_dev, self._g_dev), neigh_dist, neigh_ind)


class Sinkhorn(_DualPotentials):
    """Entropic optimal transport between source and target rows (Sinkhorn iterations in the log domain), the soft form of the
    one-to-one step `Kiez.match` takes greedily.  From f = 0, `n_iter` times:
        column step  g_j = softmin_eps over i of (d_ij - f_i) + eps log(n_s / n_t)
        row step     f_i = softmin_eps over j of (d_ij - g_j)
    with softmin_eps(x) = m - eps log sum exp(-(x - m) / eps), m = min x, in float64 over the whole index.  With P_ij =
    exp(-w_ij / eps), w_ij = (d_ij - f_i) - g_j, every row of P sums to 1 after a row step and the columns approach n_s / n_t.

    `temperature`: eps > 0, in the units of the distance the search returns.  `tol`: stop after the column step whose largest change
    of g is <= tol (the row step that follows is still taken); None runs exactly `n_iter` iterations.  After `fit`:
    `source_potential_` / `target_potential_` (numpy), `n_iter_`, `potential_change_` (the last measured change of g: None after a
    single iteration).  `support="candidates"`: the same iteration with both soft-mins taken over the pairs of the forward candidate
    lists only (`_DualPotentials`): the cost of a step no longer grows with n_source x n_target, the result depends on
    `n_candidates`; `support="union"`: over the pairs of the forward and the reverse candidate lists -- no target row is left without a
    potential.  Not a name of the resolver: pass the class or an instance, `Kiez(hubness=Sinkhorn, hubness_kwargs={...})`."""

    def __init__(self, temperature: float = 0.05, n_iter: int = 10, tol: Optional[float] = None, support: str = "index", **kwargs):
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
            raise ValueError(f"n_iter must be an integer >= 1, got {n_iter!r}")
        if tol is not None and (isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0):
            raise ValueError(f"tol must be None or a number >= 0, got {tol!r}")
        super().__init__(temperature=temperature, support=support, **kwargs)
        self.n_iter = int(n_iter)
        self.tol = None if tol is None else float(tol)

    def __repr__(self):
        return (f"{self.__class__.__name__}(temperature = {self.temperature}, n_iter = {self.n_iter}, tol = {self.tol}, "
                f"support = {self.support})")

    def _potentials_pairs(self, pairs):
        """The same iteration over the pairs of the list, in one native call (`PairList.sinkhorn`: the stop is decided on the device)."""
        f, g, self.n_iter_, self.potential_change_ = pairs.sinkhorn(self.temperature, self.n_iter, self.tol)
        return f, g

    def _potentials(self, source_m, target_m):
        ctx, eps = self.ctx, self.temperature
        shift = eps * float(np.log(source_m.shape[0] / target_m.shape[0]))
        f = g = None
        self.potential_change_ = None
        for it in range(1, self.n_iter + 1):
            # column step: the same call with target as query and source as index (f = 0 at first: no offset)
            g_new = N.softmin_rows(ctx, target_m, source_m, eps, off=f, shift=shift)
            if g is not None:
                self.potential_change_ = N.max_abs_diff(ctx, g_new, g)
            g = g_new
            f = N.softmin_rows(ctx, source_m, target_m, eps, off=g)
            self.n_iter_ = it
            if self.tol is not None and self.potential_change_ is not None and self.potential_change_ <= self.tol:
                break
        return f, g


class InvertedSoftmax(_DualPotentials):
    """The inverted softmax (Smith et al. 2017): the target-side state is a log-sum-exp over ALL source rows -- one Sinkhorn column
    step from f = 0 with the constant left out, g_j = softmin_eps over i of d_ij, and f stays 0: the lists are ranked by d_ij - g_j.
    `temperature`: eps > 0, in the units of the distance the search returns.  `support="candidates"`: the log-sum-exp runs over the
    source rows that list the target among their `n_candidates` nearest only (`_DualPotentials`); a target nobody lists gets NaN.
    `support="union"`: over those and the target's own `n_candidates` nearest source rows: every target has a value.
    Not a name of the resolver: pass the class or an instance."""

    def __repr__(self):
        return f"{self.__class__.__name__}(temperature = {self.temperature}, support = {self.support})"

    def _potentials(self, source_m, target_m):
        self.n_iter_, self.potential_change_ = 1, None
        g = N.softmin_rows(self.ctx, target_m, source_m, self.temperature)
        return self.ctx.to_device(np.zeros(source_m.shape[0], dtype=np.float64)), g

    def _potentials_pairs(self, pairs):
        """One column step over the transposed view of the pairs, without offset or constant."""
        self.n_iter_, self.potential_change_ = 1, None
        g = N.softmin_list_cols(self.ctx, pairs.transpose(), self.temperature)
        return self.ctx.to_device(np.zeros(pairs.n_q, dtype=np.float64)), g


_DESIRED_P_VALUE = 2


class DisSimLocal(HubnessReduction):
    """DisSimLocal (kiez/hubness_reduction/dis_sim.py)."""

    _device_native = True

    def __init__(self, squared: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.squared = squared
        if self.nn_algo.metric in ["euclidean", "minkowski"]:
            self.squared = False
            if hasattr(self.nn_algo, "p") and self.nn_algo.p != _DESIRED_P_VALUE:
                raise ValueError(
                    "DisSimLocal only supports squared Euclidean distances. If the provided NNAlgorithm has a `p` "
                    f"parameter it must be set to p=2. Now it is p={self.nn_algo.p}")
        elif self.nn_algo.metric in ["sqeuclidean"]:
            self.squared = True
        else:
            raise ValueError(f"DisSimLocal only supports squared Euclidean distances, not metric={self.nn_algo.metric}.")

    def __repr__(self):
        return f"{self.__class__.__name__}(squared = {self.squared})"

    def _matrices(self, source, target):
        """Device matrices of the embeddings (reused from the NN backend when it is the GPU one)."""
        nn = self.nn_algo
        if self._gpu_nn and hasattr(nn, "source_index"):
            return nn._matrix_for(source), nn._matrix_for(target)
        s = np.asarray(source)
        t = np.asarray(target)
        if s.dtype != t.dtype or s.dtype not in (np.float32, np.float64):
            s, t = s.astype(np.float64), t.astype(np.float64)
        sm = N.DeviceMatrix(self.ctx, s, "sqeuclidean")
        tm = sm if target is source else N.DeviceMatrix(self.ctx, t, "sqeuclidean")
        return sm, tm

    def _fit(self, neigh_dist, neigh_ind, source, target) -> "DisSimLocal":
        sm, tm = self._matrices(source, target)
        t2c = N.dsl_fit(self.ctx, self.ctx.as_device(neigh_ind, np.int64), sm, tm)
        self.source_ = source
        self.target_ = target
        self._source_m, self._target_m = sm, tm
        self.target_dist_to_centroids_ = t2c       # dis_sim.py:107 (device array; .numpy() gives the reference's values)
        self.target_centroids_ = None              # not needed by transform; the reference only stores it
        return self

    def transform(self, neigh_dist, neigh_ind, query):
        check_is_fitted(self, ["target_", "target_dist_to_centroids_"])
        ctx = self.ctx
        i = ctx.as_device(neigh_ind, np.int64)
        tm = self._target_m
        if query is self.source_:
            qm = self._source_m
        elif self._gpu_nn:
            qm = self.nn_algo._matrix_for(query)
            tm = self.nn_algo._partner(qm, self._target_m)   # (2-byte target rows and a query of another type: the float64 pair)
        else:
            qm = N.DeviceMatrix(ctx, np.asarray(query, dtype=self._target_m.dtype), "sqeuclidean")
        gmin = ctx.to_device(np.array([np.inf], dtype=np.float64))
        out = N.dsl_transform(ctx, i, qm, 0, tm, self.target_dist_to_centroids_, gmin)
        return self._finish(N.dsl_finalize(ctx, out, float(self._reduce_min(gmin.numpy()[0])), bool(self.squared)), neigh_dist, neigh_ind)

    _no_rank_reason = ("DisSimLocal's values come from its own gather of the embeddings around the candidate list's centroid, not from "
                       "the search's distances: a target row outside the list has no value, so there is no rank over the whole index")

    def _reduce_min(self, local_min: float) -> float:
        """Hook for the multi-GPU path: the shift uses the GLOBAL minimum (dis_sim.py:171-173)."""
        return local_min
