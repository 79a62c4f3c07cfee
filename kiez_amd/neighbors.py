"""NN backends: the reference's `NNAlgorithm` plugin interface and the MI355X exact backend behind it.

`NNAlgorithm` mirrors kiez/neighbors/neighbor_algorithm_base.py:13-136 (same method names, argument
meaning, errors and warnings).  `SklearnNN` keeps the reference class's name and constructor
(kiez/neighbors/exact/sklearn_nearest_neighbors.py:51-65) so that `Kiez(algorithm="SklearnNN", ...)`
configurations keep working, but `_fit` / `_kneighbors` run on the GPU through the C ABI
(include/kiez_amd.h): brute-force exact search, identical neighbours.
"""
from __future__ import annotations

import warnings
from abc import ABC, abstractmethod
from typing import Any, Optional, Tuple

import numpy as np

from . import _native as N


class NotFittedError(ValueError, AttributeError):
    """Same bases as sklearn.exceptions.NotFittedError (raised by the reference through check_is_fitted)."""


def check_is_fitted(obj, attributes, all_or_any=all):
    if isinstance(attributes, str):
        attributes = [attributes]
    if not all_or_any([hasattr(obj, a) for a in attributes]):
        raise NotFittedError(
            f"This {type(obj).__name__} instance is not fitted yet. Call 'fit' with appropriate arguments before "
            "using this estimator.")


class NNAlgorithm(ABC):
    """The reference's plugin interface for nearest-neighbour backends (kiez/neighbors/neighbor_algorithm_base.py:13-136).

    A backend implements `_fit(data, is_source) -> index` and `_kneighbors(k, query, index, return_distance,
    is_self_querying)`; this base class keeps the two fitted sides and does the argument checking.  Attributes after `fit`
    are the reference's: `source_`, `target_` (the caller's arrays), `source_index`, `target_index`,
    `source_equals_target`.  Organisation is this repository's own: one table of the two search directions
    (`_direction`) instead of branches, checks as small helpers.
    """

    _ALLOWED_INPUT_TYPES: Tuple[Any, ...] = (np.ndarray,)

    def __init__(self, n_candidates, metric, n_jobs):
        self.n_candidates = n_candidates
        self.metric = metric
        self.n_jobs = n_jobs

    # ---- what a backend provides --------------------------------------------------------------------
    @property
    @abstractmethod
    def valid_metrics(self):
        pass  # pragma: no cover

    @abstractmethod
    def _fit(self, data, is_source: bool) -> Any:
        pass  # pragma: no cover

    @abstractmethod
    def _kneighbors(self, k, query, index, return_distance, is_self_querying):
        pass  # pragma: no cover

    # ---- checks -------------------------------------------------------------------------------------
    def _check_input_types(self, value):
        values = value if isinstance(value, tuple) else (value,)
        allowed = type(self)._ALLOWED_INPUT_TYPES
        if any(x is not None and not isinstance(x, allowed) for x in values):
            found_types = [type(x) for x in values]
            raise ValueError(f"Not implemented for input type(s) {found_types}! Only {allowed} allowed!")

    @staticmethod
    def _same_width(source, target):
        if source.shape[1] != target.shape[1]:
            raise ValueError("Expected source and target to have the same number of features,"
                             f" but got source.shape: {source.shape} and target.shape: {target.shape}")

    def _check_k_value(self, k: int, needed_space) -> int:
        if not np.issubdtype(type(k), np.integer):
            raise TypeError(f"k does not take {type(k)} value, enter integer value")
        if k <= 0:
            raise ValueError(f"Expected k > 0. Got {k}")
        if k <= needed_space:
            return k
        warnings.warn(f"k={k} is larger than number of samples in indexed space.\n" + f"Setting to k={needed_space}",
                      stacklevel=2)
        return needed_space

    def _describe_source_target_fitted(self):
        if not hasattr(self, "source_"):
            return " is unfitted"
        return f" is fitted with: source.shape={self.source_.shape} and target.shape={self.target_.shape}"

    # ---- fit ----------------------------------------------------------------------------------------
    def fit(self, source, target=None, only_fit_target: bool = False):
        """Index the data.  One argument: a single-source search (the index serves both directions).  Two arguments: both
        sides are indexed, or only the target when the caller never searches target -> source (`only_fit_target`, used by
        NoHubnessReduction).  An index that this call does not rebuild is dropped, never left over from an earlier fit."""
        self._check_input_types((source, target))
        single = target is None
        if not single:
            self._same_width(source, target)
        for stale in ("source_index", "target_index"):
            if hasattr(self, stale):
                delattr(self, stale)
        if single:
            self.source_index = self.target_index = self._fit(source, True)
            target = source
        elif only_fit_target:
            self.target_index = self._fit(target, True)
        else:
            self.source_index = self._fit(source, True)
            self.target_index = self._fit(target, False)
        self.source_equals_target = single
        self.source_, self.target_ = source, target

    # ---- search -------------------------------------------------------------------------------------
    def _direction(self, s_to_t: bool):
        """(default query array, index searched, its size) of a search direction."""
        if s_to_t:
            return self.source_, getattr(self, "target_index", None), self.target_.shape[0]
        return self.target_, getattr(self, "source_index", None), self.source_.shape[0]

    def _select_direction(self, k, query, s_to_t):
        check_is_fitted(self, ["source_index", "target_index"], all_or_any=any)
        default_query, index, index_size = self._direction(s_to_t)
        if index is None:   # e.g. target -> source after fit(..., only_fit_target=True)
            raise NotFittedError(f"'{type(self).__name__}' object has no attribute "
                                 f"'{'target_index' if s_to_t else 'source_index'}'")
        # only the implicit query of a single-source fit searches "itself" (the explicit reverse pass of
        # HubnessReduction.fit keeps each row as its own first neighbour, base.py:37-42)
        is_self_querying = query is None and self.source_equals_target
        k = self._check_k_value(self.n_candidates if k is None else k, index_size)
        return k, (default_query if query is None else query), index, is_self_querying

    def kneighbors(self, k=None, query=None, s_to_t=True, return_distance=True):
        """k nearest neighbours of `query` (default: the fitted source, or target when `s_to_t` is False)."""
        k, query, index, is_self_querying = self._select_direction(k, query, s_to_t)
        return self._kneighbors(k=k, query=query, index=index, return_distance=return_distance,
                                is_self_querying=is_self_querying)


def _torch_if_loaded():
    """torch, but only if the caller already imported it (this package never imports torch on its own: the HIP runtime
    bundled with torch has to be loaded BEFORE libkiez_amd.so, kiez_amd/_native.py)."""
    import sys
    return sys.modules.get("torch")


def _is_tensor(x) -> bool:
    t = _torch_if_loaded()
    return t is not None and isinstance(x, t.Tensor)


def canonical_metric(metric: str, p=2) -> str:
    """Map the reference's metric spelling to one the HIP kernels implement; anything else fails loudly.

    scikit-learn's own aliases (sklearn/metrics/_dist_metrics.pyx.tp, DistanceMetric.get_metric): minkowski with p = 1 / 2 / inf IS
    manhattan / euclidean / chebyshev; `p` is ignored for every other metric name.  Euclidean, squared euclidean and cosine run the
    fused MFMA kernels; manhattan, chebyshev and minkowski(p) have no inner-product form and run on a register-tiled VALU kernel + the exact selection,
    as do braycurtis, seuclidean, correlation and hamming (scikit-learn's brute-force expressions, bit for bit).  The seven boolean
    metrics (jaccard, dice, rogerstanimoto, russellrao, sokalmichener, sokalsneath, yule: scipy's cdist on x != 0) run a popcount
    kernel on bit-packed rows + the exact selection.  'precomputed' (scikit-learn's spelling) takes a distance matrix in place of
    embeddings: no distance arithmetic at all, the exact selection on the matrix' own values."""
    if metric == "minkowski":
        if not isinstance(p, (int, float, np.integer, np.floating)) or isinstance(p, bool) or not p >= 1:
            raise ValueError(f"metric='minkowski' needs p >= 1 on the MI355X exact backend (got p={p!r})")
        if p == 2:
            return "euclidean"
        if p == 1:
            return "manhattan"
        if np.isinf(p):
            return "chebyshev"
        if p >= 1e6:    # (kz_matrix_set_minkowski_p's limit: said here, in the constructor, like every other metric error)
            raise ValueError(f"metric='minkowski' with p={p!r}: the MI355X exact backend takes 1 <= p < 1e6 (or p = inf: chebyshev)")
        return f"minkowski[{float(p)!r}]"
    if metric in ("l2", "euclidean"):
        return "euclidean"
    if metric in ("manhattan", "cityblock", "l1"):
        return "manhattan"
    if metric in ("sqeuclidean", "cosine", "chebyshev", "braycurtis", "seuclidean", "correlation", "hamming", "precomputed") or metric in N.BOOLEAN_METRICS:
        return metric
    raise ValueError(
        f"metric='{metric}' is not implemented by the MI355X exact backend; valid metrics: {SklearnNN.valid_metrics}")


class _ColumnsSide:
    """The target side of a fitted precomputed DeviceArray D [n_source, n_target]: `target_` of the backend, a distinct object so that
    `query=target_` resolves to the matrix' columns view (numpy arrays and tensors use their own transposed view, `D.T`)."""

    def __init__(self, matrix):
        self.matrix = matrix
        self.shape = (matrix.shape[1], matrix.shape[0])
        self.dtype = matrix.dtype


def seuclidean_V(metric_c: str, metric_params):
    """The variances V of metric 'seuclidean' from `metric_params` ({"V": array_like}, scikit-learn's spelling) as a float64 vector;
    None for every other metric."""
    if metric_c != "seuclidean":
        return None
    if not metric_params:
        # (scikit-learn raises TypeError at the first search, when it builds SEuclideanDistance without V; here at once)
        raise TypeError("metric='seuclidean' needs metric_params={'V': array_like of length n_features}")
    if not isinstance(metric_params, dict) or set(metric_params) != {"V"}:
        raise NotImplementedError(f"metric_params={metric_params!r} is not implemented by the MI355X exact backend "
                                  "(only metric='seuclidean' with metric_params={'V': array_like})")
    V = np.asarray(metric_params["V"], dtype=np.float64)
    if V.ndim != 1:
        raise ValueError(f"metric_params['V'] must be one-dimensional, got shape {V.shape}")
    if not (np.all(np.isfinite(V)) and np.all(V > 0)):
        # (scikit-learn divides by whatever V holds; here every variance must be finite and > 0)
        raise ValueError("metric_params['V']: every variance must be finite and > 0 on the MI355X exact backend")
    return np.ascontiguousarray(V)


class SklearnNN(NNAlgorithm):
    """Exact brute-force nearest neighbours on MI355X, under the reference class's name and signature
    (kiez/neighbors/exact/sklearn_nearest_neighbors.py:7-101).

    `algorithm`, `leaf_size` and `n_jobs` are accepted for configuration compatibility; every sklearn
    algorithm choice is exact, so the neighbours are the same and the search always runs as one fused
    distance + top-k pass on the GPU.
    """

    valid_metrics = ["braycurtis", "chebyshev", "cityblock", "correlation", "cosine", "dice", "euclidean", "hamming", "jaccard", "l1",
                     "l2", "manhattan", "minkowski", "precomputed", "rogerstanimoto", "russellrao", "seuclidean", "sokalmichener",
                     "sokalsneath", "sqeuclidean", "yule"]
    # numpy arrays as in the reference; additionally arrays already resident in HBM (zero-copy fit)
    _ALLOWED_INPUT_TYPES = (np.ndarray, N.DeviceArray)

    def __init__(self, n_candidates=5, algorithm="auto", leaf_size=30, metric="minkowski", p=2, metric_params=None,
                 n_jobs=None, device=None):
        super().__init__(n_candidates=n_candidates, metric=metric, n_jobs=n_jobs)
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.p = p
        self.metric_params = metric_params
        self.device = device
        self._metric_c = canonical_metric(metric, p)
        if metric_params and self._metric_c != "seuclidean":
            raise NotImplementedError(f"metric_params={metric_params!r} is not implemented by the MI355X exact backend "
                                      "(only metric='seuclidean' with metric_params={'V': array_like})")
        self._V = seuclidean_V(self._metric_c, metric_params)   # seuclidean: the per-feature variances, float64
        if isinstance(n_candidates, (int, np.integer)) and n_candidates > N.MAX_NEIGHBORS - 1:
            raise NotImplementedError(f"n_candidates={n_candidates} exceeds the {N.MAX_NEIGHBORS - 1} neighbours per query the "
                                      "MI355X exact backend supports")
        self._ctx = None
        self._aux = None  # (array, DeviceMatrix) of the most recent query array that is not a fitted side
        self._wide = {}   # id(index matrix of 2-byte rows) -> (that matrix, its float64 copy): built when an ad-hoc query of another
                          # element type arrives (`_partner`), kept beside _aux, dropped by the next fit
        self._forward = None  # (k, dist, ind): source -> target result that came out of a shared sweep (kneighbors_device_both)
        self.last_stats = None
        self.last_stats_reverse = None   # statistics of the target -> source direction of the last shared sweep (else None)

    def __repr__(self):
        return (f"{self.__class__.__name__}(n_candidates={self.n_candidates},algorithm={self.algorithm},"
                f"leaf_size={self.leaf_size},metric={self.metric},n_jobs={self.n_jobs} )")

    # ---- device plumbing ---------------------------------------------------------------------------
    @property
    def ctx(self) -> N.Context:
        if self._ctx is None:
            self._ctx = N.Context.get(self.device)
        return self._ctx

    def _storage(self, elem: str) -> str:
        """The element type rows of dtype name `elem` are stored as under this backend's metric (`_native.row_storage`): float32 /
        float64 as they are; float16 / bfloat16 as they are for euclidean, sqeuclidean and cosine (minkowski p = 2 IS euclidean);
        anything else widened -- float32 for the boolean metrics (they read x != 0 only: half the bytes, a nonzero value stays
        nonzero), else float64.  No device is touched."""
        return N.row_storage(self._metric_c, elem)

    def _prepare(self, data, elem: Optional[str] = None) -> np.ndarray:
        """`data` as a contiguous 2-D array of its storage type, or of `elem` ('float32' / 'float64') where one is asked for."""
        arr = np.asarray(data)
        if arr.ndim != 2:
            raise ValueError(f"Expected 2D array, got {arr.ndim}D array instead")
        store = elem if elem is not None else self._storage(arr.dtype.name)
        if arr.dtype.name != store:
            arr = arr.astype(store)
        return np.ascontiguousarray(arr)

    def _check_input_types(self, value):
        # torch tensors are accepted like the reference's Faiss backend does (kiez/neighbors/approximate/faiss.py:64-65):
        # CUDA tensors are consumed in place (zero-copy fit), CPU tensors through their numpy view
        if not isinstance(value, tuple):
            value = (value,)
        super()._check_input_types(tuple(None if _is_tensor(x) else x for x in value))

    def _check_V(self, shape):
        if self._V is not None and self._V.shape[0] != shape[1]:
            raise ValueError(f"metric_params['V'] has {self._V.shape[0]} entries, the data {shape[1]} features")

    def _make_matrix(self, data, elem: Optional[str] = None) -> N.DeviceMatrix:
        """The device matrix of `data` in its storage type (`_storage`), or in `elem` ('float32' / 'float64': the element type of the
        index an ad-hoc query is searched against) -- a query is widened, never narrowed."""
        if _is_tensor(data):
            torch = _torch_if_loaded()
            t = data.detach()
            if t.dim() != 2:
                raise ValueError(f"Expected 2D array, got {t.dim()}D array instead")
            store = elem if elem is not None else self._storage(str(t.dtype).replace("torch.", ""))
            if str(t.dtype).replace("torch.", "") != store:
                t = t.to(getattr(torch, store))
            if not t.is_cuda:
                t = t.contiguous()
                if store == "bfloat16":   # (numpy has no bfloat16: the rows go up as their 16-bit patterns)
                    self._check_V(tuple(t.shape))
                    return N.DeviceMatrix(self.ctx, t.view(torch.int16).numpy().view(np.uint16), self._metric_c, V=self._V, elem="bfloat16")
                return self._make_matrix(t.numpy(), store)
            t = t.contiguous()
            if t.device.index != self.ctx.device:
                raise ValueError(f"tensor lives on cuda:{t.device.index}, the NN backend on device {self.ctx.device}")
            self._check_V(tuple(t.shape))
            torch.cuda.current_stream(t.device).synchronize()   # the producer stream is not ours
            # zero-copy: the matrix reads the tensor's HBM in place and keeps it alive (the reference, too, only keeps
            # references to its inputs, neighbor_algorithm_base.py:95-96: they must not be modified while fitted)
            return N.DeviceMatrix(self.ctx, None, self._metric_c, device_ptr=t.data_ptr(), shape=tuple(t.shape), elem=store, borrow=True,
                                  keepalive=t, V=self._V)
        if isinstance(data, N.DeviceArray):
            half_ok = data.dtype == np.float16 and N.half_rows_supported(self._metric_c)
            if len(data.shape) != 2 or not (data.dtype in (np.float32, np.float64) or half_ok):
                raise ValueError("device inputs must be 2D float32/float64 arrays" +
                                 (" (float16 too for euclidean, sqeuclidean and cosine)" if data.dtype == np.float16 else ""))
            if elem is not None and data.dtype.name != elem:
                raise ValueError(f"device input has dtype {data.dtype}, the index has {elem}")
            self._check_V(data.shape)
            return N.DeviceMatrix(self.ctx, None, self._metric_c, device_ptr=data.ptr.value, shape=data.shape,
                                  dtype=data.dtype, borrow=True, keepalive=data, V=self._V)
        arr = self._prepare(data, elem)
        self._check_V(arr.shape)
        return N.DeviceMatrix(self.ctx, arr, self._metric_c, V=self._V)

    def _fit(self, data, is_source: bool):
        """Replaces SklearnNN._fit (sklearn_nearest_neighbors.py:83-94): upload + norms + MFMA tile packing."""
        self._aux = None
        self._wide = {}
        self._forward = None
        self.last_stats_reverse = None
        if self._half_as_float64 and self._storage(self._elem_name(data)) in N.HALF_ELEMS:
            # (the other side of this fit has another element type: `fit`)
            return self._make_matrix(data.numpy() if isinstance(data, N.DeviceArray) else data, elem="float64")
        return self._make_matrix(data)

    def _make_precomputed(self, data):
        """The two views (rows, columns) of a distance matrix [n_source, n_target]: numpy arrays are copied into HBM, DeviceArrays and
        CUDA tensors are read in place (a non-contiguous tensor through a contiguous copy).  float32 / float64 pass through, any other
        dtype is cast to float64, as `_prepare` does for embeddings."""
        if _is_tensor(data):
            torch = _torch_if_loaded()
            t = data.detach()
            if t.dim() != 2:
                raise ValueError(f"Expected 2D array, got {t.dim()}D array instead")
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
            if not t.is_cuda:
                return self._make_precomputed(t.contiguous().numpy())
            t = t.contiguous()
            if t.device.index != self.ctx.device:
                raise ValueError(f"tensor lives on cuda:{t.device.index}, the NN backend on device {self.ctx.device}")
            torch.cuda.current_stream(t.device).synchronize()   # the producer stream is not ours
            return N.DeviceMatrix.precomputed(self.ctx, None, device_ptr=t.data_ptr(), shape=tuple(t.shape),
                                              dtype=np.float32 if t.dtype == torch.float32 else np.float64, borrow=True, keepalive=t)
        if isinstance(data, N.DeviceArray):
            if len(data.shape) != 2 or data.dtype not in (np.float32, np.float64):
                raise ValueError("device inputs must be 2D float32/float64 arrays")
            return N.DeviceMatrix.precomputed(self.ctx, None, device_ptr=data.ptr.value, shape=data.shape, dtype=data.dtype,
                                              borrow=True, keepalive=data)
        return N.DeviceMatrix.precomputed(self.ctx, self._prepare(data))

    def _fit_precomputed(self, matrix, target):
        """metric='precomputed': ONE matrix D [n_source, n_target], D[i, j] = the distance from source row i to target row j.
        `source_index` / `target_index` are its rows view and its columns view; `target_` is a distinct object (the transposed view,
        never materialised) so that a search with `query=target_` resolves to the columns view, not to `source_index`."""
        if target is not None:
            raise ValueError("metric='precomputed' takes ONE distance matrix [n_source, n_target]: fit(D), not fit(source, target)")
        self._check_input_types((matrix,))
        for stale in ("source_index", "target_index"):
            if hasattr(self, stale):
                delattr(self, stale)
        self._aux = None
        self._wide = {}
        self._forward = None
        self.last_stats_reverse = None
        self.source_index, self.target_index = self._make_precomputed(matrix)
        self.source_equals_target = False
        if isinstance(matrix, N.DeviceArray):
            columns = _ColumnsSide(matrix)
        else:
            columns = matrix.t() if _is_tensor(matrix) else np.asarray(matrix).T
        self.source_, self.target_ = matrix, columns

    def fit(self, source, target=None, only_fit_target: bool = False):
        if self._metric_c == "precomputed":
            return self._fit_precomputed(source, target)
        self._check_input_types((source, target))
        if (isinstance(source, np.ndarray) and isinstance(target, np.ndarray) and source.ndim == 2 and target.ndim == 2
                and source.shape[1] == target.shape[1] and source.dtype != target.dtype):
            # one dtype for both sides (sklearn dispatches on X.dtype == Y.dtype, _dispatcher.py:292): use float64
            super().fit(np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64), only_fit_target)
            self.source_, self.target_ = source, target  # keep the caller's arrays, as the reference does
            return
        # Tensors and DeviceArrays of two element types, one of them float16 / bfloat16: a 2-byte side is read in place only beside a
        # side of its own type -- beside any other it is widened to float64, as every dtype other than float32 / float64 is (two
        # half types: both to float64; the other side keeps its type, and float32 beside float64 is refused by the search as ever)
        if target is not None:
            es, et = self._storage(self._elem_name(source)), self._storage(self._elem_name(target))
            self._half_as_float64 = es != et and (es in N.HALF_ELEMS or et in N.HALF_ELEMS)
        try:
            super().fit(source, target, only_fit_target)
        finally:
            self._half_as_float64 = False

    _half_as_float64 = False   # set by `fit` around the `_fit` calls of a two-sided fit on mixed element types

    @staticmethod
    def _elem_name(x) -> str:
        """dtype name ('float16', 'bfloat16', 'int64', ...) of a numpy array, DeviceArray or tensor."""
        if _is_tensor(x):
            return str(x.dtype).replace("torch.", "")
        return (x.dtype if isinstance(x, N.DeviceArray) else np.asarray(x).dtype).name

    def _matrix_for(self, array) -> N.DeviceMatrix:
        """Device matrix of a query array: the index of a fitted side if it IS that side's array, else an upload.  The most
        recent ad-hoc query is kept (a hubness transform asks for the same array right after the search) and replaced by
        the next one: nothing accumulates, and a new fit drops it."""
        if hasattr(self, "source_index") and array is self.source_:
            return self.source_index
        if hasattr(self, "target_index") and array is self.target_:
            return self.target_index
        if self._metric_c == "precomputed":
            # (a distance matrix answers for its own rows and columns only: there are no embeddings to measure a new row against)
            raise NotImplementedError("metric='precomputed': `query` must be a fitted side (the fitted matrix: its rows; `target_`: its "
                                      "columns) -- distances from new rows are not in the matrix; fit the extended matrix instead")
        if self._aux is not None and self._aux[0] is array:
            return self._aux[1]
        self._check_input_types(array)
        ref = self.target_index if hasattr(self, "target_index") else self.source_index
        want, have = ref.elem, self._elem_name(array)
        if want in N.HALF_ELEMS:
            # an index of 2-byte rows: a query of the same type goes up as it is; any other is widened to float64 and searched
            # against the float64 copy of the index (`_partner`) -- a query is never narrowed
            want = None if have == want else "float64"
        # (a float16 DeviceArray beside an index of another type: widened through the host -- the device has no copy to borrow)
        rows = array.numpy() if isinstance(array, N.DeviceArray) and want is not None and have == "float16" != want else array
        m = self._make_matrix(rows, elem=want)
        self._aux = (array, m)
        return m

    def _partner(self, qm: N.DeviceMatrix, index: N.DeviceMatrix) -> N.DeviceMatrix:
        """The matrix `qm` is searched against: `index` itself, or -- an index of 2-byte rows and a query matrix of another element
        type (`_matrix_for` has widened it to float64) -- the float64 copy of the index's rows, made once from the fitted array."""
        if qm.elem == index.elem or index.elem not in N.HALF_ELEMS:
            return index
        hit = self._wide.get(id(index))
        if hit is None:
            side = self.target_ if index is getattr(self, "target_index", None) else self.source_
            hit = (index, self._make_matrix(side, elem="float64"))
            self._wide[id(index)] = hit
        return hit[1]

    def _out_dtype(self, index: N.DeviceMatrix):
        # sklearn: euclidean family -> float64 always (ArgKmin); cosine -> dtype of the input; precomputed -> dtype of the matrix
        return np.float32 if (self._metric_c in ("cosine", "precomputed") and index.dtype == np.float32) else np.float64

    def kneighbors_device(self, k=None, query=None, s_to_t=True, q_begin=0, q_count=None):
        """`kneighbors` that leaves (dist float64, ind int64) in HBM; used by the GPU hubness reductions."""
        default_query = query is None
        k, query, index, is_self_querying = self._select_direction(k, query, s_to_t)
        if default_query and s_to_t and self._forward is not None:
            # the forward result of the shared sweep (kneighbors_device_both): handed out once, then dropped -- also when this
            # call asks for something else (another k, a row range): the cached [n_s, k] arrays must not stay pinned in HBM
            fk, dist, ind = self._forward
            self._forward = None
            if fk == k and q_begin == 0 and q_count is None:
                return dist, ind
            del dist, ind
        qm = self._matrix_for(query)
        index = self._partner(qm, index)
        dist, ind, stats = N.knn(self.ctx, qm, index, k, exclude_self=is_self_querying, q_begin=q_begin, q_count=q_count)
        self.last_stats = stats
        return dist, ind

    def _two_sided_operands(self, what, s_to_t=True):
        """(query matrix, index matrix) of a call that ranks every index row for every query row (`what`: `gold_ranks`,
        `kneighbors_whole_index`), after the checks they share."""
        check_is_fitted(self, ["source_index", "target_index"], all_or_any=any)
        if self.source_equals_target:
            raise NotImplementedError(f"{what} needs a two-sided fit (fit(source, target)): sklearn's self-removal rule of a "
                                      "single-source search has no meaning for a rank")
        query, index, _ = self._direction(s_to_t)
        if index is None:   # e.g. target -> source after fit(..., only_fit_target=True)
            raise NotFittedError(f"'{type(self).__name__}' object has no attribute "
                                 f"'{'target_index' if s_to_t else 'source_index'}'")
        qm = self._matrix_for(query)
        return qm, self._partner(qm, index)

    def _gold_rank_operands(self, gold, s_to_t=True):
        """(query matrix, index matrix, gold ids int64 on the device) of a `gold_ranks` call, after its checks."""
        from .evaluate import _gold_rows

        query, index = self._two_sided_operands("gold_ranks", s_to_t)
        return query, index, self.ctx.to_device(_gold_rows(gold, query.shape[0]))

    def gold_ranks_device(self, gold, s_to_t=True) -> N.DeviceArray:
        """`gold_ranks` that leaves the int64 rank vector in HBM (evaluate.rank_metrics reduces it there)."""
        query, index, gold_dev = self._gold_rank_operands(gold, s_to_t)
        return N.gold_ranks(self.ctx, query, index, gold_dev)

    def gold_ranks(self, gold, s_to_t=True) -> np.ndarray:
        """Exact 0-based rank of every query row's gold answer against the WHOLE index: the position the gold row would hold in
        `kneighbors(k = index size)` -- without that list, so for an index of any size (a search returns at most
        `_native.MAX_NEIGHBORS` neighbours).  Query rows are the fitted source rows and the index the fitted target; with
        `s_to_t=False` the target rows are ranked against the indexed source.

        `gold`: the dict `evaluate.hits` takes ({query row: index row}), or an int64 array with one gold id per query row, -1 for
        none.  Returns a numpy int64 vector: -1 where a row has no gold id (or one that is no index row), else the rank.

        These are ranks under the SEARCH METRIC.  The ranks under the hubness-reduced distances -- what MRR / hits@k after CSLS,
        LocalScaling, NICDM or MutualProximity 'normal' are computed from -- come from `Kiez.gold_ranks(gold, reduced=True)`
        (`HubnessReduction.gold_ranks`): those reductions are functions of a pair's distance and one state per side, defined for
        every index row and not for the candidate list alone.  Raises NotFittedError before `fit` and NotImplementedError after a
        single-source fit (`fit(source)`): sklearn's self-removal rule has no meaning for a rank.  `evaluate.rank_metrics` turns the
        ranks into hits@k, MR and MRR."""
        return self.gold_ranks_device(gold, s_to_t).numpy()

    # ---- every pair within a threshold, whole index ---------------------------------------------------
    def _results_to_host(self, *arrays):
        """Device results as `kneighbors` hands them out: tensors on the source's device after a fit on tensors, else numpy."""
        src = self.source_
        if _is_tensor(src):
            torch = _torch_if_loaded()
            self.ctx.sync()
            out = tuple(torch.as_tensor(a, device="cuda").clone().to(src.device) if a.nbytes else
                        torch.empty(a.shape, dtype=getattr(torch, a.dtype.name), device=src.device) for a in arrays)
            torch.cuda.current_stream().synchronize()   # before the arrays go back to our stream-ordered pool
            return out
        return tuple(a.numpy() for a in arrays)

    def _radius_distances(self, dist: N.DeviceArray, index: N.DeviceMatrix) -> N.DeviceArray:
        """The float64 values of a radius call in the dtype `kneighbors` returns (the cast comes AFTER the predicate)."""
        if self._out_dtype(index) == np.float32:
            return N.cast_f32(self.ctx, dist) if dist.shape[0] else self.ctx.empty((0,), np.float32)
        return dist

    def radius_neighbors_device(self, radius, s_to_t=True, sort_results=True):
        """`radius_neighbors` with the CSR left in HBM: (indptr int64 [n_query + 1], ind int64 [total], dist [total]) DeviceArrays."""
        radius = N.radius_value(radius)
        query, index = self._two_sided_operands("radius_neighbors", s_to_t)
        indptr, ind, dist, _ = N.radius_neighbors(self.ctx, query, index, radius, sort_results=sort_results)
        return indptr, ind, self._radius_distances(dist, self._direction(s_to_t)[1])

    def radius_neighbors(self, radius, s_to_t=True, return_distance=True, sort_results=True):
        """Every index row within `radius` of every query row under the search metric, over the whole index: the other half of
        scikit-learn's `NearestNeighbors`.  Query rows are the fitted source rows and the index the fitted target (`s_to_t=False`:
        the reverse).  Pair (i, j) is in the result exactly when d_ij <= radius, d the float64 distance `kneighbors` computes for
        the pair; a NaN distance (correlation against a constant row) is never in it.  `radius` is a real number; infinities are
        legal, NaN raises ValueError and a bool TypeError.

        Returns the CSR `(indptr, ind, dist)` -- `ind[indptr[i]:indptr[i + 1]]` are the index rows of query row i, ascending by
        (distance, index row), or by index row with `sort_results=False` -- or `(indptr, ind)` with `return_distance=False`; numpy
        arrays, or tensors when fitted on tensors.  `dist` has the dtype `kneighbors` returns: for float32 cosine / precomputed
        input it is the float64 distance rounded to float32 AFTER the comparison, so a returned value may round to just above
        `radius`.  Memory is the result's, not n_query x n_index: a total that does not fit the device raises MemoryError.
        NotFittedError before `fit`, NotImplementedError after a single-source fit, as `gold_ranks`."""
        indptr, ind, dist = self.radius_neighbors_device(radius, s_to_t, sort_results)
        return self._results_to_host(indptr, ind, dist) if return_distance else self._results_to_host(indptr, ind)

    def radius_counts(self, radius, s_to_t=True):
        """The number of index rows within `radius` of every query row (`radius_neighbors`' rule) -- int64 [n_query], numpy or a
        tensor when fitted on tensors -- without the pairs: nothing but n_query + 1 offsets is allocated."""
        radius = N.radius_value(radius, "radius_counts")
        query, index = self._two_sided_operands("radius_counts", s_to_t)
        indptr, _ = N.radius_counts(self.ctx, query, index, radius)
        indptr, = self._results_to_host(indptr)
        return indptr[1:] - indptr[:-1]

    # ---- the neighbour pairs of both directions as a CSR ----------------------------------------------
    def _pairs_args(self, k, mode, what="neighbor_pairs"):
        """(k, mode) of a `neighbor_pairs` call after the checks that need no device: `mode` one of the four, k None (`n_candidates`,
        silently: this is not `kneighbors`) or an int >= 1 -- never clamped to `n_candidates`."""
        mode = N.pair_mode(mode, what)
        if k is None:
            k = self.n_candidates
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"{what} needs a positive integer k (or None: n_candidates), got {k!r}")
        return int(k), mode

    def _raw_pair_lists(self, k, mode, query, index):
        """The raw lists the pairs are taken from -> (forward (dist, ind) | None, reverse ind | None): the k nearest targets of every
        source row and the k nearest sources of every target row, each as far as `mode` reads it and each with the search's own checks
        on k.  Where both are asked for and one sweep can serve both (`kneighbors_device_both`) it does; forward lists a shared
        sweep left cached are read, not consumed: `_forward` is left as found."""
        fwd = rev = None
        cached = self._forward
        try:
            if mode != "reverse":
                k_f = self._check_k_value(k, index.shape[0])
                if cached is not None and cached[0] == k_f:
                    fwd = cached[1:]
            if mode != "forward":
                k_r = self._check_k_value(k, query.shape[0])
                if (mode != "reverse" and fwd is None and query is getattr(self, "source_index", None)
                        and index is getattr(self, "target_index", None)):
                    both = self.kneighbors_device_both(k)
                    if both is not None:
                        rev, fwd = both[1], self._forward[1:]
                if rev is None:
                    _, rev, self.last_stats_reverse = N.knn(self.ctx, index, query, k_r)
            if mode != "reverse" and fwd is None:
                dist, ind, self.last_stats = N.knn(self.ctx, query, index, k_f)
                fwd = (dist, ind)
        finally:
            self._forward = cached
        return fwd, rev

    def _neighbor_pairs(self, k, mode, sort_results, return_distance, kind=None, q_state=None, t_state=None, cast=True):
        """The device CSR of `neighbor_pairs` -> (indptr, ind, dist | None, forward lists | None): the set step on the raw lists, the
        value of every pair (plain, or reduced by `kind` and its state), the row sort, the output dtype LAST."""
        query, index = self._two_sided_operands("neighbor_pairs")
        fwd, rev = self._raw_pair_lists(k, mode, query, index)
        ctx = self.ctx
        indptr, ind, _ = N.lists_combine(ctx, fwd[1] if fwd is not None else None, rev, mode, query.shape[0], index.shape[0])
        del rev
        if not (return_distance or sort_results):
            return indptr, ind, None, fwd
        dist = N.pairs_values(ctx, query, index, indptr, ind, kind, q_state, t_state)
        if sort_results:
            N.csr_sort_rows(ctx, indptr, ind, dist, index.shape[0])
        if not return_distance:
            return indptr, ind, None, fwd
        return indptr, ind, (self._radius_distances(dist, self.target_index) if cast else dist), fwd

    def neighbor_pairs_device(self, k=None, mode="union", sort_results=True, return_distance=True):
        """`neighbor_pairs` with the CSR left in HBM: (indptr int64 [n_source + 1], ind int64 [total], dist [total]) DeviceArrays, or
        (indptr, ind) with `return_distance=False`."""
        k, mode = self._pairs_args(k, mode)
        indptr, ind, dist, _ = self._neighbor_pairs(k, mode, sort_results, return_distance)
        return (indptr, ind, dist) if return_distance else (indptr, ind)

    def neighbor_pairs(self, k=None, mode="union", return_distance=True, sort_results=True):
        """The neighbour pairs of BOTH search directions as one CSR over the source rows.  F = the pairs (i, j) with target row j among
        the k nearest targets of source row i (`kneighbors(k)`), R = the pairs (i, j) with source row i among the k nearest sources
        of target row j (`kneighbors(k, query=target, s_to_t=False)`); membership is decided by those raw lists, ties included.
        `mode`: "forward" = F, "reverse" = R grouped by source row, "union" = F | R (bidirectional candidates: a target that no source
        lists still takes part), "mutual" = F & R (mutual nearest neighbours).  Every pair appears once.  The value of a pair is
        ALWAYS the distance `kneighbors` computes from source row i to target row j -- also for a pair only R holds -- with the bits
        `radius_neighbors(inf)` returns for it; a NaN value stays (membership is by lists) and sorts last.

        `k`: None means `n_candidates` (no warning); else an int >= 1, not clamped to `n_candidates`; each direction's search applies
        its own checks.  Returns `(indptr int64 [n_source + 1], ind int64 [total], dist [total])`, or `(indptr, ind)` with
        `return_distance=False`: the targets of source row i are `ind[indptr[i]:indptr[i + 1]]`, ascending by (value, target row) or,
        with `sort_results=False`, by target row; rows have no length limit (a hub source can be listed by every target).  numpy
        arrays, or tensors when fitted on tensors; `dist` in the dtype `kneighbors` returns (for float32 cosine / precomputed input
        the cast comes last).  A fit that indexed the target only (NoHubnessReduction) searches the reverse direction against an
        upload of the source.  NotFittedError before `fit`, NotImplementedError after a single-source fit, ValueError for a `mode`
        outside the four or a k that is no positive int.  A shared sweep's cached forward lists are left as found."""
        return self._results_to_host(*self.neighbor_pairs_device(k, mode, sort_results, return_distance))

    def kneighbors_device_both(self, k=None):
        """Both directions between the fitted source and target from ONE sweep of the distance matrix (kz_knn_dual): returns
        the target -> source result (what HubnessReduction.fit needs, base.py:37-42) and keeps the source -> target result
        for the `kneighbors_device(query=None, k)` call that follows (base.py:95-96).  Identical results to the two separate
        searches.  None when sharing does not apply (sides clamped to different k, more neighbours than the fused kernels keep)."""
        check_is_fitted(self, ["source_index", "target_index"], all_or_any=all)
        k = self.n_candidates if k is None else k
        if self._metric_c == "precomputed":
            return None   # (no sweep to share: both directions read the caller's matrix -- two searches)
        if self.source_equals_target:
            # single source: the reverse search (explicit query: every row keeps itself) and the forward search (the row
            # itself stripped) are two views of ONE search for k + 1 neighbours (kz_split_self)
            n = self.source_.shape[0]
            if not np.issubdtype(type(k), np.integer) or k <= 0 or k + 1 > n or k + 1 > N.MAX_FUSED_NEIGHBORS:
                return None
            dist, ind, stats = N.knn(self.ctx, self.source_index, self.source_index, k + 1, exclude_self=False)
            self.last_stats = stats
            self.last_stats_reverse = None   # (one search serves both views: there is no second set of statistics)
            rev, fwd = N.split_self(self.ctx, dist, ind)
            self._forward = (k,) + fwd
            return rev
        n_s, n_t = self.source_.shape[0], self.target_.shape[0]
        if not np.issubdtype(type(k), np.integer) or k <= 0 or k > min(n_s, n_t):
            return None   # (the per-direction checks and clamps of kneighbors() apply: leave it to the separate searches)
        # the larger side sweeps as the query side: fewer rows get event buffers
        s_is_a = n_s >= n_t
        a, b = (self.source_index, self.target_index) if s_is_a else (self.target_index, self.source_index)
        (d_ab, i_ab, st_ab), (d_ba, i_ba, st_ba) = N.knn_dual(self.ctx, a, b, k)
        self.last_stats = st_ab
        self.last_stats_reverse = st_ba
        fwd, rev = ((d_ab, i_ab), (d_ba, i_ba)) if s_is_a else ((d_ba, i_ba), (d_ab, i_ab))
        self._forward = (k,) + fwd
        return rev

    def _kneighbors(self, k, query, index, return_distance, is_self_querying):
        """Replaces SklearnNN._kneighbors (sklearn_nearest_neighbors.py:96-101)."""
        qm = self._matrix_for(query)
        index = self._partner(qm, index)
        dist, ind, stats = N.knn(self.ctx, qm, index, k, exclude_self=is_self_querying)
        self.last_stats = stats
        if _is_tensor(query):   # tensors in -> tensors out (on the query's device), as the reference does with Faiss
            torch = _torch_if_loaded()
            self.ctx.sync()
            dev = query.device
            ind_t = torch.as_tensor(ind, device="cuda").clone().to(dev)
            dist_t = None
            if return_distance:
                dist_t = torch.as_tensor(dist, device="cuda").clone().to(dev)
                if self._out_dtype(index) == np.float32:
                    dist_t = dist_t.to(torch.float32)
            # the clones run on torch's stream, the pool that takes `dist` / `ind` back is ordered on OURS: finish them
            # before the DeviceArrays are released
            torch.cuda.current_stream().synchronize()
            return (dist_t, ind_t) if return_distance else ind_t
        ind_h = ind.numpy()
        if not return_distance:
            return ind_h
        dist_h = dist.numpy()
        out_dtype = self._out_dtype(index)
        if out_dtype != np.float64:
            dist_h = dist_h.astype(out_dtype)
        return dist_h, ind_h


def available_nn_algorithms(as_string: bool = False):
    """kiez/neighbors/util.py:18-39 (only the exact backend exists here; names are lower-cased as in the reference)."""
    return ["sklearnnn"] if as_string else [SklearnNN]
