"""ctypes binding of libkiez_amd.so (the C ABI declared in include/kiez_amd.h).

The HIP library is the product path: if it is missing, was built for another architecture, or no MI355X
is visible, every entry point raises — there is no CPU fallback anywhere in this package.

Import-order note (DESIGN.md "Process model"): PyTorch-ROCm wheels bundle their own HIP runtime.  When a
process uses both torch (for torch.distributed / RCCL) and this library, torch must be imported FIRST so
that both resolve to one HIP runtime; `load()` therefore imports torch before dlopen when it is already
importable and KIEZ_AMD_WITH_TORCH=1 is set (bench.py and kiez_amd.distributed do this).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
import threading
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

_LIB_NAME = "libkiez_amd.so"
_lib = None
_lock = threading.Lock()

KZ_F32, KZ_F64 = 0, 1
KZ_F16, KZ_BF16 = 2, 3   # 2-byte STORAGE types (IEEE binary16, the upper half of a float32): rows read in place, float64 answers
# element types by name: what DeviceMatrix.elem holds (bfloat16 has no numpy dtype; its rows travel as their uint16 bit patterns)
ELEM_CODES = {"float32": KZ_F32, "float64": KZ_F64, "float16": KZ_F16, "bfloat16": KZ_BF16}
HALF_ELEMS = ("float16", "bfloat16")
KZ_EUCLIDEAN, KZ_SQEUCLIDEAN, KZ_COSINE, KZ_MANHATTAN, KZ_CHEBYSHEV, KZ_MINKOWSKI = 0, 1, 2, 3, 4, 5
KZ_BRAYCURTIS, KZ_SEUCLIDEAN, KZ_CORRELATION, KZ_HAMMING = 6, 7, 8, 9
KZ_JACCARD, KZ_DICE, KZ_ROGERSTANIMOTO, KZ_RUSSELLRAO, KZ_SOKALMICHENER, KZ_SOKALSNEATH, KZ_YULE = 10, 11, 12, 13, 14, 15, 16
# scipy's boolean metrics: searched on a bit-packed image of the rows (x != 0), kz_bool.hip
BOOLEAN_METRICS = ("jaccard", "dice", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "yule")
METRIC_IDS = {"euclidean": KZ_EUCLIDEAN, "sqeuclidean": KZ_SQEUCLIDEAN, "cosine": KZ_COSINE, "manhattan": KZ_MANHATTAN,
              "chebyshev": KZ_CHEBYSHEV, "minkowski": KZ_MINKOWSKI, "braycurtis": KZ_BRAYCURTIS, "seuclidean": KZ_SEUCLIDEAN,
              "correlation": KZ_CORRELATION, "hamming": KZ_HAMMING, "jaccard": KZ_JACCARD, "dice": KZ_DICE,
              "rogerstanimoto": KZ_ROGERSTANIMOTO, "russellrao": KZ_RUSSELLRAO, "sokalmichener": KZ_SOKALMICHENER,
              "sokalsneath": KZ_SOKALSNEATH, "yule": KZ_YULE}
KZ_PRECOMPUTED = 17   # scikit-learn's metric="precomputed": not in METRIC_IDS -- kz_matrix_create refuses it, PrecomputedMatrix makes the handles


def half_rows_supported(metric: str) -> bool:
    """True for the metrics whose matrices take float16 / bfloat16 rows (the fused MFMA kernels: euclidean, sqeuclidean, cosine);
    kz_matrix_create refuses the 2-byte types for every other metric."""
    return METRIC_IDS.get(split_metric(metric)[0], KZ_PRECOMPUTED) <= KZ_COSINE


def row_storage(metric: str, elem: str) -> str:
    """The element type rows of type `elem` (a dtype name: 'float16', 'int32', ...) are stored as for `metric`: float32 / float64 as
    they are; float16 / bfloat16 as they are where the metric takes 2-byte rows; anything else widened -- to float32 for the
    boolean metrics (they read x != 0 only), else to float64."""
    if elem in ("float32", "float64") or (elem in HALF_ELEMS and half_rows_supported(metric)):
        return elem
    return "float32" if split_metric(metric)[0] in BOOLEAN_METRICS else "float64"


def split_metric(metric: str):
    """'minkowski[3.0]' -> ('minkowski', 3.0); any other canonical metric name -> (name, None)."""
    if metric.startswith("minkowski[") and metric.endswith("]"):
        return "minkowski", float(metric[len("minkowski["):-1])
    return metric, None
MAX_FUSED_NEIGHBORS = 110   # neighbours per query ONE fused list keeps (list length 128 minus the certification margin): the limit of
                            # the shared sweep and of the single-source split; kz_knn itself takes 111 .. ~540 on its long-k route
                            # (lists over many index ranges) and anything up to MAX_NEIGHBORS on the exact float64 kernels
MAX_NEIGHBORS = 4096
MAX_HUBNESS_CANDIDATES = 4096  # n_candidates the device hubness kernels (transform, final sort) handle (KZ_MAX_CANDIDATES)
MERGE_MAX_ENTRIES = 8192       # entries per row kz_merge_topk merges (KZ_MERGE_MAX_ENTRIES)
ABI_VERSION = 7

_ERR_TYPES = {1: ValueError, 2: RuntimeError, 3: NotImplementedError, 4: MemoryError, 5: ValueError}


class KnnStats(C.Structure):
    _fields_ = [
        ("main_kernel_ms", C.c_double),
        ("finalize_ms", C.c_double),
        ("fallback_ms", C.c_double),
        ("n_fallback_rows", C.c_int64),
        ("list_len", C.c_int32),
        ("n_splits", C.c_int32),
        ("n_blocks", C.c_int32),
        ("first_pass", C.c_int32),
        ("n_escalated_rows", C.c_int64),
        ("max_err_ratio", C.c_double),
        ("dual", C.c_int32),
        ("n_first_pass_fail", C.c_int32),
        ("n_events", C.c_int64),
        ("n_overflow_rows", C.c_int64),
        ("n_logged_groups", C.c_int64),
        ("wide_lists", C.c_int32),
        ("n_spec_rows", C.c_int32),
        ("probe_ms", C.c_double),
        ("n_range_rows", C.c_int64),
        ("n_range_pairs", C.c_int64),
        ("n_range_group_rows", C.c_int64),
        ("thresh_source", C.c_int32),
        ("model_max_events", C.c_int32),
        ("model_mean_events", C.c_double),
        ("floor_r2", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FitInfo(C.Structure):
    """kz_fit_info: the sizes, the plan that ran and the statistics of the searches of a fitted object."""
    _fields_ = [
        ("n_source", C.c_int64),
        ("n_target", C.c_int64),
        ("n_candidates", C.c_int32),
        ("hubness", C.c_int32),
        ("single_source", C.c_int32),
        ("shared_sweep", C.c_int32),
        ("search", C.c_int32),
        ("larger_first", C.c_int32),
        ("tail", C.c_int32),
        ("fused", C.c_int32),
        ("forward_ready", C.c_int32),
        ("n_searches", C.c_int32),
        ("stats_forward", KnnStats),
        ("stats_reverse", KnnStats),
    ]

    def as_dict(self):
        return {name: (getattr(self, name).as_dict() if name.startswith("stats_") else getattr(self, name)) for name, _ in self._fields_}


# every symbol include/kiez_amd.h declares: (name, restype, argtypes)
_P = C.c_void_p
_I64 = C.c_int64
SYMBOLS = [
    ("kz_abi_version", C.c_int, []),
    ("kz_last_error", C.c_char_p, []),
    ("kz_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("kz_ctx_create", C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    ("kz_ctx_destroy", C.c_int, [_P]),
    ("kz_ctx_sync", C.c_int, [_P]),
    ("kz_ctx_trim", C.c_int, [_P]),
    ("kz_ctx_mem_info", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("kz_ctx_set_option", C.c_int, [_P, C.c_char_p, C.c_double]),
    ("kz_malloc", C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    ("kz_free", C.c_int, [_P, _P]),
    ("kz_memcpy_h2d", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("kz_memcpy_d2h", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("kz_memcpy_d2d", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("kz_matrix_create", C.c_int, [_P, _P, C.c_int, _I64, _I64, C.c_int, C.c_int, C.POINTER(_P)]),
    ("kz_matrix_create_precomputed", C.c_int, [_P, _P, C.c_int, _I64, _I64, C.c_int, C.POINTER(_P), C.POINTER(_P)]),
    ("kz_matrix_destroy", C.c_int, [_P]),
    ("kz_matrix_set_minkowski_p", C.c_int, [_P, C.c_double]),
    ("kz_matrix_set_seuclidean_v", C.c_int, [_P, _P, _I64]),
    ("kz_matrix_shape", C.c_int, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("kz_knn", C.c_int, [_P, _P, _I64, _I64, _P, C.c_int, C.c_int, _P, _P, C.POINTER(KnnStats)]),
    ("kz_knn_dual", C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P, C.POINTER(KnnStats), C.POINTER(KnnStats)]),
    ("kz_pair_values", C.c_int, [_P, _P, _I64, _I64, _P, _P, C.c_int, _P]),
    ("kz_merge_topk", C.c_int, [_P, _P, _P, _P, _I64, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("kz_split_self", C.c_int, [_P, _P, _P, _I64, C.c_int, _I64, _P, _P, _P, _P]),
    ("kz_knn_plan", C.c_int, [_I64, _I64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                              C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("kz_selftest_div", C.c_int, [_P, _I64, C.c_uint64, C.c_int, C.POINTER(_I64)]),
    ("kz_selftest_image", C.c_int, [_P, _P, _P, C.c_int, _I64, C.POINTER(C.c_int), _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("kz_selftest_finalize", C.c_int, [_P, _P, _P, _P]),
    ("kz_selftest_sweep", C.c_int, [_P, _P, _P, _P]),
    ("kz_row_stats", C.c_int, [_P, _P, _I64, C.c_int, _P, _P, _P]),
    ("kz_row_nanstats", C.c_int, [_P, _P, _I64, C.c_int, _P, _P]),
    ("kz_csls", C.c_int, [_P, _P, _P, _I64, C.c_int, _P, _P]),
    ("kz_dual_shift", C.c_int, [_P, _P, _P, _I64, C.c_int, _P, _P, _P]),
    ("kz_local_scaling", C.c_int, [_P, _P, _P, _I64, C.c_int, _P, C.c_int, _P]),
    ("kz_mp_normal", C.c_int, [_P, _P, _P, _I64, C.c_int, _P, _P, _P]),
    ("kz_mp_empiric", C.c_int, [_P, _P, _P, _I64, C.c_int, _P, _P, _I64, C.c_int, _P]),
    ("kz_dsl_fit", C.c_int, [_P, _P, _I64, C.c_int, _P, _P, _I64, _P]),
    ("kz_dsl_transform", C.c_int, [_P, _P, _I64, C.c_int, _P, _I64, _P, _P, _P, _P]),
    ("kz_dsl_finalize", C.c_int, [_P, _P, _I64, C.c_double, C.c_int]),
    ("kz_select_topk", C.c_int, [_P, _P, _P, _I64, C.c_int, C.c_int, _P, _P]),
    ("kz_cast_f64_f32", C.c_int, [_P, _P, _P, _I64]),
    ("kz_rescale_select", C.c_int, [_P, _P, _P, _I64, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    ("kz_fit", C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("kz_kneighbors", C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    ("kz_fitted_info", C.c_int, [_P, C.POINTER(FitInfo)]),
    ("kz_fitted_state", C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_I64), C.POINTER(C.c_int)]),
    ("kz_fitted_destroy", C.c_int, [_P]),
    ("kz_minmax_i64", C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    ("kz_minmax_i64_2d", C.c_int, [_P, _P, _I64, C.c_int, C.c_int, C.POINTER(_I64), C.POINTER(_I64)]),
    ("kz_k_occurrence", C.c_int, [_P, _P, _I64, C.c_int, C.c_int, _I64, _P]),
    ("kz_kocc_stats", C.c_int, [_P, _P, _I64, C.c_double, C.c_int, C.POINTER(C.c_double)]),
    ("kz_kocc_select", C.c_int, [_P, _P, _I64, C.c_int, C.c_double, _P, C.POINTER(_I64)]),
    ("kz_hit_positions", C.c_int, [_P, _P, _P, _I64, C.c_int, _P]),
    ("kz_gold_ranks", C.c_int, [_P, _P, _I64, _I64, _P, _P, _P]),
    ("kz_gold_ranks_reduced", C.c_int, [_P, _P, _I64, _I64, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    ("kz_knn_reduced", C.c_int, [_P, _P, _I64, _I64, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("kz_radius_neighbors", C.c_int, [_P, _P, _I64, _I64, _P, C.c_double, C.c_int, _I64, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_radius_neighbors_reduced", C.c_int, [_P, _P, _I64, _I64, _P, C.c_double, C.c_int, _I64, C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                              C.POINTER(_I64)]),
    ("kz_softmin_rows", C.c_int, [_P, _P, _I64, _I64, _P, C.c_double, _P, C.c_double, _P]),
    ("kz_max_abs_diff", C.c_int, [_P, _P, _P, _I64, C.POINTER(C.c_double)]),
    ("kz_lists_transpose", C.c_int, [_P, _P, _P, _I64, C.c_int, _I64, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_softmin_list_rows", C.c_int, [_P, _P, _P, _I64, C.c_int, _I64, C.c_double, _P, C.c_double, _P]),
    ("kz_softmin_list_cols", C.c_int, [_P, _P, _P, _P, _I64, _I64, C.c_double, _P, C.c_double, _P]),
    ("kz_sinkhorn_lists", C.c_int, [_P, _P, _P, _I64, C.c_int, _I64, C.c_double, C.c_int, C.c_double, _P, _P, C.POINTER(C.c_int),
                                    C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("kz_rank_stats", C.c_int, [_P, _P, _I64, C.POINTER(_I64), C.c_int, C.POINTER(_I64), C.POINTER(C.c_double)]),
    ("kz_match_lists", C.c_int, [_P, _P, C.c_int, _P, _I64, C.c_int, _I64, _P, _P, C.POINTER(_I64)]),
    ("kz_match_values", C.c_int, [_P, _P, C.c_int, _P, _I64, C.c_int, _P]),
    ("kz_assign_lists", C.c_int, [_P, _P, C.c_int, _P, _I64, C.c_int, _I64, C.c_double, C.c_double, _I64, C.c_int, _P, _P, _P,
                                  C.POINTER(_I64), C.POINTER(C.c_int)]),
    ("kz_assign_range", C.c_int, [_P, _P, C.c_int, _P, _I64, C.c_int, _I64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_int)]),
    ("kz_match_csr", C.c_int, [_P, _P, _P, _P, C.c_int, _I64, _I64, _I64, _P, _P, C.POINTER(_I64)]),
    ("kz_match_values_csr", C.c_int, [_P, _P, _P, C.c_int, _P, _I64, _I64, _P]),
    ("kz_assign_csr", C.c_int, [_P, _P, _P, _P, C.c_int, _I64, _I64, _I64, C.c_double, C.c_double, _I64, C.c_int, _P, _P, _P,
                                C.POINTER(_I64), C.POINTER(C.c_int)]),
    ("kz_assign_range_csr", C.c_int, [_P, _P, _P, _P, C.c_int, _I64, _I64, _I64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int)]),
    ("kz_csr_transpose", C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_softmin_csr_rows", C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, C.c_double, _P, C.c_double, _P]),
    ("kz_sinkhorn_csr", C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, C.c_double, C.c_int, C.c_double, _P, _P, C.POINTER(C.c_int),
                                  C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("kz_lists_combine", C.c_int, [_P, _P, _I64, C.c_int, _P, _I64, C.c_int, C.c_int, _I64, _P, _P, C.POINTER(_I64)]),
    ("kz_pairs_values", C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, C.c_int, _P, _P, _P, _P, _P]),
    ("kz_csr_sort_rows", C.c_int, [_P, _P, _I64, _I64, _I64, _P, _P]),
    ("kz_components_csr", C.c_int, [_P, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_components_lists", C.c_int, [_P, _P, _I64, C.c_int, _I64, _P, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_components_edges", C.c_int, [_P, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, C.POINTER(_I64)]),
    ("kz_forest_csr", C.c_int, [_P, _P, _P, _P, C.c_int, _I64, _I64, _I64, _P, _P, _P, _P, C.POINTER(_I64), C.POINTER(_I64),
                                C.POINTER(C.c_int)]),
    ("kz_forest_lists", C.c_int, [_P, _P, C.c_int, _P, _I64, C.c_int, _I64, _P, _P, _P, _P, C.POINTER(_I64), C.POINTER(_I64),
                                  C.POINTER(C.c_int)]),
    ("kz_comm_unique_id", C.c_int, [_P]),
    ("kz_comm_create", C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    ("kz_comm_destroy", C.c_int, [_P]),
    ("kz_comm_rank", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("kz_comm_broadcast", C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    ("kz_comm_all_gather", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("kz_comm_all_to_all", C.c_int, [_P, _P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _P, C.c_size_t]),
    ("kz_comm_all_reduce_min_f64", C.c_int, [_P, _P, C.c_size_t]),
]


def library_path() -> Path:
    override = os.environ.get("KIEZ_AMD_LIB")  # diagnostic builds (tools/ablate.sh)
    return Path(override) if override else Path(__file__).resolve().parent / _LIB_NAME


def load():
    """dlopen libkiez_amd.so and bind every symbol (no GPU call is made here)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not path.exists():
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C kiez_amd/csrc`).  kiez_amd has no CPU fallback.")
        if os.environ.get("KIEZ_AMD_WITH_TORCH") == "1" and "torch" not in sys.modules:
            import torch  # noqa: F401  (one HIP runtime per process: torch's must be loaded first)
        lib = C.CDLL(str(path))
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.kz_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {lib.kz_abi_version()} != {ABI_VERSION}")
        _lib = lib
    return _lib


def _check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().kz_last_error().decode("utf-8", "replace")
        raise _ERR_TYPES.get(rc, RuntimeError)(msg or f"{what} failed with status {rc}")


def _call(owner, name: str, *args):
    """The library call `name(owner.handle, *args)` of a Context (or anything with its `lib` and `handle`), checked."""
    _check(getattr(owner.lib, name)(owner.handle, *args), name)


class Context:
    """One GPU (kz_ctx).  Contexts are cached per (device, stream)."""

    _cache = {}

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        lib = load()
        n = C.c_int(0)
        rc = lib.kz_device_count(C.byref(n))
        if rc != 0 or n.value < 1:
            raise RuntimeError(
                "kiez_amd: no MI355X (gfx950) device is visible to HIP; the exact-kNN path runs on the GPU only "
                f"({lib.kz_last_error().decode('utf-8', 'replace')})")
        h = _P()
        _check(lib.kz_ctx_create(int(device), _P(stream) if stream else None, C.byref(h)), "kz_ctx_create")
        self.lib = lib
        self.handle = h
        self.device = int(device)

    @classmethod
    def get(cls, device: Optional[int] = None, stream: Optional[int] = None) -> "Context":
        if device is None:
            device = int(os.environ.get("KIEZ_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = C.c_int(0)
            if load().kz_device_count(C.byref(n)) == 0 and n.value > 0:
                device %= n.value
        key = (device, stream)
        ctx = cls._cache.get(key)
        if ctx is None:
            ctx = cls(device, stream)
            cls._cache[key] = ctx
        return ctx

    def set_option(self, name: str, value: float):
        _call(self, "kz_ctx_set_option", name.encode(), float(value))

    def sync(self):
        _call(self, "kz_ctx_sync")

    def trim(self):
        """Release the context's cached device buffers (kz_ctx_trim)."""
        _call(self, "kz_ctx_trim")

    def mem_info(self) -> Tuple[int, int]:
        """(bytes a device allocation can still get -- free HBM plus the released buffers the context keeps --, bytes of the device)."""
        free, total = C.c_size_t(), C.c_size_t()
        _call(self, "kz_ctx_mem_info", C.byref(free), C.byref(total))
        return int(free.value), int(total.value)

    # ---- device arrays -------------------------------------------------------------------------------
    def empty(self, shape, dtype) -> "DeviceArray":
        return DeviceArray(self, shape, dtype)

    def to_device(self, arr: np.ndarray) -> "DeviceArray":
        arr = np.ascontiguousarray(arr)
        out = DeviceArray(self, arr.shape, arr.dtype)
        if arr.nbytes:
            _call(self, "kz_memcpy_h2d", out.ptr, arr.ctypes.data_as(_P), arr.nbytes)
        return out

    def as_device(self, arr, dtype=None) -> "DeviceArray":
        """numpy array -> uploaded copy; DeviceArray -> itself."""
        if isinstance(arr, DeviceArray):
            if dtype is not None and arr.dtype != np.dtype(dtype):
                raise TypeError(f"device array has dtype {arr.dtype}, expected {np.dtype(dtype)}")
            return arr
        a = np.asarray(arr)
        if dtype is not None:
            a = a.astype(dtype, copy=False)
        return self.to_device(a)


class DeviceArray:
    """A dense array in HBM owned by this object (freed on garbage collection)."""

    def __init__(self, ctx: Context, shape, dtype, ptr: Optional[int] = None, owner=None):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._owner = owner
        if ptr is None:
            p = _P()
            _call(ctx, "kz_malloc", max(self.nbytes, 16), C.byref(p))
            self.ptr = p
            self._owned = True
        else:
            self.ptr = _P(ptr)
            self._owned = False

    def __del__(self):
        if getattr(self, "_owned", False) and self.ptr:
            try:
                self.ctx.lib.kz_free(self.ctx.handle, self.ptr)
            except Exception:
                pass
            self._owned = False

    @property
    def __cuda_array_interface__(self):
        """Zero-copy export (torch.as_tensor(device_array, device="cuda"), cupy, numba)."""
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr.value or 0, False), "version": 3,
                "strides": None}

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            _call(self.ctx, "kz_memcpy_d2h", out.ctypes.data_as(_P), self.ptr, self.nbytes)
        return out

    def view_rows(self, begin: int, count: int) -> "DeviceArray":
        """A non-owning view of rows [begin, begin+count)."""
        row_bytes = self.nbytes // max(self.shape[0], 1)
        return DeviceArray(self.ctx, (count,) + self.shape[1:], self.dtype, ptr=(self.ptr.value or 0) + begin * row_bytes,
                           owner=self)

    def copy_from(self, other: "DeviceArray"):
        assert other.nbytes == self.nbytes
        _call(self.ctx, "kz_memcpy_d2d", self.ptr, other.ptr, self.nbytes)

    def fill_from_host(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes
        _call(self.ctx, "kz_memcpy_h2d", self.ptr, arr.ctypes.data_as(_P), arr.nbytes)


class DeviceMatrix:
    """kz_matrix: an embedding matrix in HBM (exact rows + float64 norms + MFMA operand images: float32 and split-bf16)."""

    def __init__(self, ctx: Context, data, metric: str, device_ptr: Optional[int] = None, shape=None, dtype=None,
                 borrow: bool = False, keepalive=None, rows_only: bool = False, V=None, elem: Optional[str] = None):
        """`device_ptr` + `borrow=True`: zero-copy -- the matrix reads the caller's HBM buffer in place (kz_matrix_create
        rows_on_device = 2); `keepalive` (the tensor / array that owns it) is held until the matrix is destroyed and must
        not be modified meanwhile (the reference holds its inputs the same way, neighbor_algorithm_base.py:95-96).
        `V`: metric 'seuclidean', the per-feature variances (kz_matrix_set_seuclidean_v; both matrices of a search need the same).
        `elem`: the element type by name (ELEM_CODES) where `dtype` cannot say it: 'bfloat16' rows have no numpy dtype and come as
        their uint16 bit patterns (host `data` of dtype uint16, or a device pointer).  float16 numpy arrays are uploaded as they
        are, 2 bytes per element, for the metrics that take 2-byte rows (`half_rows_supported`); for any other metric they are
        widened to float64 like every other dtype.  `self.elem` is the stored element type, `self.dtype` its numpy dtype (uint16
        for bfloat16)."""
        self.ctx = ctx
        self.metric = metric
        metric, mink_p = split_metric(metric)
        h = _P()
        if device_ptr is None:
            arr = np.ascontiguousarray(data)
            if arr.ndim != 2:
                raise ValueError(f"Expected 2D array, got {arr.ndim}D array instead")
            if elem == "bfloat16":
                if arr.dtype != np.uint16:
                    raise ValueError(f"bfloat16 rows come as their uint16 bit patterns, got {arr.dtype}")
            elif elem is not None:     # (said by the caller: taken as it is, and the library refuses what it does not take)
                if elem not in ELEM_CODES or np.dtype(elem) != arr.dtype:
                    raise ValueError(f"elem={elem!r} does not describe an array of dtype {arr.dtype}")
            else:
                elem = row_storage(self.metric, arr.dtype.name)
                if arr.dtype.name != elem:
                    arr = arr.astype(elem)
            self.shape = arr.shape
            self.dtype = arr.dtype
            self.elem = elem
            _call(ctx, "kz_matrix_create", arr.ctypes.data_as(_P), 0, arr.shape[0], arr.shape[1], ELEM_CODES[elem], METRIC_IDS[metric], C.byref(h))
        else:
            self.shape = tuple(shape)
            self.dtype = np.dtype(np.uint16 if elem == "bfloat16" else (dtype if dtype is not None else elem))
            self.elem = elem if elem is not None else self.dtype.name
            if self.elem not in ELEM_CODES or (self.elem != "bfloat16" and np.dtype(self.elem) != self.dtype):
                raise ValueError(f"device rows must be float32, float64, float16 or bfloat16 (elem='bfloat16'), got dtype={dtype!r} elem={elem!r}")
            self._keepalive = keepalive if borrow else None
            self.rows_ptr = int(device_ptr) if borrow else None   # borrowed rows: the caller's buffer, read in place
            if rows_only and not borrow:
                raise ValueError("rows_only needs a borrowed device buffer")
            # (rows_only: kz_matrix_create rows_on_device = 3 -- a row source for kz_dsl_fit, nothing computed, not searchable)
            _call(ctx, "kz_matrix_create", _P(device_ptr), (3 if rows_only else 2) if borrow else 1, self.shape[0], self.shape[1],
                  ELEM_CODES[self.elem], METRIC_IDS[metric], C.byref(h))
        self.handle = h
        if mink_p is not None:
            _check(ctx.lib.kz_matrix_set_minkowski_p(h, mink_p), "kz_matrix_set_minkowski_p")
        if V is not None:
            v = np.ascontiguousarray(V, dtype=np.float64)
            _check(ctx.lib.kz_matrix_set_seuclidean_v(h, v.ctypes.data_as(_P), v.shape[0]), "kz_matrix_set_seuclidean_v")

    rows_ptr = None   # borrowed rows only: the address of the caller's buffer the matrix reads in place
    view = None   # a view of a precomputed distance matrix: "rows" or "columns" (DeviceMatrix.precomputed); None: an embedding matrix

    @classmethod
    def precomputed(cls, ctx: Context, data, device_ptr: Optional[int] = None, shape=None, dtype=None, borrow: bool = False,
                    keepalive=None) -> Tuple["DeviceMatrix", "DeviceMatrix"]:
        """kz_matrix_create_precomputed: the two views (rows, columns) of ONE distance matrix [n_source, n_target], float32 or float64
        -- `rows` has one row per source row, `columns` one per target row; a search pairs one view as query with the other as
        index.  `data`: a 2-D numpy array (copied into HBM; NaN, an infinity or a negative value raise ValueError here), or
        `device_ptr` + `shape` + `dtype` as in the constructor (`borrow=True`: read in place, `keepalive` held until both views are
        gone; the verdict on the values then comes from the first search).  The storage is shared and reference counted in the
        library: the views may be dropped in either order."""
        rows_h, cols_h = _P(), _P()
        if device_ptr is None:
            arr = np.ascontiguousarray(data)
            if arr.ndim != 2:
                raise ValueError(f"Expected 2D array, got {arr.ndim}D array instead")
            if arr.dtype not in (np.float32, np.float64):
                arr = arr.astype(np.float64)
            shape, dtype = arr.shape, arr.dtype
            ptr, where = arr.ctypes.data_as(_P), 0
        else:
            shape, dtype = tuple(int(s) for s in shape), np.dtype(dtype)
            if len(shape) != 2 or dtype not in (np.float32, np.float64):
                raise ValueError("a precomputed device matrix must be a 2D float32/float64 array")
            ptr, where = _P(device_ptr), 2 if borrow else 1
        _call(ctx, "kz_matrix_create_precomputed", ptr, where, shape[0], shape[1], KZ_F32 if dtype == np.float32 else KZ_F64, C.byref(rows_h),
              C.byref(cols_h))
        views = []
        for handle, view, shp in ((rows_h, "rows", (shape[0], shape[1])), (cols_h, "columns", (shape[1], shape[0]))):
            m = cls.__new__(cls)
            m.ctx, m.metric, m.shape, m.dtype, m.handle, m.view = ctx, "precomputed", shp, np.dtype(dtype), handle, view
            m.elem = m.dtype.name
            m._keepalive = keepalive if (device_ptr is not None and borrow) else None
            views.append(m)
        return views[0], views[1]

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.ctx.lib.kz_matrix_destroy(h)
            except Exception:
                pass
            self.handle = None


# ---- the two buffer kinds ---------------------------------------------------------------------------------------------------------
# This module is the only one that calls the library.  The wrappers `distributed.HipEngine` shares with the single-GPU classes take
# device buffers as DeviceArrays or contiguous torch CUDA tensors (`_ptr`; no dtype check: callers pass reinterpreted views) and allocate
# outputs through `alloc`: (shape, numpy dtype) -> buffer, None: `ctx.empty`.  What a call computes: its declaration in include/kiez_amd.h.
def _ptr(buf, what: str = "an output"):
    """The device address of `buf` as a c_void_p: a DeviceArray's `.ptr`, None for None, a tensor's `data_ptr()` -- of a contiguous
    CUDA tensor only: anything else raises TypeError naming the argument `what` (a host pointer must never reach a kernel)."""
    if hasattr(buf, "data_ptr"):
        if not (buf.is_cuda and buf.is_contiguous()):
            raise TypeError(f"{what} must be a DeviceArray or a contiguous CUDA tensor")
        return _P(buf.data_ptr())
    return None if buf is None else buf.ptr


def knn(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, k: int, exclude_self: bool = False,
        q_begin: int = 0, q_count: Optional[int] = None, alloc=None) -> Tuple[DeviceArray, DeviceArray, dict]:
    """kz_knn -> (dist float64 [q, k], ind int64 [q, k], stats) on the device."""
    alloc = alloc or ctx.empty
    if q_count is None:
        q_count = query.shape[0] - q_begin
    dist, ind, st = alloc((q_count, k), np.float64), alloc((q_count, k), np.int64), KnnStats()
    _call(ctx, "kz_knn", query.handle, q_begin, q_count, index.handle, int(k), int(bool(exclude_self)), _ptr(dist), _ptr(ind), C.byref(st))
    return dist, ind, st.as_dict()


def knn_dual(ctx: Context, a: DeviceMatrix, b: DeviceMatrix, k: int, alloc=None):
    """kz_knn_dual: both directions between two matrices from one sweep of the distance matrix.
    Returns ((dist, ind, stats) of a -> b [a.n, k], (dist, ind, stats) of b -> a [b.n, k])."""
    alloc = alloc or ctx.empty
    d_ab, i_ab = alloc((a.shape[0], k), np.float64), alloc((a.shape[0], k), np.int64)
    d_ba, i_ba = alloc((b.shape[0], k), np.float64), alloc((b.shape[0], k), np.int64)
    s_ab, s_ba = KnnStats(), KnnStats()
    _call(ctx, "kz_knn_dual", a.handle, b.handle, int(k), _ptr(d_ab), _ptr(i_ab), _ptr(d_ba), _ptr(i_ba), C.byref(s_ab), C.byref(s_ba))
    return (d_ab, i_ab, s_ab.as_dict()), (d_ba, i_ba, s_ba.as_dict())


def pair_values(ctx: Context, query: DeviceMatrix, q_begin: int, q_count: int, index: DeviceMatrix, ind, alloc=None):
    out = (alloc or ctx.empty)(tuple(ind.shape), np.float64)
    _call(ctx, "kz_pair_values", query.handle, q_begin, q_count, index.handle, _ptr(ind, "ind"), ind.shape[1], _ptr(out))
    return out


def merge_topk(ctx: Context, key, ind, dist, segs: int, seg_len: int, k: int, alloc=None):
    """kz_merge_topk -> (dist or key [n, k], ind [n, k]) of key [n, segs * seg_len <= MERGE_MAX_ENTRIES]; `ind` / `dist` may be None."""
    alloc = alloc or ctx.empty
    od, oi = alloc((key.shape[0], k), np.float64), alloc((key.shape[0], k), np.int64)
    _call(ctx, "kz_merge_topk", _ptr(key, "key"), _ptr(ind, "ind"), _ptr(dist, "dist"), key.shape[0], segs, seg_len, k, _ptr(od), _ptr(oi))
    return od, oi


def gold_ranks(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, gold_dev: DeviceArray, q_begin: int = 0,
               q_count: Optional[int] = None) -> DeviceArray:
    """kz_gold_ranks -> int64 [q_count] on the device: the 0-based rank of index row gold_dev[r] for query row q_begin + r against
    the whole index (the position it holds in kz_knn with k = index.n), -1 where gold_dev[r] is INT64_MIN or no index row."""
    if q_count is None:
        q_count = query.shape[0] - q_begin
    if gold_dev.dtype != np.int64 or gold_dev.shape != (q_count,):
        raise ValueError(f"gold_dev must be int64 of shape ({q_count},), got {gold_dev.dtype} {gold_dev.shape}")
    rank = ctx.empty((q_count,), np.int64)
    _call(ctx, "kz_gold_ranks", query.handle, q_begin, q_count, index.handle, gold_dev.ptr, rank.ptr)
    return rank


# kz_gold_ranks_reduced's kinds (include/kiez_amd.h: KZ_RANK_*)
RANK_CSLS, RANK_LS, RANK_NICDM, RANK_MP_NORMAL = 1, 2, 3, 4
RANK_DUAL = 8   # w = (d - f_i) - g_j, the dual potentials of Sinkhorn / the inverted softmax (5 .. 7 stay unknown kinds)


def gold_ranks_reduced(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, gold_dev: DeviceArray, kind: int, q_state, t_state,
                       q_begin: int = 0, q_count: Optional[int] = None) -> DeviceArray:
    """kz_gold_ranks_reduced -> int64 [q_count] on the device: the rank of index row gold_dev[r] for query row q_begin + r against the
    whole index under a pointwise hubness reduction (`kind`: RANK_CSLS, RANK_LS, RANK_NICDM, RANK_MP_NORMAL).  `q_state`: the
    float64 DeviceArrays [q_count] of the query side, entry r for query row q_begin + r -- one (mean / last) or, for MP normal, two
    (nanmean, nanstd); `t_state`: the same of the index side, [index rows].  A single DeviceArray stands for a 1-tuple."""
    if q_count is None:
        q_count = query.shape[0] - q_begin
    if gold_dev.dtype != np.int64 or gold_dev.shape != (q_count,):
        raise ValueError(f"gold_dev must be int64 of shape ({q_count},), got {gold_dev.dtype} {gold_dev.shape}")
    state = _reduction_state(q_state, t_state, q_count, index.shape[0])
    rank = ctx.empty((q_count,), np.int64)
    _call(ctx, "kz_gold_ranks_reduced", query.handle, q_begin, q_count, index.handle, gold_dev.ptr, int(kind), *state, rank.ptr)
    return rank


def _reduction_state(q_state, t_state, q_count: int, n_index: int):
    """The four state pointers (q_a, q_b, t_a, t_b; None where a side has one vector) of kz_gold_ranks_reduced / kz_knn_reduced."""
    q_state = (q_state,) if isinstance(q_state, DeviceArray) else tuple(q_state)
    t_state = (t_state,) if isinstance(t_state, DeviceArray) else tuple(t_state)
    for what, state, n in (("q_state", q_state, q_count), ("t_state", t_state, n_index)):
        if not 1 <= len(state) <= 2:
            raise ValueError(f"{what}: one or two device vectors, got {len(state)}")
        for v in state:
            if not isinstance(v, DeviceArray) or v.dtype != np.float64 or v.shape != (n,):
                raise ValueError(f"{what} must hold float64 device vectors of shape ({n},)")
    qp = [v.ptr for v in q_state] + [None]
    tp = [v.ptr for v in t_state] + [None]
    return qp[0], qp[1], tp[0], tp[1]


# neighbours per query of kz_knn_reduced (include/kiez_amd.h: KZ_KNN_REDUCED_MAX_K)
KNN_REDUCED_MAX_K = 512


def knn_reduced(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, k: int, kind: int, q_state, t_state, q_begin: int = 0,
                q_count: Optional[int] = None) -> Tuple[DeviceArray, DeviceArray]:
    """kz_knn_reduced -> (w float64 [q_count, k], ind int64 [q_count, k]) on the device: the k index rows with the smallest
    hubness-reduced distance to query row q_begin + r over the WHOLE index, ascending by (w, index row) -- the list the ranks of
    `gold_ranks_reduced` are positions in.  `kind`, `q_state` and `t_state` as there."""
    if q_count is None:
        q_count = query.shape[0] - q_begin
    state = _reduction_state(q_state, t_state, q_count, index.shape[0])
    k = int(k)
    # (a k the call refuses -- it says why, before it writes anything -- gets no [q_count, k] arrays)
    shape = (q_count, k) if 1 <= k <= min(index.shape[0], KNN_REDUCED_MAX_K) else (0, 0)
    w = ctx.empty(shape, np.float64)
    ind = ctx.empty(shape, np.int64)
    _call(ctx, "kz_knn_reduced", query.handle, q_begin, q_count, index.handle, k, int(kind), *state, w.ptr, ind.ptr)
    return w, ind


def radius_value(radius, what: str = "radius_neighbors") -> float:
    """The threshold of a radius call as a float: a real number -- +-inf and negative values are legal (CSLS values are routinely
    negative); a bool or anything that is no real number raises TypeError, NaN raises ValueError.  Checked on the host, before the
    device is touched."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what} needs a real number as radius, got {radius!r}")
    radius = float(radius)
    if radius != radius:
        raise ValueError(f"{what} needs a radius that is not NaN")
    return radius


# pairs per query row the first call of `radius_neighbors` leaves room for, before it knows the total
RADIUS_FIRST_CAPACITY_PER_ROW = 32


def _radius_call(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, radius: float, sort_results: bool, capacity: int, kind, state,
                 q_begin: int, q_count: int):
    """One kz_radius_neighbors / kz_radius_neighbors_reduced call -> (indptr [q_count + 1], ind [capacity], dist [capacity], total)."""
    indptr = ctx.empty((q_count + 1,), np.int64)
    ind = ctx.empty((capacity,), np.int64)
    dist = ctx.empty((capacity,), np.float64)
    total = _I64(0)
    if kind is None:
        _call(ctx, "kz_radius_neighbors", query.handle, q_begin, q_count, index.handle, radius, int(bool(sort_results)), capacity, indptr.ptr,
              ind.ptr, dist.ptr, C.byref(total))
    else:
        _call(ctx, "kz_radius_neighbors_reduced", query.handle, q_begin, q_count, index.handle, radius, int(bool(sort_results)), capacity, int(kind),
              *state, indptr.ptr, ind.ptr, dist.ptr, C.byref(total))
    return indptr, ind, dist, int(total.value)


def radius_neighbors(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, radius: float, kind: Optional[int] = None, q_state=None,
                     t_state=None, sort_results: bool = True, capacity: Optional[int] = None, q_begin: int = 0,
                     q_count: Optional[int] = None) -> Tuple[DeviceArray, DeviceArray, DeviceArray, int]:
    """kz_radius_neighbors (`kind` None) / kz_radius_neighbors_reduced -> (indptr int64 [q_count + 1], ind int64, dist float64, total):
    every index row j with w <= radius for query row q_begin + r, as a CSR on the device -- w the distance `knn` returns or, with a
    `kind` of `gold_ranks_reduced` and its `q_state` / `t_state`, the hubness-reduced distance of `knn_reduced`; a NaN w is never in
    the result.  Rows ascend by (w, index row) in `knn_reduced`'s order, or with `sort_results=False` by index row.

    `capacity` None: the allocation policy -- a first call with room for min(n_q n_t, 32 n_q) pairs; when the total is larger, ONE
    second call with room for exactly the total, refused with MemoryError (naming the total) when the output would not fit what
    the device has free; ind / dist come back with `total` entries.  `capacity` given: that one call as the library makes it -- ind /
    dist have `capacity` entries, hold the rows whose end offset is <= capacity and nothing defined beyond them; indptr and total
    are exact either way (capacity 0: `radius_counts`)."""
    radius = radius_value(radius)
    if q_count is None:
        q_count = query.shape[0] - q_begin
    state = None
    if kind is not None:
        if q_state is None or t_state is None:
            state = (None, None, None, None)   # (the library says which vectors the kind needs)
        else:
            state = _reduction_state(q_state, t_state, q_count, index.shape[0])
    elif q_state is not None or t_state is not None:
        raise ValueError("q_state / t_state belong to a reduced call: name its kind")
    if capacity is not None:
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
            raise ValueError(f"capacity must be a non-negative integer, got {capacity!r}")
        return _radius_call(ctx, query, index, radius, sort_results, int(capacity), kind, state, q_begin, q_count)
    n_q = max(int(q_count), 0)
    first = min(n_q * index.shape[0], RADIUS_FIRST_CAPACITY_PER_ROW * n_q)
    indptr, ind, dist, total = _radius_call(ctx, query, index, radius, sort_results, first, kind, state, q_begin, q_count)
    if total > first:
        del ind, dist   # (back to the context's pool: counted as free below)
        # 16 bytes per pair, and as much again while rows beyond the LDS sort's reach are sorted through HBM
        need = 16 * total * (2 if sort_results else 1)
        free, _ = ctx.mem_info()   # (the exact stage's value block is allocated by now: what is free is what it leaves)
        if need > free:
            raise MemoryError(f"radius_neighbors: total = {total} pairs within radius {radius!r} need {need} bytes of device memory, "
                              f"{free} are free: use a smaller radius or a row range (q_begin / q_count)")
        indptr, ind, dist, total = _radius_call(ctx, query, index, radius, sort_results, total, kind, state, q_begin, q_count)
    return indptr, ind.view_rows(0, total), dist.view_rows(0, total), total


def radius_counts(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, radius: float, kind: Optional[int] = None, q_state=None,
                  t_state=None, q_begin: int = 0, q_count: Optional[int] = None) -> Tuple[DeviceArray, int]:
    """`radius_neighbors` with capacity 0 -> (indptr int64 [q_count + 1] on the device, total): the counts alone, nothing else written."""
    indptr, _, _, total = radius_neighbors(ctx, query, index, radius, kind, q_state, t_state, False, 0, q_begin, q_count)
    return indptr, total


# index rows per first-level workgroup of kz_softmin_rows (include/kiez_amd.h: KZ_SOFTMIN_CHUNK_ROWS): part of its summation order
SOFTMIN_CHUNK = 4096


def _f64_vector(what: str, v, n: Optional[int] = None) -> DeviceArray:
    """`v` if it is a 1-D float64 device vector (of length `n`, where one is given)."""
    if not isinstance(v, DeviceArray) or v.dtype != np.float64 or len(v.shape) != 1 or (n is not None and v.shape[0] != n):
        raise ValueError(f"{what} must be a float64 device vector" + ("" if n is None else f" of shape ({n},)"))
    return v


def softmin_rows(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, eps: float, off: Optional[DeviceArray] = None,
                 shift: float = 0.0, q_begin: int = 0, q_count: Optional[int] = None) -> DeviceArray:
    """kz_softmin_rows -> float64 [q_count] on the device: per query row q_begin + r the soft-min at temperature `eps` over EVERY
    index row j of (d_rj - off[j]), plus `shift`; d is the distance kz_knn returns for the pair.  `off`: a float64 DeviceArray
    [index rows] or None.  NaN entries count as +inf; the bits of a row do not depend on how the rows are split into calls."""
    if q_count is None:
        q_count = query.shape[0] - q_begin
    if off is not None:
        _f64_vector("off", off, index.shape[0])
    out = ctx.empty((max(q_count, 0),), np.float64)
    _call(ctx, "kz_softmin_rows", query.handle, q_begin, q_count, index.handle, float(eps), off.ptr if off is not None else None, float(shift),
          out.ptr)
    return out


def dual_shift(ctx: Context, dist: DeviceArray, ind: DeviceArray, f: DeviceArray, g: DeviceArray) -> DeviceArray:
    """kz_dual_shift -> float64 [n, K] on the device: (dist[i, c] - f[i]) - g[ind[i, c]], the candidate-list form of RANK_DUAL.
    Every entry of `ind` must be a row of `g` (the native call trusts it, as kz_csls does: `index_range` reads the range back)."""
    if len(dist.shape) != 2 or dist.shape != ind.shape or dist.dtype != np.float64 or ind.dtype != np.int64:
        raise ValueError(f"dist (float64) and ind (int64) must be 2-D device arrays of one shape, got {dist.dtype} {dist.shape} and "
                         f"{ind.dtype} {ind.shape}")
    n, K = dist.shape
    _f64_vector("f", f, n)
    _f64_vector("g", g)
    out = ctx.empty((n, K), np.float64)
    _call(ctx, "kz_dual_shift", dist.ptr, ind.ptr, n, K, f.ptr, g.ptr, out.ptr)
    return out


def index_range(ctx: Context, ind: DeviceArray) -> Tuple[int, int]:
    """kz_minmax_i64 -> (smallest, largest) entry of a non-empty int64 device array."""
    lo, hi = _I64(0), _I64(0)
    _call(ctx, "kz_minmax_i64", ind.ptr, int(np.prod(ind.shape, dtype=np.int64)), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def max_abs_diff(ctx: Context, a: DeviceArray, b: DeviceArray) -> float:
    """kz_max_abs_diff -> max |a - b| of two float64 device vectors of one shape, NaN differences ignored (0.0 when none is left)."""
    _f64_vector("b", b, _f64_vector("a", a).shape[0])
    h = C.c_double(0.0)
    _call(ctx, "kz_max_abs_diff", a.ptr, b.ptr, a.shape[0], C.byref(h))
    return float(h.value)


# entries of a column per first-level wave of kz_softmin_list_cols (include/kiez_amd.h: KZ_SOFTMIN_LIST_CHUNK): part of its summation order
SOFTMIN_LIST_CHUNK = 512
# a row with more entries bids with one wave in kz_assign_csr (include/kiez_amd.h: KZ_CSR_LONG_ROW)
CSR_LONG_ROW = 256
COMPONENTS_MAX_NODES = 2 ** 31 - 2   # n_source + n_target of kz_components_*: node ids are int32 on the device


def _list_ids(what: str, ind: DeviceArray):
    if not isinstance(ind, DeviceArray) or len(ind.shape) != 2 or ind.dtype != np.int64:
        raise ValueError(f"{what} must be a 2-D int64 DeviceArray of ids, got "
                         f"{getattr(ind, 'dtype', type(ind).__name__)} {getattr(ind, 'shape', '')}")
    return ind.shape


class ListsTransposed:
    """The column-major view of the pairs of a pair list (`PairList.transpose`): `colptr` int64 [n_index + 1], `col_row` int32 and
    `col_val` float64 with `nnz` entries used (the arrays hold every entry); column j is colptr[j] .. colptr[j + 1] - 1, ascending
    source row."""

    def __init__(self, colptr, col_row, col_val, nnz, n_q, n_index):
        self.colptr, self.col_row, self.col_val, self.nnz, self.n_q, self.n_index = colptr, col_row, col_val, nnz, n_q, n_index


class PairList:
    """A PAIR LIST on the device in either of its two layouts -- THE place of the Python side that knows them apart (the native one:
    kz_rows.h / kz_rows.hip).  Fixed width (`PairList.lists`): dist / ind [n_q, k], entry (i, c) pairs source row i with target row
    ind[i, c].  CSR (`PairList.csr`): indptr int64 [n_q + 1], ind and dist [nnz], row i holds the entries indptr[i] ..
    indptr[i + 1] - 1; rows of any length, also none.  Either way an entry is a pair when 0 <= ind < n_target (a -1, the INT_MAX
    padding of `knn_reduced`: none), ind is int64 and dist float32 or float64; `dist` None: a list without values (`components`),
    `ind` None: values alone (`values`).  The constructors check shapes and dtypes; the CONTENT of a CSR's indptr is checked on the
    device, by every call, before anything reads through it (a bad one raises ValueError).

    Every operation is one method with one body: it allocates the outputs, puts the layout's leading arguments in the order its
    native symbol takes them (`_head`) and calls the symbol of the layout (`OPS`); what follows the head is the same for both."""

    # operation -> (the fixed-width symbol, the CSR symbol, which leading arguments the pair takes: `_head`'s keywords)
    OPS = {
        "match": ("kz_match_lists", "kz_match_csr", {"dtype": True}),
        "values": ("kz_match_values", "kz_match_values_csr", {"dtype": True, "ids": False, "col": True}),
        "assign": ("kz_assign_lists", "kz_assign_csr", {"dtype": True}),
        "value_range": ("kz_assign_range", "kz_assign_range_csr", {"dtype": True}),
        "transpose": ("kz_lists_transpose", "kz_csr_transpose", {}),
        "softmin_rows": ("kz_softmin_list_rows", "kz_softmin_csr_rows", {}),
        "sinkhorn": ("kz_sinkhorn_lists", "kz_sinkhorn_csr", {}),
        "components": ("kz_components_lists", "kz_components_csr", {"values": False}),
    }
    # the hierarchy of a pair list is no operation ON its pairs but another structure made from them: its pair of symbols, by layout
    FOREST = ("kz_forest_lists", "kz_forest_csr")

    def __init__(self, ctx, dist, ind, indptr, n_target, n_q, width):
        self.ctx, self.dist, self.ind, self.indptr = ctx, dist, ind, indptr
        self.n_target = None if n_target is None else int(n_target)
        self.n_q = n_q
        self._width = width   # fixed width: k; CSR: nnz -- what follows n_q in a native call

    @classmethod
    def lists(cls, ctx: "Context", dist: Optional[DeviceArray], ind: Optional[DeviceArray], n_target: Optional[int]) -> "PairList":
        """The fixed-width lists dist / ind [n_q, k]."""
        if dist is None:
            n_q, k = _list_ids("ind", ind)
        elif ind is None:
            if len(dist.shape) != 2 or dist.dtype not in (np.float32, np.float64):
                raise ValueError(f"dist must be a 2-D float32 or float64 device array, got {dist.dtype} {dist.shape}")
            n_q, k = dist.shape
        else:
            if not isinstance(dist, DeviceArray) or not isinstance(ind, DeviceArray):
                raise ValueError("dist and ind must be DeviceArrays")
            if len(dist.shape) != 2 or dist.shape != ind.shape:
                raise ValueError(f"dist and ind must be 2-D and of one shape, got {dist.shape} and {ind.shape}")
            if dist.dtype not in (np.float32, np.float64) or ind.dtype != np.int64:
                raise ValueError(f"dist must be float32 or float64 and ind int64, got {dist.dtype} and {ind.dtype}")
            n_q, k = dist.shape
        return cls(ctx, dist, ind, None, n_target, n_q, k)

    @classmethod
    def csr(cls, ctx: "Context", indptr: DeviceArray, ind: Optional[DeviceArray], dist: Optional[DeviceArray],
            n_target: Optional[int]) -> "PairList":
        """The CSR (indptr, ind, dist)."""
        ptr_ok = isinstance(indptr, DeviceArray) and len(indptr.shape) == 1 and indptr.shape[0] >= 1 and indptr.dtype == np.int64
        if dist is None:
            if not ptr_ok or not isinstance(ind, DeviceArray) or len(ind.shape) != 1 or ind.dtype != np.int64:
                raise ValueError("indptr must be a 1-D int64 DeviceArray of n_q + 1 entries and ind a 1-D int64 DeviceArray")
        elif ind is None:
            if not ptr_ok:
                raise ValueError("indptr must be a 1-D int64 DeviceArray of n_q + 1 entries")
            if not isinstance(dist, DeviceArray) or len(dist.shape) != 1 or dist.dtype not in (np.float32, np.float64):
                raise ValueError("with indptr, dist must be a 1-D float32 or float64 DeviceArray")
        else:
            if not all(isinstance(a, DeviceArray) for a in (indptr, ind, dist)):
                raise ValueError("indptr, ind and dist must be DeviceArrays")
            if not ptr_ok:
                raise ValueError(f"indptr must be a 1-D int64 array of n_q + 1 entries, got {indptr.dtype} {indptr.shape}")
            if len(dist.shape) != 1 or dist.shape != ind.shape:
                raise ValueError(f"with indptr, dist and ind must be 1-D and of one length, got {dist.shape} and {ind.shape}")
            if dist.dtype not in (np.float32, np.float64) or ind.dtype != np.int64:
                raise ValueError(f"dist must be float32 or float64 and ind int64, got {dist.dtype} and {ind.dtype}")
        return cls(ctx, dist, ind, indptr, n_target, indptr.shape[0] - 1, (dist if ind is None else ind).shape[0])

    @property
    def is_csr(self) -> bool:
        return self.indptr is not None

    @property
    def n_entries(self) -> int:
        return self._width if self.is_csr else self.n_q * self._width

    @property
    def dtype_code(self) -> int:
        return KZ_F32 if self.dist.dtype == np.float32 else KZ_F64

    def require_f64(self) -> "PairList":
        """`self` if its values are float64, as the soft-min calls and the row sort take them."""
        if self.dist.dtype != np.float64:
            raise ValueError(f"the soft-min over {'a CSR pair list' if self.is_csr else 'neighbour lists'} takes float64 values, "
                             f"got {self.dist.dtype}")
        return self

    def _head(self, values: bool = True, dtype: bool = False, ids: bool = True, col: Optional[DeviceArray] = None) -> tuple:
        """The leading arguments of a native call: fixed width `ctx, dist[, dtype], ind[, col], n_q, k`, CSR
        `ctx, indptr, ind, dist[, dtype][, col], n_q, nnz` -- without the values, the ids or with `col` where the call says so."""
        d = ((self.dist.ptr,) + ((self.dtype_code,) if dtype else ())) if values else ()
        i = (self.ind.ptr,) if ids else ()
        c = () if col is None else (col.ptr,)
        if self.is_csr:
            return (self.ctx.handle, self.indptr.ptr) + i + d + c + (self.n_q, self._width)
        return (self.ctx.handle,) + d + i + c + (self.n_q, self._width)

    def _call(self, op: str, *tail, col: Optional[DeviceArray] = None):
        """The native symbol of `op` for this layout: its head, then `tail`."""
        name = self.OPS[op][self.is_csr]
        head = {key: (col if key == "col" else flag) for key, flag in self.OPS[op][2].items()}
        _check(getattr(self.ctx.lib, name)(*self._head(**head), *tail), name)

    def match(self) -> Tuple[DeviceArray, DeviceArray, int]:
        """kz_match_lists / kz_match_csr -> (match int64 [n_q], col int64 [n_q], rounds): the source-proposing stable matching against
        n_target target rows.  match[i] is the target row of source row i and col[i] the column of that pair -- in a CSR the position
        of the entry inside row i --, -1 both where the row stays unmatched; rounds counts the proposal rounds."""
        match, col = self.ctx.empty((self.n_q,), np.int64), self.ctx.empty((self.n_q,), np.int64)
        rounds = _I64(0)
        self._call("match", self.n_target, match.ptr, col.ptr, C.byref(rounds))
        return match, col, int(rounds.value)

    def values(self, col: DeviceArray) -> DeviceArray:
        """kz_match_values[_csr] -> the value of entry col[i] of row i in dist's dtype, NaN where col[i] is outside the row (-1): [n_q]
        on the device."""
        if col.dtype != np.int64 or col.shape != (self.n_q,):
            raise ValueError(f"col must be int64 of shape ({self.n_q},), got {col.dtype} {col.shape}")
        out = self.ctx.empty((self.n_q,), self.dist.dtype)
        self._call("values", out.ptr, col=col)
        return out

    def assign(self, unmatched_cost: float, eps: float, max_rounds: int, tail_rows: int = 0, want_prices: bool = False):
        """kz_assign_lists / kz_assign_csr -> (match int64 [n_q], col int64 [n_q], prices float64 [n_target] | None, rounds,
        converged): the forward auction against n_target target rows -- a one-to-one matching whose cost (the values of the matched
        pairs plus unmatched_cost per unmatched row) is within n_q * eps of the minimum.  match / col as `match` returns them.
        tail_rows: 0 the default switch to the single-workgroup kernel, 1 .. 1024 that many FREE rows, negative never; rows of a CSR
        with more than CSR_LONG_ROW entries bid with one wave; the arrays depend on neither.  converged False: max_rounds ended the
        run, the matching is valid but not optimal."""
        match, col = self.ctx.empty((self.n_q,), np.int64), self.ctx.empty((self.n_q,), np.int64)
        prices = self.ctx.empty((self.n_target,), np.float64) if want_prices and 1 <= self.n_target < 2 ** 31 - 1 else None
        rounds, converged = _I64(0), C.c_int(0)
        self._call("assign", self.n_target, float(unmatched_cost), float(eps), int(max_rounds), int(tail_rows), match.ptr, col.ptr,
                   prices.ptr if prices is not None else None, C.byref(rounds), C.byref(converged))
        return match, col, prices, int(rounds.value), bool(converged.value)

    def value_range(self):
        """kz_assign_range[_csr] -> (smallest, largest) finite value listed with 0 <= ind < n_target, as float64; None when there is
        none."""
        lo, hi, some = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        self._call("value_range", self.n_target, C.byref(lo), C.byref(hi), C.byref(some))
        return (float(lo.value), float(hi.value)) if some.value else None

    def transpose(self) -> ListsTransposed:
        """kz_lists_transpose / kz_csr_transpose -> the column-major view of the pairs (float64 values): the entries of a column in
        ascending flat position (ascending source row).  The same arrays from every run."""
        ctx = self.require_f64().ctx
        colptr = ctx.empty((self.n_target + 1,), np.int64)
        col_row, col_val = ctx.empty((self.n_entries,), np.int32), ctx.empty((self.n_entries,), np.float64)
        nnz = _I64(0)
        self._call("transpose", self.n_target, colptr.ptr, col_row.ptr, col_val.ptr, C.byref(nnz))
        return ListsTransposed(colptr, col_row, col_val, int(nnz.value), self.n_q, self.n_target)

    def softmin_rows(self, eps: float, off: Optional[DeviceArray] = None, shift: float = 0.0) -> DeviceArray:
        """kz_softmin_list_rows / kz_softmin_csr_rows -> float64 [n_q] on the device: per row the soft-min at temperature `eps` over
        the row's PAIRS of (dist - off[ind]), plus `shift`.  `off`: a float64 DeviceArray [n_target] or None.  A row without a pair
        gives NaN; the bits of a row do not depend on the other rows of the call.  The summation tree differs by layout: fixed width
        the tree of k, a CSR row the one `softmin_list_cols` gives a column of as many entries -- the same bits as that call on the
        view (colptr = indptr, col_row = ind, col_val = dist)."""
        self.require_f64()
        if off is not None:
            _f64_vector("off", off, self.n_target)
        out = self.ctx.empty((self.n_q,), np.float64)
        self._call("softmin_rows", self.n_target, float(eps), off.ptr if off is not None else None, float(shift), out.ptr)
        return out

    def sinkhorn(self, eps: float, n_iter: int, tol: Optional[float] = None) -> Tuple[DeviceArray, DeviceArray, int, Optional[float]]:
        """kz_sinkhorn_lists / kz_sinkhorn_csr -> (f float64 [n_q], g float64 [n_target], iterations done, last measured change of g or
        None): the Sinkhorn iteration of `softmin_list_cols` on `transpose`'s view and `softmin_rows` from f = 0, queued at once, the
        stopping rule (`tol`; None: none) decided on the device."""
        ctx = self.require_f64().ctx
        f, g = ctx.empty((self.n_q,), np.float64), ctx.empty((self.n_target,), np.float64)
        done, change, measured = C.c_int(0), C.c_double(0.0), C.c_int(0)
        self._call("sinkhorn", self.n_target, float(eps), int(n_iter), -1.0 if tol is None else float(tol), f.ptr, g.ptr, C.byref(done),
                   C.byref(change), C.byref(measured))
        return f, g, int(done.value), float(change.value) if measured.value else None

    def components(self, sizes: bool = False):
        """kz_components_lists / kz_components_csr -> (source_label int64 [n_q], target_label int64 [n_target], n_components) on the
        device, with `sizes` the int64 arrays (n_source_in, n_target_in) [n_components] in front of the count: the connected
        components of the bipartite graph whose edges are the pairs (fixed width: any k >= 1), numbered in the order of their smallest
        node, source rows before target rows.  More than COMPONENTS_MAX_NODES rows raise NotImplementedError."""
        ctx, n_q, n_t = self.ctx, self.n_q, self.n_target
        label_q, label_t = ctx.empty((n_q,), np.int64), ctx.empty((n_t,), np.int64)
        room = n_q + n_t if sizes and 1 <= n_q + n_t <= COMPONENTS_MAX_NODES else 0
        size_q = ctx.empty((room,), np.int64) if sizes else None
        size_t = ctx.empty((room,), np.int64) if sizes else None
        count = _I64(0)
        self._call("components", n_t, label_q.ptr, label_t.ptr, size_q.ptr if sizes else None, size_t.ptr if sizes else None, C.byref(count))
        n = int(count.value)
        if not sizes:
            return label_q, label_t, n
        return label_q, label_t, size_q.view_rows(0, n), size_t.view_rows(0, n), n

    def forest(self):
        """kz_forest_lists / kz_forest_csr -> (source int64 [m], target int64 [m], value float64 [m], entry int64 [m], n_components,
        rounds): the minimum spanning forest of the weighted pair graph on the device, its m = n_q + n_target - n_components edges
        ascending by (the order key of the value, the entry's flat position `entry`); an entry with a NaN value is no edge.  The
        components of the pairs with value <= t are those of the forest's edges with value <= t (`components_edges` on that prefix);
        `rounds` counts the Boruvka rounds that joined something.  The same bytes from every run.  More than COMPONENTS_MAX_NODES
        rows raise NotImplementedError."""
        ctx, n_q, n_t = self.ctx, self.n_q, self.n_target
        room = max(n_q + n_t - 1, 1) if n_q + n_t <= COMPONENTS_MAX_NODES else 1
        source, target, entry = (ctx.empty((room,), np.int64) for _ in range(3))
        value = ctx.empty((room,), np.float64)
        m, count, rounds = _I64(0), _I64(0), C.c_int(0)
        name = self.FOREST[self.is_csr]
        _check(getattr(ctx.lib, name)(*self._head(dtype=True), n_t, source.ptr, target.ptr, value.ptr, entry.ptr, C.byref(m), C.byref(count),
                                      C.byref(rounds)), name)
        m = int(m.value)
        return source.view_rows(0, m), target.view_rows(0, m), value.view_rows(0, m), entry.view_rows(0, m), int(count.value), int(rounds.value)


def components_edges(ctx: Context, source: DeviceArray, target: DeviceArray, n_source: int, n_target: int, sizes: bool = False,
                     count: Optional[int] = None):
    """kz_components_edges -> what `PairList.components` returns, for the first `count` (default: all) edges of the int64 arrays
    (source[e], target[e]): any order, an edge may repeat, an edge with an id out of range is no pair."""
    for what, a in (("source", source), ("target", target)):
        if not isinstance(a, DeviceArray) or len(a.shape) != 1 or a.dtype != np.int64:
            raise ValueError(f"{what} must be a 1-D int64 DeviceArray, got {getattr(a, 'dtype', type(a).__name__)} {getattr(a, 'shape', '')}")
    if source.shape != target.shape:
        raise ValueError(f"source and target must be of one length, got {source.shape} and {target.shape}")
    count = source.shape[0] if count is None else int(count)
    if not 0 <= count <= source.shape[0]:
        raise ValueError(f"count = {count} is outside [0, {source.shape[0]}]")
    n_q, n_t = int(n_source), int(n_target)
    label_q, label_t = ctx.empty((n_q,), np.int64), ctx.empty((n_t,), np.int64)
    room = n_q + n_t if sizes and 1 <= n_q + n_t <= COMPONENTS_MAX_NODES else 0
    size_q = ctx.empty((room,), np.int64) if sizes else None
    size_t = ctx.empty((room,), np.int64) if sizes else None
    n = _I64(0)
    _call(ctx, "kz_components_edges", source.ptr, target.ptr, count, n_q, n_t, label_q.ptr, label_t.ptr, size_q.ptr if sizes else None,
          size_t.ptr if sizes else None, C.byref(n))
    n = int(n.value)
    if not sizes:
        return label_q, label_t, n
    return label_q, label_t, size_q.view_rows(0, n), size_t.view_rows(0, n), n


# ---- the calls of `PairList` by name and layout, as tests and tools take them ---------------------------------------------------
def match_lists(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int) -> Tuple[DeviceArray, DeviceArray, int]:
    return PairList.lists(ctx, dist, ind, n_index).match()


def match_csr(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int) -> Tuple[DeviceArray, DeviceArray, int]:
    return PairList.csr(ctx, indptr, ind, dist, n_index).match()


def match_values(ctx: Context, dist: DeviceArray, col: DeviceArray) -> DeviceArray:
    return PairList.lists(ctx, dist, None, None).values(col)


def match_values_csr(ctx: Context, indptr: DeviceArray, dist: DeviceArray, col: DeviceArray) -> DeviceArray:
    return PairList.csr(ctx, indptr, None, dist, None).values(col)


def assign_lists(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int, unmatched_cost: float, eps: float, max_rounds: int,
                 tail_rows: int = 0, want_prices: bool = False):
    return PairList.lists(ctx, dist, ind, n_index).assign(unmatched_cost, eps, max_rounds, tail_rows, want_prices)


def assign_csr(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int, unmatched_cost: float, eps: float,
               max_rounds: int, tail_rows: int = 0, want_prices: bool = False):
    return PairList.csr(ctx, indptr, ind, dist, n_index).assign(unmatched_cost, eps, max_rounds, tail_rows, want_prices)


def assign_range(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int):
    return PairList.lists(ctx, dist, ind, n_index).value_range()


def assign_range_csr(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int):
    return PairList.csr(ctx, indptr, ind, dist, n_index).value_range()


def lists_transpose(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int) -> ListsTransposed:
    return PairList.lists(ctx, dist, ind, n_index).transpose()


def csr_transpose(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int) -> ListsTransposed:
    return PairList.csr(ctx, indptr, ind, dist, n_index).transpose()


def softmin_list_rows(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int, eps: float, off: Optional[DeviceArray] = None,
                      shift: float = 0.0) -> DeviceArray:
    return PairList.lists(ctx, dist, ind, n_index).softmin_rows(eps, off, shift)


def softmin_csr_rows(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int, eps: float,
                     off: Optional[DeviceArray] = None, shift: float = 0.0) -> DeviceArray:
    return PairList.csr(ctx, indptr, ind, dist, n_index).softmin_rows(eps, off, shift)


def sinkhorn_lists(ctx: Context, dist: DeviceArray, ind: DeviceArray, n_index: int, eps: float, n_iter: int,
                   tol: Optional[float] = None) -> Tuple[DeviceArray, DeviceArray, int, Optional[float]]:
    return PairList.lists(ctx, dist, ind, n_index).sinkhorn(eps, n_iter, tol)


def sinkhorn_csr(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int, eps: float, n_iter: int,
                 tol: Optional[float] = None) -> Tuple[DeviceArray, DeviceArray, int, Optional[float]]:
    return PairList.csr(ctx, indptr, ind, dist, n_index).sinkhorn(eps, n_iter, tol)


def components_lists(ctx: Context, ind: DeviceArray, n_target: int, sizes: bool = False):
    return PairList.lists(ctx, None, ind, n_target).components(sizes)


def components_csr(ctx: Context, indptr: DeviceArray, ind: DeviceArray, n_target: int, sizes: bool = False):
    return PairList.csr(ctx, indptr, ind, None, n_target).components(sizes)


def softmin_list_cols(ctx: Context, view: ListsTransposed, eps: float, off: Optional[DeviceArray] = None, shift: float = 0.0) -> DeviceArray:
    """kz_softmin_list_cols -> float64 [n_index] on the device: per column of the view `PairList.transpose` returned the soft-min over
    its entries of (col_val[p] - off[col_row[p]]), plus `shift`.  `off`: a float64 DeviceArray [n_q] or None.  A column without an
    entry gives NaN; the bits of a column depend on its entry count and SOFTMIN_LIST_CHUNK only."""
    if off is not None:
        _f64_vector("off", off, view.n_q)
    out = ctx.empty((view.n_index,), np.float64)
    _call(ctx, "kz_softmin_list_cols", view.colptr.ptr, view.col_row.ptr, view.col_val.ptr, view.n_index, view.nnz, float(eps),
          off.ptr if off is not None else None, float(shift), out.ptr)
    return out


# ---- neighbour pairs of both directions as a CSR (include/kiez_amd.h: KZ_PAIRS_*) ----------------------------------------------
PAIR_MODES = {"forward": 0, "reverse": 1, "union": 2, "mutual": 3}


def pair_mode(mode, what: str = "neighbor_pairs") -> str:
    """`mode` if it names one of the four set combinations, else ValueError -- on the host, before the device is touched."""
    if not isinstance(mode, str) or mode not in PAIR_MODES:
        raise ValueError(f"{what}: mode must be one of {tuple(PAIR_MODES)}, got {mode!r}")
    return mode


def _combine_call(ctx: Context, fwd_ind, rev_ind, n_q: int, k_f: int, n_index: int, k_r: int, mode: int, capacity: int):
    """One kz_lists_combine call -> (indptr [n_q + 1], ind [capacity], total)."""
    indptr = ctx.empty((n_q + 1,), np.int64)
    ind = ctx.empty((capacity,), np.int64)
    total = _I64(0)
    _call(ctx, "kz_lists_combine", fwd_ind.ptr if fwd_ind is not None else None, n_q, k_f, rev_ind.ptr if rev_ind is not None else None, n_index, k_r,
          mode, capacity, indptr.ptr, ind.ptr, C.byref(total))
    return indptr, ind, int(total.value)


def lists_combine(ctx: Context, fwd_ind: Optional[DeviceArray], rev_ind: Optional[DeviceArray], mode: str, n_q: Optional[int] = None,
                  n_index: Optional[int] = None, capacity: Optional[int] = None) -> Tuple[DeviceArray, DeviceArray, int]:
    """kz_lists_combine -> (indptr int64 [n_q + 1], ind int64, total): the pairs (source row, target row) of the forward lists
    `fwd_ind` [n_q, k_f] (target ids per source row), of the reverse lists `rev_ind` [n_index, k_r] (source ids per target row:
    "reverse", grouped by source row), of their union or of their intersection ("mutual"), every pair once, as a CSR over the source
    rows on the device, a row ascending by target id.  An id outside its range (-1, INT_MAX padding, >= n) is no pair; a repeated id
    counts once.  "forward" takes no `rev_ind` and "reverse" no `fwd_ind` (None); `n_q` / `n_index` default to the row count of the
    array that has them as rows.

    `capacity` None: the allocation policy -- ONE call with room for the obvious upper bound (the entries of the lists the mode reads;
    "mutual": of the smaller one), so that a second call is never needed -- unless that bound does not fit a quarter of what the
    device has free: then a count-only call and a second one with room for exactly the total, refused with MemoryError (naming the
    total) when that does not fit either.  ind comes back with `total` entries.  `capacity` given: that one call as the library
    makes it (`radius_neighbors`' contract: rows that end beyond the capacity are not written; indptr and total are exact)."""
    mode_c = PAIR_MODES[pair_mode(mode, "lists_combine")]
    use_f, use_r = mode != "reverse", mode != "forward"
    if use_f:
        shape = _list_ids("fwd_ind", fwd_ind)
        n_q = shape[0] if n_q is None else n_q
        if shape[0] != n_q:
            raise ValueError(f"fwd_ind has {shape[0]} rows, n_source is {n_q}")
    if use_r:
        shape = _list_ids("rev_ind", rev_ind)
        n_index = shape[0] if n_index is None else n_index
        if shape[0] != n_index:
            raise ValueError(f"rev_ind has {shape[0]} rows, n_target is {n_index}")
    if n_q is None or n_index is None:
        raise ValueError(f"lists_combine(mode={mode!r}): name n_source and n_target, the one list array does not say both")
    n_q, n_index = int(n_q), int(n_index)
    k_f = fwd_ind.shape[1] if use_f else 1
    k_r = rev_ind.shape[1] if use_r else 1
    args = (fwd_ind if use_f else None, rev_ind if use_r else None, n_q, k_f, n_index, k_r, mode_c)
    if capacity is not None:
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
            raise ValueError(f"capacity must be a non-negative integer, got {capacity!r}")
        return _combine_call(ctx, *args, int(capacity))
    n_f, n_r = (n_q * k_f if use_f else 0), (n_index * k_r if use_r else 0)
    bound = min(n_f, n_r) if mode == "mutual" else n_f + n_r
    free, _ = ctx.mem_info()
    first = bound if 8 * bound <= free // 4 else 0
    indptr, ind, total = _combine_call(ctx, *args, first)
    if total > first:
        del ind
        free, _ = ctx.mem_info()
        if 8 * total > free:
            raise MemoryError(f"lists_combine: total = {total} pairs need {8 * total} bytes of device memory for their ids (and as much "
                              f"again per value), {free} are free")
        indptr, ind, total = _combine_call(ctx, *args, total)
    return indptr, ind.view_rows(0, total), total


def pairs_values(ctx: Context, query: DeviceMatrix, index: DeviceMatrix, indptr: DeviceArray, ind: DeviceArray, kind: Optional[int] = None,
                 q_state=None, t_state=None) -> DeviceArray:
    """kz_pairs_values -> float64 [nnz] on the device: the value of every entry of the CSR (indptr [n_q + 1], ind [nnz]) between the
    query row that holds it and index row ind[p] -- the distance `knn` returns for the pair (`kind` None) or, with a `kind` of
    `gold_ranks_reduced` and its `q_state` / `t_state`, the hubness-reduced distance: the bits `radius_neighbors` returns for the
    pair, whether or not a neighbour list holds it."""
    pairs = PairList.csr(ctx, indptr, ind, None, index.shape[0])
    n_q, nnz = pairs.n_q, pairs.n_entries
    if kind is None:
        if q_state is not None or t_state is not None:
            raise ValueError("q_state / t_state belong to a reduced call: name its kind")
        kind_c, state = 0, (None, None, None, None)
    else:
        kind_c = int(kind)
        state = (None, None, None, None) if q_state is None or t_state is None else _reduction_state(q_state, t_state, n_q, index.shape[0])
    out = ctx.empty((nnz,), np.float64)
    _call(ctx, "kz_pairs_values", query.handle, index.handle, indptr.ptr, ind.ptr, n_q, nnz, kind_c, *state, out.ptr)
    return out


def csr_sort_rows(ctx: Context, indptr: DeviceArray, ind: DeviceArray, dist: DeviceArray, n_index: int):
    """kz_csr_sort_rows: every row of the float64 CSR ascending by (value, index row) in `knn_reduced`'s order, NaN last -- ind and
    dist permuted in place (`radius_neighbors`' row sort, a row of any length)."""
    pairs = PairList.csr(ctx, indptr, ind, dist, n_index).require_f64()
    _call(ctx, "kz_csr_sort_rows", indptr.ptr, pairs.n_q, pairs.n_entries, pairs.n_target, ind.ptr, dist.ptr)


def rank_stats(ctx: Context, rank: DeviceArray, ks):
    """kz_rank_stats -> ([#(0 <= rank < k) for k in ks], #(rank >= 0), sum(rank + 1), sum 1 / (rank + 1)) of an int64 rank vector."""
    n_k = len(ks)
    h_ks = (_I64 * max(n_k, 1))(*[int(k) for k in ks])
    h_hits = (_I64 * max(n_k, 1))()
    h_out = (C.c_double * 3)()
    _call(ctx, "kz_rank_stats", rank.ptr, rank.shape[0], h_ks, n_k, h_hits, h_out)
    return [int(h_hits[j]) for j in range(n_k)], int(h_out[0]), float(h_out[1]), float(h_out[2])


def split_self(ctx: Context, dist: DeviceArray, ind: DeviceArray, row0: int = 0):
    """kz_split_self: [n, K + 1] self-search without stripping -> ((rev_dist, rev_ind), (fwd_dist, fwd_ind)), each [n, K]."""
    n, k1 = dist.shape
    outs = [ctx.empty((n, k1 - 1), np.float64), ctx.empty((n, k1 - 1), np.int64), ctx.empty((n, k1 - 1), np.float64),
            ctx.empty((n, k1 - 1), np.int64)]
    _call(ctx, "kz_split_self", dist.ptr, ind.ptr, n, int(k1), int(row0), outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr)
    return (outs[0], outs[1]), (outs[2], outs[3])


def row_stats(ctx: Context, dist, mean=False, std=False, last=False, alloc=None):
    alloc = alloc or ctx.empty
    m, s, l_ = (alloc((dist.shape[0],), np.float64) if want else None for want in (mean, std, last))
    _call(ctx, "kz_row_stats", _ptr(dist, "dist"), *dist.shape, _ptr(m), _ptr(s), _ptr(l_))
    return m, s, l_


def row_nanstats(ctx: Context, dist, alloc=None):
    """kz_row_nanstats -> (np.nanmean, np.nanstd) of every row, each [n]."""
    alloc = alloc or ctx.empty
    m, s = alloc((dist.shape[0],), np.float64), alloc((dist.shape[0],), np.float64)
    _call(ctx, "kz_row_nanstats", _ptr(dist, "dist"), *dist.shape, _ptr(m), _ptr(s))
    return m, s


def select_topk(ctx: Context, dist, ind, k: int, alloc=None):
    alloc = alloc or ctx.empty
    od, oi = alloc((dist.shape[0], k), np.float64), alloc((dist.shape[0], k), np.int64)
    _call(ctx, "kz_select_topk", _ptr(dist, "dist"), _ptr(ind, "ind"), *dist.shape, int(k), _ptr(od), _ptr(oi))
    return od, oi


# ---- the hubness reductions of candidate lists dist / ind [n, K] -> float64 [n, K], and DisSimLocal's three steps -----------------
def csls(ctx: Context, dist, ind, r_train, alloc=None):
    out = (alloc or ctx.empty)(tuple(dist.shape), np.float64)
    _call(ctx, "kz_csls", _ptr(dist, "dist"), _ptr(ind, "ind"), *dist.shape, _ptr(r_train, "r_train"), _ptr(out))
    return out


def local_scaling(ctx: Context, dist, ind, r_t, nicdm: bool, alloc=None):
    out = (alloc or ctx.empty)(tuple(dist.shape), np.float64)
    _call(ctx, "kz_local_scaling", _ptr(dist, "dist"), _ptr(ind, "ind"), *dist.shape, _ptr(r_t, "r_t"), int(nicdm), _ptr(out))
    return out


def mp_normal(ctx: Context, dist, ind, mu_t, sd_t, alloc=None):
    out = (alloc or ctx.empty)(tuple(dist.shape), np.float64)
    _call(ctx, "kz_mp_normal", _ptr(dist, "dist"), _ptr(ind, "ind"), *dist.shape, _ptr(mu_t, "mu_t"), _ptr(sd_t, "sd_t"), _ptr(out))
    return out


def mp_empiric(ctx: Context, dist, ind, dist_t2s, ind_t2s, alloc=None):
    out = (alloc or ctx.empty)(tuple(dist.shape), np.float64)
    _call(ctx, "kz_mp_empiric", _ptr(dist, "dist"), _ptr(ind, "ind"), *dist.shape, _ptr(dist_t2s, "dist_t2s"), _ptr(ind_t2s, "ind_t2s"),
          *dist_t2s.shape, _ptr(out))
    return out


def dsl_fit(ctx: Context, ind_t2s, sm: DeviceMatrix, tm: DeviceMatrix, t_begin: int = 0, alloc=None):
    out = (alloc or ctx.empty)((ind_t2s.shape[0],), np.float64)
    _call(ctx, "kz_dsl_fit", _ptr(ind_t2s, "ind_t2s"), *ind_t2s.shape, sm.handle, tm.handle, t_begin, _ptr(out))
    return out


def dsl_transform(ctx: Context, ind, qm: DeviceMatrix, q_begin: int, tm: DeviceMatrix, t2c, gmin, alloc=None):
    """kz_dsl_transform -> the values before `dsl_finalize`; `gmin`: the caller's one-element float64 buffer, initialised to +inf."""
    out = (alloc or ctx.empty)(tuple(ind.shape), np.float64)
    _call(ctx, "kz_dsl_transform", _ptr(ind, "ind"), *ind.shape, qm.handle, q_begin, tm.handle, _ptr(t2c, "t2c"), _ptr(out), _ptr(gmin, "gmin"))
    return out


def dsl_finalize(ctx: Context, out, min_value: float, squared: bool):
    _call(ctx, "kz_dsl_finalize", _ptr(out), math.prod(out.shape), float(min_value), int(squared))
    return out


# ---- k-occurrence and hits@k over a neighbour matrix ind int64 [n, cols] (analysis.py, evaluate.py) -------------------------------
def minmax_i64_2d(ctx: Context, ind, k: int) -> Tuple[int, int]:
    lo, hi = _I64(0), _I64(0)
    _call(ctx, "kz_minmax_i64_2d", _ptr(ind, "ind"), *ind.shape, int(k), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def k_occurrence(ctx: Context, ind, k: int, n_bins: int, alloc=None):
    kocc = (alloc or ctx.empty)((n_bins,), np.int64)
    _call(ctx, "kz_k_occurrence", _ptr(ind, "ind"), *ind.shape, int(k), n_bins, _ptr(kocc))
    return kocc


def kocc_stats(ctx: Context, kocc, thr: float, want_gini: bool) -> Tuple[float, ...]:
    st = (C.c_double * 10)()
    _call(ctx, "kz_kocc_stats", _ptr(kocc, "kocc"), kocc.shape[0], float(thr), int(want_gini), st)
    return tuple(float(x) for x in st)


def kocc_select(ctx: Context, kocc, mode: int, thr: float, alloc=None):
    """kz_kocc_select -> (ids int64 [n_bins], count): the `count` ids with kocc == 0 (mode 0) or kocc >= thr (mode 1), ascending."""
    out, cnt = (alloc or ctx.empty)((kocc.shape[0],), np.int64), _I64(0)
    _call(ctx, "kz_kocc_select", _ptr(kocc, "kocc"), kocc.shape[0], mode, float(thr), _ptr(out), C.byref(cnt))
    return out, int(cnt.value)


def hit_positions(ctx: Context, ind, gold, alloc=None):
    hist = (alloc or ctx.empty)((ind.shape[1] + 1,), np.int64)
    _call(ctx, "kz_hit_positions", _ptr(ind, "ind"), _ptr(gold, "gold"), *ind.shape, _ptr(hist))
    return hist


# ---- the library's own collectives (RCCL on the context's stream); buffers as above, sizes, offsets[r] and lengths[r] in bytes -----
def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(load().kz_comm_unique_id(buf), "kz_comm_unique_id")
    return buf.raw


def comm_create(ctx: Context, unique_id: bytes, rank: int, world: int):
    h = _P()
    _call(ctx, "kz_comm_create", C.create_string_buffer(bytes(unique_id), 128), rank, world, C.byref(h))
    return h


def comm_destroy(comm):
    load().kz_comm_destroy(comm)   # (status dropped: this runs from close() / __del__, where nothing can act on it)


def comm_broadcast(comm, buf, nbytes: int, root: int):
    _check(load().kz_comm_broadcast(comm, _ptr(buf, "buf"), nbytes, int(root)), "kz_comm_broadcast")


def comm_all_gather(comm, send, recv, nbytes: int):
    _check(load().kz_comm_all_gather(comm, _ptr(send, "send"), _ptr(recv, "recv"), nbytes), "kz_comm_all_gather")


def comm_all_to_all(comm, send, offsets, lengths, recv, recv_bytes: int):
    offs, lens = (C.c_size_t * len(offsets))(*offsets), (C.c_size_t * len(lengths))(*lengths)
    _check(load().kz_comm_all_to_all(comm, _ptr(send, "send"), offs, lens, _ptr(recv, "recv"), recv_bytes), "kz_comm_all_to_all")


def comm_all_reduce_min(comm, buf, count: int):
    _check(load().kz_comm_all_reduce_min_f64(comm, _ptr(buf, "buf"), count), "kz_comm_all_reduce_min_f64")


def cast_f32(ctx: Context, arr: DeviceArray) -> DeviceArray:
    out = ctx.empty(arr.shape, np.float32)
    _call(ctx, "kz_cast_f64_f32", arr.ptr, out.ptr, int(np.prod(arr.shape, dtype=np.int64)))
    return out


# ---- the tail of kneighbors in one launch, and one call per fit / kneighbors --------------------------------------------------------
HUB_NONE, HUB_CSLS, HUB_LS, HUB_NICDM, HUB_MP_NORMAL, HUB_MP_EMPIRIC = 0, 1, 2, 3, 4, 5   # KZ_HUB_*: 1 .. 4 are RANK_CSLS .. RANK_MP_NORMAL
FIT_SEARCH_NONE, FIT_SEARCH_DUAL, FIT_SEARCH_REVERSE, FIT_SEARCH_SPLIT = 0, 1, 2, 3       # FitInfo.search
FIT_TAIL_KNN, FIT_TAIL_FUSED, FIT_TAIL_EMPIRIC = 0, 1, 2                                  # FitInfo.tail
RESCALE_SELECT_FUSED_MAX_K = 128   # candidates per row the fused kernel takes; beyond, kz_rescale_select runs the kernel sequence itself


def _dtype_code(out_dtype) -> int:
    dt = np.dtype(out_dtype)
    if dt not in (np.float32, np.float64):
        raise ValueError(f"out_dtype must be float32 or float64, got {dt}")
    return KZ_F32 if dt == np.float32 else KZ_F64


def rescale_select(ctx: Context, dist, ind, k: int, kind: int, t_a=None, t_b=None, out_dtype=np.float64, alloc=None):
    """kz_rescale_select: rescale (`kind`: HUB_NONE .. HUB_MP_NORMAL, index-side state `t_a` / `t_b`) + `_sort` selection + output cast
    of candidate lists dist / ind [n, K] -> (dist `out_dtype` [n, k], ind int64 [n, k])."""
    alloc = alloc or ctx.empty
    code = _dtype_code(out_dtype)
    n, K = dist.shape
    cols = int(k) if 1 <= int(k) <= K else 1   # (a k the library refuses sizes nothing: the refusal is the library's, nothing is written)
    od, oi = alloc((n, cols), np.dtype(out_dtype)), alloc((n, cols), np.int64)
    _call(ctx, "kz_rescale_select", _ptr(dist, "dist"), _ptr(ind, "ind"), n, K, int(k), int(kind), _ptr(t_a, "t_a"), _ptr(t_b, "t_b"), code,
          _ptr(od), _ptr(oi))
    return od, oi


class Fitted:
    """kz_fitted: a whole fit in the library -- the reverse lists, the fit state of the reduction and, once they exist, the forward
    lists.  It borrows the two matrices (held here, so they outlive it) and is released by `close()` or garbage collection."""

    STATE = {"reverse_dist": (0, np.float64), "reverse_ind": (1, np.int64), "forward_dist": (2, np.float64), "forward_ind": (3, np.int64),
             "state_a": (4, np.float64), "state_b": (5, np.float64)}

    def __init__(self, ctx: Context, handle, source_m: DeviceMatrix, target_m: Optional[DeviceMatrix]):
        self.ctx, self.handle = ctx, handle
        self._matrices = (source_m, target_m)
        self.n_query = source_m.shape[0]
        self.n_candidates = self.info["n_candidates"]

    def kneighbors(self, k: int, out_dtype=np.float64, alloc=None):
        """kz_kneighbors -> (dist `out_dtype` [n_source, k], ind int64 [n_source, k]) on the device; 1 <= k <= n_candidates."""
        if not self.handle:
            raise ValueError("the fitted object has been closed")
        alloc = alloc or self.ctx.empty
        code = _dtype_code(out_dtype)
        cols = int(k) if 1 <= int(k) <= self.n_candidates else 1   # (a k the library refuses sizes nothing: the refusal is the library's)
        od, oi = alloc((self.n_query, cols), np.dtype(out_dtype)), alloc((self.n_query, cols), np.int64)
        _check(self.ctx.lib.kz_kneighbors(self.handle, int(k), code, _ptr(od), _ptr(oi)), "kz_kneighbors")
        return od, oi

    @property
    def info(self) -> dict:
        """kz_fitted_info as a dict: sizes, the plan that ran (`search`, `tail`, ...) and `stats_forward` / `stats_reverse`."""
        if not self.handle:
            raise ValueError("the fitted object has been closed")
        st = FitInfo()
        _check(self.ctx.lib.kz_fitted_info(self.handle, C.byref(st)), "kz_fitted_info")
        return st.as_dict()

    def state(self, name: str) -> Optional[DeviceArray]:
        """kz_fitted_state: a non-owning DeviceArray over one of `Fitted.STATE` (lists [rows, n_candidates], state vectors [rows]) that
        keeps this object alive; None where the object holds no such array (forward lists before they exist, a state the kind lacks)."""
        if not self.handle:
            raise ValueError("the fitted object has been closed")
        if name not in self.STATE:
            raise ValueError(f"unknown state {name!r}: one of {sorted(self.STATE)}")
        what, dtype = self.STATE[name]
        p, rows, cols = _P(), _I64(0), C.c_int(0)
        _check(self.ctx.lib.kz_fitted_state(self.handle, what, C.byref(p), C.byref(rows), C.byref(cols)), "kz_fitted_state")
        if not p.value:
            return None
        shape = (rows.value,) if what >= 4 else (rows.value, cols.value)
        return DeviceArray(self.ctx, shape, dtype, ptr=p.value, owner=self)

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self.ctx.lib.kz_fitted_destroy(h)
            except Exception:
                pass

    __del__ = close


def fit(ctx: Context, source_m: DeviceMatrix, target_m: Optional[DeviceMatrix], kind: int, K: int, shared_sweep: bool = True) -> Fitted:
    """kz_fit: the searches and the fit state of a hubness-reduced fit (`kind`: HUB_*; `target_m` None: single source) in one call."""
    h = _P()
    _call(ctx, "kz_fit", source_m.handle, target_m.handle if target_m is not None else None, int(kind), int(K), int(bool(shared_sweep)), C.byref(h))
    return Fitted(ctx, h, source_m, target_m)
