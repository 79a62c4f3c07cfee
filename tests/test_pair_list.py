"""`_native.PairList` without a device: every operation has ONE body that puts the layout's leading arguments in front of arguments
both layouts share -- so the two native symbols of an operation must agree in everything behind those heads --, and the module-level
functions the tests and tools call by layout keep their names and parameters."""
import inspect

import numpy as np
import pytest

from kiez_amd import _native as N

SYMBOLS = {name: argtypes for name, _, argtypes in N.SYMBOLS}


def _fake(shape, dtype):
    """A DeviceArray around an address nothing reads: no allocation, no context."""
    return N.DeviceArray(None, shape, dtype, ptr=64)


class _NoContext:
    handle = None


def _both_layouts():
    ctx = _NoContext()
    lists = N.PairList.lists(ctx, _fake((5, 3), np.float64), _fake((5, 3), np.int64), 7)
    csr = N.PairList.csr(ctx, _fake((6,), np.int64), _fake((15,), np.int64), _fake((15,), np.float64), 7)
    return lists, csr


def test_what_a_pair_list_says_about_itself():
    lists, csr = _both_layouts()
    assert (lists.is_csr, lists.n_q, lists.n_entries, lists.n_target, lists.dtype_code) == (False, 5, 15, 7, N.KZ_F64)
    assert (csr.is_csr, csr.n_q, csr.n_entries, csr.n_target, csr.dtype_code) == (True, 5, 15, 7, N.KZ_F64)
    f32 = N.PairList.lists(_NoContext(), _fake((2, 4), np.float32), None, None)
    assert (f32.n_q, f32.n_entries, f32.dtype_code) == (2, 8, N.KZ_F32)
    with pytest.raises(ValueError, match="float64"):
        f32.require_f64()
    ids = N.PairList.csr(_NoContext(), _fake((3,), np.int64), _fake((9,), np.int64), None, 4)
    assert (ids.n_q, ids.n_entries, ids.dist) == (2, 9, None)


def test_every_operation_has_a_method_and_both_symbols():
    assert sorted(N.PairList.OPS) == ["assign", "components", "match", "sinkhorn", "softmin_rows", "transpose", "value_range", "values"]
    for op, (lists_symbol, csr_symbol, _) in N.PairList.OPS.items():
        assert callable(getattr(N.PairList, op)), op
        assert lists_symbol in SYMBOLS and csr_symbol in SYMBOLS, op


@pytest.mark.parametrize("op", sorted(N.PairList.OPS))
def test_the_two_symbols_agree_behind_their_layout_heads(op):
    lists_symbol, csr_symbol, head = N.PairList.OPS[op]
    col = _fake((5,), np.int64)
    kwargs = {key: (col if key == "col" else flag) for key, flag in head.items()}
    lists, csr = _both_layouts()
    n_lists, n_csr = len(lists._head(**kwargs)), len(csr._head(**kwargs))
    assert n_csr == n_lists + 1                                                    # (indptr)
    tail_lists, tail_csr = SYMBOLS[lists_symbol][n_lists:], SYMBOLS[csr_symbol][n_csr:]
    assert tail_lists == tail_csr and len(tail_lists) >= 1, (op, tail_lists, tail_csr)
    # ... and the heads end the way `_head` builds them: the row count, then the width (k: int) or the entry count (nnz: int64)
    assert SYMBOLS[lists_symbol][n_lists - 2:n_lists] == [N._I64, N.C.c_int]
    assert SYMBOLS[csr_symbol][n_csr - 2:n_csr] == [N._I64, N._I64]


class _RecordingLib:
    """Stands in for the loaded library: every symbol returns KZ_OK and notes how many arguments it got."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


class _RecordingContext(_NoContext):
    def __init__(self):
        self.lib = _RecordingLib()

    def empty(self, shape, dtype):
        return _fake(shape, dtype)


METHOD_ARGS = {"match": (), "values": None, "assign": (1.0, 1e-3, 10), "value_range": (), "transpose": (), "softmin_rows": (0.05,),
               "sinkhorn": (0.05, 3), "components": (True,)}


@pytest.mark.parametrize("op", sorted(N.PairList.OPS))
def test_every_method_fills_the_argument_list_of_either_symbol(op):
    ctx = _RecordingContext()
    lists = N.PairList.lists(ctx, _fake((5, 3), np.float64), _fake((5, 3), np.int64), 7)
    csr = N.PairList.csr(ctx, _fake((6,), np.int64), _fake((15,), np.int64), _fake((15,), np.float64), 7)
    args = (_fake((5,), np.int64),) if op == "values" else METHOD_ARGS[op]
    getattr(lists, op)(*args)
    getattr(csr, op)(*args)
    lists_symbol, csr_symbol, _ = N.PairList.OPS[op]
    assert ctx.lib.calls == [(lists_symbol, len(SYMBOLS[lists_symbol])), (csr_symbol, len(SYMBOLS[csr_symbol]))]


# name -> parameter names, as the GPU suites and tools/ call them
FUNCTIONS = {
    "match_lists": ["ctx", "dist", "ind", "n_index"],
    "match_csr": ["ctx", "indptr", "ind", "dist", "n_index"],
    "match_values": ["ctx", "dist", "col"],
    "match_values_csr": ["ctx", "indptr", "dist", "col"],
    "assign_lists": ["ctx", "dist", "ind", "n_index", "unmatched_cost", "eps", "max_rounds", "tail_rows", "want_prices"],
    "assign_csr": ["ctx", "indptr", "ind", "dist", "n_index", "unmatched_cost", "eps", "max_rounds", "tail_rows", "want_prices"],
    "assign_range": ["ctx", "dist", "ind", "n_index"],
    "assign_range_csr": ["ctx", "indptr", "ind", "dist", "n_index"],
    "lists_transpose": ["ctx", "dist", "ind", "n_index"],
    "csr_transpose": ["ctx", "indptr", "ind", "dist", "n_index"],
    "softmin_list_rows": ["ctx", "dist", "ind", "n_index", "eps", "off", "shift"],
    "softmin_csr_rows": ["ctx", "indptr", "ind", "dist", "n_index", "eps", "off", "shift"],
    "softmin_list_cols": ["ctx", "view", "eps", "off", "shift"],
    "sinkhorn_lists": ["ctx", "dist", "ind", "n_index", "eps", "n_iter", "tol"],
    "sinkhorn_csr": ["ctx", "indptr", "ind", "dist", "n_index", "eps", "n_iter", "tol"],
    "components_lists": ["ctx", "ind", "n_target", "sizes"],
    "components_csr": ["ctx", "indptr", "ind", "n_target", "sizes"],
}
DEFAULTS = {"tail_rows": 0, "want_prices": False, "off": None, "shift": 0.0, "tol": None, "sizes": False}


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_the_module_level_functions_keep_their_parameters(name):
    params = inspect.signature(getattr(N, name)).parameters
    assert list(params) == FUNCTIONS[name]
    for p in params.values():
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert p.default == DEFAULTS.get(p.name, inspect.Parameter.empty), (name, p.name)
