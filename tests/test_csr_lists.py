"""The CSR (ragged) form of the one-to-one, assignment and Sinkhorn steps, without a device: the argument errors of
`matching.one_to_one_csr` / `assignment_csr` / `sinkhorn_csr`, `matching.from_sparse` against a dense argsort, the header and
the symbol table, and the facade's new methods beside the unchanged list calls.  Everything here raises or returns before a device call."""
import re
from pathlib import Path

import numpy as np
import pytest

from kiez_amd import matching

ROOT = Path(__file__).resolve().parent.parent
CSR_SYMBOLS = ("kz_match_csr", "kz_match_values_csr", "kz_assign_csr", "kz_assign_range_csr", "kz_csr_transpose", "kz_softmin_csr_rows",
               "kz_sinkhorn_csr")
FUNCTIONS = (matching.one_to_one_csr, matching.assignment_csr, matching.sinkhorn_csr)


def _good():
    return np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]), np.array([0, 1, 2, 3, 0, 1, 2, 3]), np.array([0, 5, 5, 8])


@pytest.mark.parametrize("fn", FUNCTIONS, ids=lambda f: f.__name__)
def test_argument_errors_of_the_csr_form(fn):
    dist, ind, indptr = _good()
    with pytest.raises(ValueError, match="1-D"):                       # 2-D lists together with indptr
        fn(indptr, ind.reshape(2, 4), dist.reshape(2, 4), 4)
    with pytest.raises(ValueError, match="one length"):                # length mismatch
        fn(indptr, ind, dist[:7], 4)
    with pytest.raises(ValueError, match="never decrease"):            # non-monotone, inside bounds
        fn(np.array([0, 5, 3, 8]), ind, dist, 4)
    with pytest.raises(ValueError, match="start at 0"):                # wrong first entry
        fn(np.array([1, 5, 5, 8]), ind, dist, 4)
    with pytest.raises(ValueError, match="end at the number of entries 8"):   # wrong last entry: short, and past the arrays
        fn(np.array([0, 5, 5, 7]), ind, dist, 4)
    with pytest.raises(ValueError, match="end at the number of entries 8"):
        fn(np.array([0, 5, 5, 9]), ind, dist, 4)
    with pytest.raises(ValueError, match="integer row starts"):        # non-integer indptr
        fn(np.array([0.0, 5.0, 5.0, 8.0]), ind, dist, 4)
    with pytest.raises(ValueError, match="1-D array of n_source"):
        fn(np.zeros((2, 2), dtype=np.int64), ind, dist, 4)
    with pytest.raises(ValueError, match="integer row ids"):
        fn(indptr, ind.astype(np.float64), dist, 4)
    with pytest.raises(ValueError, match="n_target"):
        fn(indptr, ind, dist, 0)


def test_assignment_checks_eps_against_the_csr_values_before_the_device():
    dist, ind, indptr = _good()
    with pytest.raises(ValueError, match="2\\*\\*-40"):
        matching.assignment_csr(indptr, ind, dist, 4, eps=1e-30)


def test_from_sparse_is_the_dense_argsort_with_explicit_zeros_kept():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(5)
    n_s, n_t = 40, 30
    dense = np.round(rng.random((n_s, n_t)), 1)                        # (ties: the target row decides)
    stored = rng.random((n_s, n_t)) < 0.3
    stored[7] = False                                                  # an empty row
    stored[3, 4], dense[3, 4] = True, 0.0                              # an explicit zero is a pair of value 0
    r, c = np.nonzero(stored)
    S = sp.coo_matrix((dense[r, c], (r, c)), shape=(n_s, n_t))
    for M in (S, S.tocsr(), S.tocsc()):
        indptr, ind, dist = matching.from_sparse(M)
        assert indptr.dtype == np.int64 and ind.dtype == np.int64 and dist.dtype == np.float64
        np.testing.assert_array_equal(np.diff(indptr), stored.sum(axis=1))
        masked = np.where(stored, dense, np.inf)
        for i in range(n_s):
            want = np.argsort(masked[i], kind="stable")[:stored[i].sum()]          # by (value, target row)
            np.testing.assert_array_equal(ind[indptr[i]:indptr[i + 1]], want)
            np.testing.assert_array_equal(dist[indptr[i]:indptr[i + 1]], dense[i, want])
    assert 4 in ind[indptr[3]:indptr[4]] and dist[indptr[3]] == 0.0
    with pytest.raises(ValueError, match="scipy sparse"):
        matching.from_sparse(dense)


def test_every_csr_symbol_is_declared_and_bound_and_the_abi_is_still_7():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {s[0] for s in N.SYMBOLS}
    for name in CSR_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared in include/kiez_amd.h"
        assert name in bound, f"{name} has no ctypes prototype"
    assert re.search(r"#define KZ_ABI_VERSION 7\b", header) and N.ABI_VERSION == 7
    assert int(re.search(r"#define KZ_CSR_LONG_ROW (\d+)", header).group(1)) == N.CSR_LONG_ROW
    for fn in ("match_csr", "match_values_csr", "assign_csr", "assign_range_csr", "csr_transpose", "softmin_csr_rows", "sinkhorn_csr"):
        assert callable(getattr(N, fn))
    lib = N.load()
    for name in CSR_SYMBOLS:
        assert hasattr(lib, name), f"libkiez_amd.so does not export {name}"


def test_the_facade_gains_methods_and_the_list_calls_keep_their_signatures(monkeypatch):
    import inspect
    from kiez_amd import Kiez
    from kiez_amd import _native as N
    names = lambda f: list(inspect.signature(f).parameters)[1:]
    assert names(Kiez.match_radius) == ["radius", "reduced", "return_distance"]
    assert names(Kiez.match_radius_device) == ["radius", "reduced"]
    assert names(Kiez.assign_radius) == ["radius", "reduced", "return_distance", "unmatched_cost", "eps"]
    assert names(Kiez.assign_radius_device) == ["radius", "reduced", "unmatched_cost", "eps"]
    for f in (Kiez.match, Kiez.match_device, Kiez.assign, Kiez.assign_device, matching.one_to_one, matching.assignment, matching.sinkhorn_lists):
        assert "radius" not in inspect.signature(f).parameters and "indptr" not in inspect.signature(f).parameters
    for f in FUNCTIONS:
        assert list(inspect.signature(f).parameters)[:4] == ["indptr", "ind", "dist", "n_target"]

    def no_device(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    kz = Kiez()
    for call in (kz.match_radius, kz.match_radius_device, kz.assign_radius, kz.assign_radius_device):
        with pytest.raises(ValueError, match="NaN"):                   # radius_neighbors' own check, before anything else
            call(float("nan"))
        with pytest.raises(TypeError):
            call(True)
    with pytest.raises(ValueError, match="eps"):
        kz.assign_radius(0.1, eps=-1.0)
