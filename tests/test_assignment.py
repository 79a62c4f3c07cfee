"""The minimum-cost assignment, the part that needs no GPU: the numpy restatement of the auction (tests/assignment_restate.py)
against scipy's dense optimum -- cost <= optimum + n_q * eps, exactly equal on integer values -- and its certificate; the errors
`matching.assignment` and `Kiez.assign` raise before the device is touched; the header, the binding and ABI 7."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import assignment_restate as AR
from tests.test_match import random_lists

ROOT = Path(__file__).resolve().parent.parent

SHAPES = [(300, 300, 5), (500, 400, 10), (400, 600, 3), (64, 64, 64)]
KINDS = ["uniform", "hubs", "integer", "negative"]


def lists_of(kind, n_q, n_target, k, seed=0):
    """(dist, ind, eps | None) of one data kind; rows sorted by value."""
    rng = np.random.default_rng([seed, n_q, n_target, k])
    dist, ind = random_lists(rng, n_q, n_target, k)
    eps = None
    if kind == "hubs":        # every target has a spread of its own, over three decades: a few targets are near to everybody
        spread = 10.0 ** rng.uniform(-2.0, 1.0, n_target)
        dist = np.abs(dist) * spread[ind]
    elif kind == "integer":
        dist = rng.integers(0, 21, (n_q, k)).astype(np.float64)
        eps = 1.0 / (n_q + 1) * (1.0 - 2.0 ** -20)    # (strictly below 1 / (n_q + 1))
    elif kind == "negative":
        dist = -np.abs(dist) - 0.5
    order = np.argsort(dist, axis=1, kind="stable")
    return np.take_along_axis(dist, order, axis=1), np.take_along_axis(ind, order, axis=1), eps


@pytest.mark.parametrize("half", [False, True], ids=["u_default", "u_half_range"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_q,n_target,k", SHAPES)
def test_restatement_reaches_the_optimum(n_q, n_target, k, kind, half):
    dist, ind, eps = lists_of(kind, n_q, n_target, k)
    lo, hi = AR.value_range(dist, ind, n_target)
    u, eps = AR.defaults(dist, ind, n_target, u=lo + (hi - lo) / 2 if half else None, eps=eps)
    match, col, price, rounds, converged = AR.auction(dist, ind, n_target, u, eps)
    assert converged and rounds >= 1
    got, want = AR.cost(dist, ind, n_target, u, match, col), AR.optimum(dist, ind, n_target, u)
    print(f"{kind} {n_q} x {n_target} x {k} u = {u:.6g} eps = {eps:.3g}: rounds {rounds}, matched {np.count_nonzero(match >= 0)}, "
          f"cost - optimum = {got - want:.3g} (bound {n_q * eps:.3g})")
    if kind == "integer":
        assert got == want
    assert got - want <= n_q * eps
    assert AR.slack_violation(dist, ind, n_target, u, eps, match, col, price) == 0
    if half:
        assert (dist[match >= 0, col[match >= 0]] <= u).all()                 # u is a threshold too
    else:
        assert u == hi


def test_restatement_details():
    # two rows, one target: the smaller value wins whatever the row order; the loser stays out once the price has passed its margin
    ind = np.zeros((2, 1), dtype=np.int64)
    for dist, want in ((np.array([[1.0], [2.0]]), [0, -1]), (np.array([[2.0], [1.0]]), [-1, 0])):
        match, col, price, rounds, converged = AR.auction(dist, ind, 1, 5.0, 0.25)
        assert match.tolist() == want and converged
        assert price[0] > 3.0            # the loser's margin u - w = 3: it left when the price passed it
    # equal bids: the smallest row
    match, *_ = AR.auction(np.ones((3, 1)), np.zeros((3, 1), dtype=np.int64), 1, 2.0, 0.5)
    assert match.tolist() == [0, -1, -1]
    # a row is matched only if that is strictly better than staying out; values above u, NaN, inf and padding are no pairs
    dist = np.array([[1.0, 9.0], [1.0, 3.0], [np.nan, np.inf], [0.5, 0.5], [-np.inf, 0.0]])
    ind = np.array([[0, 1], [0, 1], [2, 2], [-1, 0x7fffffff], [3, 9]], dtype=np.int64)
    match, col, price, rounds, converged = AR.auction(dist, ind, 4, 1.0, 0.125)
    assert match.tolist() == [-1, -1, -1, -1, -1] and rounds == 1 and (price == 0).all() and converged
    match, col, *_ = AR.auction(dist, ind, 4, 3.0, 0.125)
    assert match.tolist() == [0, -1, -1, -1, -1] and col.tolist() == [0, -1, -1, -1, -1]      # row 1's 3.0 is not better than u = 3.0
    match, col, *_ = AR.auction(dist, ind, 4, 3.5, 0.125)
    assert sorted(match[:2].tolist()) == [0, 1]
    # the round cap: a valid matching, not converged
    dist, ind, _ = lists_of("uniform", 300, 300, 5)
    u, eps = AR.defaults(dist, ind, 300)
    match, col, price, rounds, converged = AR.auction(dist, ind, 300, u, eps, max_rounds=1)
    assert rounds == 1 and not converged
    AR.cost(dist, ind, 300, u, match, col)
    # no rows
    match, col, price, rounds, converged = AR.auction(np.zeros((0, 4)), np.zeros((0, 4), dtype=np.int64), 3, 1.0, 0.1)
    assert match.shape == (0,) and rounds == 0 and converged and (price == 0).all()


def test_entry_points_are_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kiez_amd.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+kz_assign_lists\s*\(([^)]*)\)", header)
    assert decl and decl.group(1).count(",") == 15
    assert re.sub(r"\s+", " ", decl.group(1)).startswith(
        "kz_ctx* ctx, const void* d_dist, int dist_dtype, const int64_t* d_ind, int64_t n_q, int k, int64_t n_index, "
        "double unmatched_cost, double eps, int64_t max_rounds, int tail_rows, int64_t* d_match, int64_t* d_col, double* d_price")
    bound = {s[0]: s for s in N.SYMBOLS}
    assert len(bound["kz_assign_lists"][2]) == 16 and bound["kz_assign_lists"][1] is ctypes.c_int
    assert bound["kz_assign_lists"][2][7] is ctypes.c_double and bound["kz_assign_lists"][2][8] is ctypes.c_double
    assert len(bound["kz_assign_range"][2]) == 10
    lib = N.load()
    assert hasattr(lib, "kz_assign_lists") and hasattr(lib, "kz_assign_range")
    assert lib.kz_abi_version() == N.ABI_VERSION == 7
    assert "kz_assign.hip" in (ROOT / "kiez_amd" / "csrc" / "Makefile").read_text()


def test_public_signatures():
    from kiez_amd import Kiez, matching
    sig = inspect.signature(matching.assignment)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("dist", inspect.Parameter.empty), ("ind", inspect.Parameter.empty), ("n_target", inspect.Parameter.empty),
        ("unmatched_cost", None), ("eps", None), ("max_rounds", 1_000_000), ("return_distance", True), ("return_prices", False),
        ("ctx", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    sig = inspect.signature(Kiez.assign)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("k", None), ("whole_index", False), ("return_distance", True), ("unmatched_cost", None), ("eps", None)]
    sig = inspect.signature(Kiez.assign_device)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("k", None), ("whole_index", False), ("unmatched_cost", None), ("eps", None)]


def test_argument_errors_come_before_the_device(monkeypatch):
    from kiez_amd import Kiez, NotFittedError
    from kiez_amd import _native as N
    from kiez_amd import matching

    def no_device(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N, "load", no_device)
    d, i = np.arange(12, dtype=np.float64).reshape(4, 3), np.zeros((4, 3), dtype=np.int64)
    for dist, ind, n_target in [(d[0], i[0], 5), (d, i[:, :2], 5), (d, i.astype(np.float64), 5), (d.astype(np.int64), i, 5), (d, i, 0),
                                (d, i, 2.0)]:                                  # the checks of one_to_one
        with pytest.raises(ValueError):
            matching.assignment(dist, ind, n_target)
    for kw in [{"unmatched_cost": np.inf}, {"unmatched_cost": np.nan}, {"unmatched_cost": "3"}, {"unmatched_cost": True},
               {"eps": 0.0}, {"eps": -1.0}, {"eps": np.inf}, {"eps": np.nan}, {"eps": "1e-3"},
               {"max_rounds": 0}, {"max_rounds": 2.5}, {"max_rounds": None}, {"max_rounds": True}]:
        with pytest.raises(ValueError, match=next(iter(kw))):
            matching.assignment(d, i, 5, **kw)
    # eps below 2**-40 of the value spread (11.0 here): a bid may fail to raise a price
    with pytest.raises(ValueError, match="2\\*\\*-40"):
        matching.assignment(d, i, 5, eps=11.0 * 2.0 ** -41)
    with pytest.raises(AssertionError, match="the device was touched"):       # (at the bound it goes to the device)
        matching.assignment(d, i, 5, eps=11.0 * 2.0 ** -40)
    with pytest.raises(AssertionError, match="the device was touched"):
        matching.assignment(d, i, 5)
    # the facade: option errors first, then the fit
    for kw in [{"unmatched_cost": np.inf}, {"eps": 0.0}, {"eps": "x"}]:
        with pytest.raises(ValueError, match=next(iter(kw))):
            Kiez().assign(3, **kw)
    with pytest.raises(NotFittedError):
        Kiez().assign(3)
    with pytest.raises(NotFittedError):
        Kiez(hubness="CSLS").assign_device(3)
