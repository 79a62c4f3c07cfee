"""Sinkhorn and the inverted softmax over the whole index, the parts that need no GPU: the binding of kz_softmin_rows, kz_dual_shift
and kz_max_abs_diff, the new kind's number, the classes' construction and constructor errors, and the numpy restatement
(tests/sinkhorn_restate.py) against np.logaddexp and its own normalisation.  The device side: tests/test_gpu_sinkhorn.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sinkhorn_restate as SR

ROOT = Path(__file__).resolve().parent.parent


def test_symbols_are_declared_bound_and_exported():
    from kiez_amd import _native as N
    header = (ROOT / "include" / "kiez_amd.h").read_text()
    assert re.search(r"^#define KZ_RANK_DUAL 8\b", header, flags=re.M)
    assert N.RANK_DUAL == 8
    assert (N.RANK_CSLS, N.RANK_LS, N.RANK_NICDM, N.RANK_MP_NORMAL) == (1, 2, 3, 4)        # (the existing kinds keep their numbers)
    chunk = re.search(r"^#define KZ_SOFTMIN_CHUNK_ROWS (\d+)\b", header, flags=re.M)
    assert chunk and int(chunk.group(1)) == N.SOFTMIN_CHUNK
    source = (ROOT / "kiez_amd" / "csrc" / "kz_softmin.h").read_text()
    assert re.search(rf"constexpr int KZ_SOFTMIN_CHUNK = {N.SOFTMIN_CHUNK};", source)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {s[0]: s for s in N.SYMBOLS}
    lib = N.load()
    for name, n_args in (("kz_softmin_rows", 9), ("kz_dual_shift", 8), ("kz_max_abs_diff", 5)):
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in include/kiez_amd.h"
        assert len(bound[name][2]) == n_args
        assert hasattr(lib, name)
    assert len(bound["kz_gold_ranks_reduced"][2]) == 12 and len(bound["kz_knn_reduced"][2]) == 13      # (they keep their signatures)
    assert re.search(r"^#define KZ_ABI_VERSION 7$", (ROOT / "include" / "kiez_amd.h").read_text(), flags=re.M)
    assert N.ABI_VERSION == 7 and lib.kz_abi_version() == 7                                            # (purely additive)
    assert list(inspect.signature(N.softmin_rows).parameters) == ["ctx", "query", "index", "eps", "off", "shift", "q_begin", "q_count"]
    assert list(inspect.signature(N.dual_shift).parameters) == ["ctx", "dist", "ind", "f", "g"]
    assert list(inspect.signature(N.max_abs_diff).parameters) == ["ctx", "a", "b"]


def test_classes_construct_and_the_resolver_keeps_its_names():
    import kiez_amd
    from kiez_amd import InvertedSoftmax, Kiez, Sinkhorn, hubness_reduction_resolver
    from kiez_amd.hubness_reduction import HubnessReduction
    from kiez_amd.neighbors import SklearnNN
    assert hubness_reduction_resolver.options == {"no", "csls", "localscaling", "mutualproximity", "dissimlocal"}
    assert set(Kiez.show_hubness_options()) == hubness_reduction_resolver.options
    assert "Sinkhorn" in kiez_amd.__all__ and "InvertedSoftmax" in kiez_amd.__all__
    with pytest.raises(KeyError):
        Kiez(hubness="Sinkhorn")                                # (not a name: the class or an instance)
    kz = Kiez(n_candidates=7, hubness=Sinkhorn)
    assert isinstance(kz.hubness, Sinkhorn) and (kz.hubness.temperature, kz.hubness.n_iter, kz.hubness.tol) == (0.05, 10, None)
    assert kz.algorithm.n_candidates == 7
    kz = Kiez(hubness=Sinkhorn, hubness_kwargs={"temperature": 0.2, "n_iter": 3, "tol": 1e-4})
    assert (kz.hubness.temperature, kz.hubness.n_iter, kz.hubness.tol) == (0.2, 3, 1e-4)
    inst = Sinkhorn(temperature=1, n_iter=np.int64(4), tol=0, nn_algo=SklearnNN(n_candidates=5, metric="cosine"))
    assert Kiez(hubness=inst).hubness is inst and inst.n_iter == 4 and inst.tol == 0.0
    kz = Kiez(hubness=InvertedSoftmax, hubness_kwargs={"temperature": 0.5})
    assert isinstance(kz.hubness, InvertedSoftmax) and kz.hubness.temperature == 0.5
    inst = InvertedSoftmax(nn_algo=SklearnNN(n_candidates=5, metric="cosine"))
    assert Kiez(hubness=inst).hubness is inst and inst.temperature == 0.05
    for cls in (Sinkhorn, InvertedSoftmax):
        assert issubclass(cls, HubnessReduction) and cls._no_rank_reason is None and cls._device_native
        assert cls.fit is not HubnessReduction.fit and cls._forward_rank_state is not HubnessReduction._forward_rank_state
        # everything that ranks is the base class's
        for inherited in ("kneighbors", "kneighbors_device", "kneighbors_whole_index", "kneighbors_whole_index_device", "gold_ranks",
                          "gold_ranks_device"):
            assert getattr(cls, inherited) is getattr(HubnessReduction, inherited)
    assert "temperature = 0.05" in repr(Sinkhorn(nn_algo=SklearnNN(n_candidates=5))) and "Sinkhorn" in repr(Kiez(hubness=Sinkhorn))


def test_constructor_errors_come_before_the_device(monkeypatch):
    from kiez_amd import InvertedSoftmax, Kiez, Sinkhorn
    from kiez_amd import _native as N
    from kiez_amd.neighbors import NotFittedError, SklearnNN

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(N.Context, "get", classmethod(no_device))
    monkeypatch.setattr(N.Context, "__init__", no_device)
    nn = lambda: SklearnNN(n_candidates=5, metric="cosine")   # noqa: E731
    for cls in (Sinkhorn, InvertedSoftmax):
        for bad in (0, 0.0, -0.05, np.nan, np.inf, -np.inf, None, "0.1", True):
            with pytest.raises(ValueError, match="temperature"):
                cls(temperature=bad, nn_algo=nn())
            with pytest.raises(ValueError, match="temperature"):
                Kiez(hubness=cls, hubness_kwargs={"temperature": bad})
    for bad in (0, -1, 2.5, 10.0, "10", None, True):
        with pytest.raises(ValueError, match="n_iter"):
            Sinkhorn(n_iter=bad, nn_algo=nn())
    for bad in (-1e-9, -1, np.nan, "0.1", True):
        with pytest.raises(ValueError, match="tol"):
            Sinkhorn(tol=bad, nn_algo=nn())
    with pytest.raises(ValueError, match="single candidate"):                  # (the base class's own check still holds)
        Sinkhorn(nn_algo=SklearnNN(n_candidates=1))
    # a single-source fit is refused before anything is indexed; an unfitted instance has no potentials
    for cls in (Sinkhorn, InvertedSoftmax):
        hub = cls(nn_algo=nn())
        with pytest.raises(ValueError, match="two-sided data only"):
            hub.fit(np.zeros((4, 3)))
        with pytest.raises(ValueError, match="two-sided data only"):
            Kiez(hubness=cls).fit(np.zeros((4, 3)))
        assert not hasattr(hub.nn_algo, "source_index")
        with pytest.raises(NotFittedError):
            hub.source_potential_
        with pytest.raises(NotFittedError):
            hub.target_potential_
        with pytest.raises(NotFittedError):
            hub.transform(np.zeros((4, 2)), np.zeros((4, 2), dtype=np.int64), None)
        with pytest.raises(NotFittedError):
            hub.kneighbors_whole_index(2)
        with pytest.raises(NotFittedError):
            hub.gold_ranks(np.arange(4))


def test_restatement_is_logaddexp():
    rng = np.random.default_rng(3)
    for eps in (1e-3, 0.05, 1.0, 50.0):
        for base, spread in ((0.0, 1.0), (1000.0, 40.0)):
            x = base + spread * rng.standard_normal((7, 301))
            want = -eps * np.logaddexp.reduce(-x / eps, axis=1)
            got = SR.softmin(x, eps, axis=1)
            assert (np.abs(got - want) <= 1e-12 * (np.abs(want) + eps) + 4 * np.spacing(np.abs(want))).all(), (eps, base)
            np.testing.assert_array_equal(SR.softmin(x.T, eps, axis=0), got)
    # the limits: eps -> 0 is the minimum, a constant row of n entries is c - eps log n, a single entry is itself
    x = rng.standard_normal((5, 40))
    np.testing.assert_allclose(SR.softmin(x, 1e-9, axis=1), x.min(axis=1), rtol=0, atol=1e-7)
    np.testing.assert_allclose(SR.softmin(np.full((2, 8), 3.0), 0.5), 3.0 - 0.5 * np.log(8), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(SR.softmin(x[:, :1], 0.3), x[:, 0])
    # far from unit scale without the shift every term underflows: the restatement does not
    far = 1000.0 + 40.0 * rng.standard_normal(500)
    with np.errstate(divide="ignore"):
        assert np.isinf(-0.02 * np.log(np.exp(-far / 0.02).sum()))
    assert abs(SR.softmin(far, 0.02) - far.min()) < 1.0
    # special values
    nan, inf = np.nan, np.inf
    assert SR.softmin(np.array([nan, 2.0, nan]), 0.1) == 2.0
    assert SR.softmin(np.array([nan, inf, nan]), 0.1) == inf and SR.softmin(np.array([1.0, -inf, nan, -inf]), 0.1) == -inf
    assert SR.softmin(np.array([1.0, 1.0, inf]), 1.0) == 1.0 - np.log(2.0)


def test_restated_plan_is_normalised():
    """After a row step every row of P = exp(-w / eps) sums to 1; on the first fit case the columns have reached n_s / n_t."""
    s, t, gold = SR.alignment_case(200, 200, 0.3)
    assert s.shape == (200, 16) and t.shape == (200, 16) and sorted(gold.tolist()) == list(range(200))
    D = 1.0 - s @ t.T
    f, g = SR.sinkhorn_potentials(D, 0.1, 50)
    P = np.exp(-SR.w(D, f, g) / 0.1)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12
    assert np.abs(P.sum(axis=0) - 1.0).max() <= 1e-3
    np.testing.assert_array_equal(SR.w(D, f, g), (D - f[:, None]) - g[None, :])
    # rectangular: the columns approach n_s / n_t
    s, t, gold = SR.alignment_case(180, 257, 0.3)
    assert len(set(gold.tolist())) == 180 and gold.max() < 257
    D = 1.0 - s @ t.T
    f, g = SR.sinkhorn_potentials(D, 0.05, 50)
    P = np.exp(-SR.w(D, f, g) / 0.05)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12 and np.abs(P.sum(axis=0) - 180 / 257).max() <= 1e-2
    # the inverted softmax is the first column step without its constant
    g1 = SR.inverted_softmax_potential(D, 0.05)
    f1, g1c = SR.sinkhorn_potentials(D, 0.05, 1)
    np.testing.assert_allclose(g1c, g1 + 0.05 * np.log(180 / 257), rtol=0, atol=1e-15)
