"""Sinkhorn / InvertedSoftmax with support="union": the potentials over the pairs of the forward AND the reverse candidate lists
(`neighbor_pairs(n_candidates, mode="union")`, kz_sinkhorn_csr).  Bit for bit against `matching.sinkhorn_csr` on that CSR, and
against the float64 numpy restatement of tests/sinkhorn_lists_restate.py (on the padded lists of the CSR) within the bracket
tests/test_gpu_sinkhorn_lists.py applies to it."""
import numpy as np
import pytest

from tests import csr_lists_restate as CR
from tests import sinkhorn_lists_restate as LR
from tests import sinkhorn_restate as SR
from tests.test_gpu_sinkhorn import FIT_CASES
from tests.test_gpu_sinkhorn_lists import _assert_in_bracket, _bits

pytestmark = pytest.mark.gpu

CASE = FIT_CASES[2]   # 300 x 300, eps 0.02, 100 iterations, noise 1.0
K = 5


def _kiez(hubness, K, metric="cosine", **kw):
    from kiez_amd import Kiez
    return Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=kw)


@pytest.fixture(scope="module")
def union_fit():
    """The 300 x 300 case of the list tests plus ONE target far from every source (of 4 096 random unit vectors the one whose largest
    cosine to a source is smallest): the
    fitted instance, the searches `fit` and `kneighbors(5)` ran, the union CSR, the restatement's potentials -- once; read-only."""
    from kiez_amd import Sinkhorn
    from kiez_amd import _native as N
    n_s, n_t, eps, L, noise = CASE
    s, t, gold = SR.alignment_case(n_s, n_t, noise)
    cand = np.random.default_rng(1).standard_normal((4096, s.shape[1]))
    cand /= np.linalg.norm(cand, axis=1, keepdims=True)
    far = cand[np.argmin((cand @ s.T).max(axis=1))]   # (largest cosine to any source: 0.47; no source has it among its 5 nearest)
    t = np.concatenate([t, far[None, :]])
    n_t += 1
    calls = []
    real_knn, real_dual = N.knn, N.knn_dual

    def knn(*a, **k):
        calls.append(("knn", a[3]))
        return real_knn(*a, **k)

    def knn_dual(*a, **k):
        calls.append(("dual", a[3]))
        return real_dual(*a, **k)
    N.knn, N.knn_dual = knn, knn_dual
    try:
        kz = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, support="union").fit(s, t)
        fit_calls = tuple(calls)
        cached_k, cd_dev, ci_dev = kz.algorithm._forward
        cd, ci = cd_dev.numpy(), ci_dev.numpy()
        d5, i5 = kz.kneighbors(5)
        all_calls = tuple(calls)
    finally:
        N.knn, N.knn_dual = real_knn, real_dual
    csr = kz.algorithm.neighbor_pairs(K, mode="union")
    pd, pi = CR.pad(*csr)
    f_want, g_want, _, _ = LR.sinkhorn_potentials(pd, pi, n_t, eps, L)
    hub = kz.hubness
    res = dict(s=s, t=t, gold=gold, n_t=n_t, csr=csr, cd=cd, ci=ci, d5=d5, i5=i5, f=hub.source_potential_, g=hub.target_potential_,
               f_want=f_want, g_want=g_want, pd=pd, pi=pi, fit_calls=fit_calls, all_calls=all_calls, cached_k=cached_k, n_iter_=hub.n_iter_,
               change=hub.potential_change_)
    for a in list(res.values()) + list(csr):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return kz, res


def test_union_potentials(union_fit):
    from kiez_amd import Sinkhorn, matching
    n_s, _, eps, L, _ = CASE
    kz, r = union_fit
    n_t, f, g = r["n_t"], r["f"], r["g"]
    indptr, ind, dist = r["csr"]
    # ONE shared sweep for fit + kneighbors, the forward lists left in the one-shot cache
    assert r["fit_calls"] == (("dual", K),) and r["all_calls"] == r["fit_calls"] and r["cached_k"] == K
    assert r["cd"].shape == r["ci"].shape == (n_s, K)
    # every target row lists K sources: every column of the union has at least K pairs, and g has no NaN at all
    per_target = np.bincount(ind, minlength=n_t)
    assert per_target.min() >= K and (np.diff(indptr) >= K).all() and dist.dtype == np.float64
    assert not np.isnan(g).any() and not np.isnan(f).any() and f.shape == (n_s,) and g.shape == (n_t,)
    assert r["n_iter_"] == L and r["change"] is not None
    # matching.sinkhorn_csr on neighbor_pairs(n_candidates, mode="union"): the class's potentials, bit for bit
    f2, g2, info = matching.sinkhorn_csr(indptr, ind, dist, n_t, temperature=eps, n_iter=L, return_info=True)
    np.testing.assert_array_equal(_bits(f2), _bits(f))
    np.testing.assert_array_equal(_bits(g2), _bits(g))
    assert info == {"n_iter": L, "potential_change": r["change"]}
    # the float64 restatement over the same pairs
    print("worst error of f:", _assert_in_bracket(f, r["f_want"], eps, f"f after {L} iterations", factor=2 * L), "of the bracket; of g:",
          _assert_in_bracket(g, r["g_want"], eps, f"g after {L} iterations", factor=2 * L))
    # kneighbors(5): the stable sort of (d - f) - g over the CANDIDATES with these potentials -- transform and the rest are unchanged
    w5, want_i5 = LR.topk_lists(LR.list_w(r["cd"], r["ci"], f, g), r["ci"], 5)
    np.testing.assert_array_equal(r["i5"], want_i5)
    np.testing.assert_array_equal(r["d5"], w5)
    # the planted far target: no source lists it -- NaN under "candidates", finite under "union"
    far = n_t - 1
    assert not (r["ci"] == far).any()
    cand = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, support="candidates").fit(r["s"], r["t"])
    g_cand = cand.hubness.target_potential_
    assert np.isnan(g_cand[far]) and np.isfinite(g[far])
    print("targets without a potential under 'candidates':", int(np.isnan(g_cand).sum()), "under 'union':", int(np.isnan(g).sum()))
    # hits@1, recorded beside candidates and the whole index (not a gate)
    index = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, support="index").fit(r["s"], r["t"])
    hits = {name: float((m.kneighbors(1)[1][:, 0] == r["gold"]).mean()) for name, m in (("union", kz), ("candidates", cand), ("index", index))}
    print("hits@1 at K = 5:", hits)
    # the whole-index calls read f and g as ever: position == rank, and no target ranks last for want of a potential
    wi_w, wi_i = kz.kneighbors_whole_index(10)
    assert not np.isnan(wi_w).any()
    for c in (0, 9):
        np.testing.assert_array_equal(kz.gold_ranks(np.ascontiguousarray(wi_i[:, c]), reduced=True), np.full(n_s, c))


def test_union_early_stopping(union_fit):
    from kiez_amd import Sinkhorn
    _, _, eps, L, _ = CASE
    _, r = union_fit
    tol = 1e-3
    _, _, done, change = LR.sinkhorn_potentials(r["pd"], r["pi"], r["n_t"], eps, L, tol=tol)
    assert 1 < done < L                                               # (the restated loop stops early: 1e-3 is reached)
    hub = _kiez(Sinkhorn, K, temperature=eps, n_iter=L, tol=tol, support="union").fit(r["s"], r["t"]).hubness
    print("iterations to 1e-3:", hub.n_iter_, "restated:", done, "change:", hub.potential_change_, "restated:", change)
    assert hub.n_iter_ == done and hub.potential_change_ <= tol
    # (a change is the difference of two g vectors, each within 2 L brackets of its restated value)
    assert abs(hub.potential_change_ - change) <= 4 * L * np.nanmax(SR.bracket(r["g_want"], eps))
    one = _kiez(Sinkhorn, K, temperature=eps, n_iter=1, tol=tol, support="union").fit(r["s"], r["t"]).hubness
    assert one.n_iter_ == 1 and one.potential_change_ is None


def test_inverted_softmax_on_the_union(union_fit):
    from kiez_amd import InvertedSoftmax
    from kiez_amd import _native as N
    n_s, _, eps, _, _ = CASE
    _, r = union_fit
    n_t = r["n_t"]
    kz = _kiez(InvertedSoftmax, K, temperature=eps, support="union").fit(r["s"], r["t"])
    hub = kz.hubness
    f, g = hub.source_potential_, hub.target_potential_
    np.testing.assert_array_equal(f, np.zeros(n_s))
    assert hub.n_iter_ == 1 and hub.potential_change_ is None and not np.isnan(g).any()
    # one column step over the union's transposed view
    ctx = N.Context.get()
    indptr, ind, dist = (ctx.to_device(a) for a in r["csr"])
    one = N.softmin_list_cols(ctx, N.csr_transpose(ctx, indptr, ind, dist, n_t), eps).numpy()
    np.testing.assert_array_equal(_bits(one), _bits(g))
    want = LR.inverted_softmax_potential(r["pd"], r["pi"], n_t, eps)
    print("worst error of g:", _assert_in_bracket(g, want, eps, "inverted softmax g over the union"), "of the bracket")
    cached_k = kz.algorithm._forward[0]
    d5, i5 = kz.kneighbors(5)
    w5, want_i5 = LR.topk_lists(LR.list_w(r["cd"], r["ci"], f, g), r["ci"], 5)
    assert cached_k == K
    np.testing.assert_array_equal(i5, want_i5)
    np.testing.assert_array_equal(d5, w5)
