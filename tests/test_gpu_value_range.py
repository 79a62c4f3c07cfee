"""Every search route on data far from unit scale (generators, cases and the checker: tests/value_regimes.py; their preconditions
are proven on the CPU by tests/test_value_regimes.py; tools/fuzz_values.py draws the same regimes at random).

The rounding bound that certifies a candidate set is built from magnitudes -- the fp16 image's centre and
power-of-two scale, the measured per-row residuals and their per-matrix maxima, the raw maxima of the float32 / split-bf16 bound.
Unit-scale `rand` / `randn` data, which is all the rest of the suite draws, gives every row about the same norm: a maximum over any
subset of the rows, an unmeasured clamp, a query norm in place of the index maximum all still bound it.  Here they do not:

  pow2(e)            both matrices times 2^e, e in {-66, -50, -40, -20, 20, 40, e_max}: indices equal the unscaled run and the oracle,
                     distances are the unscaled ones times exactly 2^e / 4^e / 1, bit for bit; and 2^-110, beyond the +-100 clamp of
                     the fp16 scale's exponent
  cosine_row_scales  every row times its own 2^U{-30..30}: indices and distance bits equal the unscaled run
  mismatch(r)        query or index times 2^r, r in {2, 3, 6, 10, 20}: oracle index for index, distances rtol 1e-9
  offset(c)          common centre c spreads from the origin, c in {1e2, 1e3, 1e4}: oracle index for index; 1e5: tie-tolerant
  outlier(m, where)  one row times 1e3 / 1e6 / 1e9 in the index, the query matrix or both; first, middle, last row, alone in a tile
  heavy_rows         row norms over 2^-6 .. 2^6, the lightest rows in the first tile
  limit              rows just under |x| = 1e15 are answered exactly, just over it is a ValueError that names the limit

Every case runs under precision 0, 2 and 1 (fp16 first pass, split-bf16, float32 operands), bit-identical; the widths 64, 200, 320,
768, 1536 and 400 put it on every build of the fp16 kernel and on the width whose first pass has float32 operands.  Every run asserts
max_err_ratio < 1: the largest |approximate key - exact key| of a re-ranked candidate over the bound that was used for it -- the
design's own claim, not a tuned number (unit-scale data stays under 0.6).  The reference for all of it is
oracle.kiez_oracle.knn_exact / kiez_pipeline in float64 (kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101,
kiez/hubness_reduction/base.py:33-50).

Pairs left out: the shared sweep and the hubness kinds run on the fit cases of value_regimes.fit_cases() (pow2, mismatch in both
directions, outlier in source and in target, offset(1e3)), not on cosine_row_scales / heavy_rows / limit -- the sweep shares the
images and the bound of the ordinary search, which those regimes cover; offset(1e5) has no k = 50 / dealt-image case (its
comparison is tie-tolerant already).

Largest max_err_ratio per regime and first-pass tier, measured on an MI355X (profiles/value_range_ratios.md):
  regime                               fp16 first pass  split-bf16  float32 operands
  pow2                                 0.247            0.015       0.022
  pow2(-110)                           0.215            0.000       0.004
  cosine_row_scales                    0.285            0.034       0.040
  mismatch                             0.490            0.021       0.074
  offset                               0.233            0.030       0.040
  offset(1e5)                          0.162            0.040       0.040
  outlier                              0.214            0.008       0.031
  heavy_rows                           0.067            0.006       0.004
  limit                                0.223            0.021       0.038
  clamped query rows                   0.286            -           -
  fits (CSLS, sweep / two searches)    0.279            -           -
  inherited centre and scale           0.420            -           -
(the bound is closest where a query is packed with the scale of a much smaller index: mismatch, query 2^10 times the index, 0.49)
"""
import os
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import value_regimes as V
from tests.golden_util import HUB, knife_edge_rows, knife_edge_topk_ok

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CASES = V.knn_cases()
FITS = V.fit_cases()


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("precision", 0), ("dual_force", 0), ("dual_stride", 1), ("short_ord_min_tiles", 48)):
        c.set_option(name, value)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_regime_through_the_three_tiers(ctx, case):
    problems, ratios, st = V.check_knn_case(ctx, case, routes=not os.environ.get("KZ_PRECISION"))   # (no tier pinned from outside)
    print("RATIO", case["regime"], case["id"], " ".join(f"{t}={r:.4f}" for t, r in sorted(ratios.items())),
          "first-pass-fail", st["n_first_pass_fail"], "escalated", st["n_escalated_rows"], "fallback", st["n_fallback_rows"],
          "lists", st["n_splits"], "x", st["list_len"])
    assert not problems, problems


def test_clamped_query_rows_keep_their_measured_residual(ctx):
    """mismatch, query 2^3 .. 2^20 times the index: the query is packed with the index's scale, its elements beyond 4 x the index's
    largest are clamped at +-65504 and the clamped part must be in the row's residual |r_q|.  The bound then sends such rows down
    (at 2^20 every one); computed from the value before the clamp the residual is ~0 and garbage keys are certified."""
    from kiez_amd import _native as N
    for r, d in V.CLAMP_CASES:
        q, y = V.clamp_inputs(r, d)
        dd, ii, st = N.knn(ctx, N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean"), 10)
        print("RATIO clamp", f"r={r} d={d} ratio={st['max_err_ratio']:.4f} first-pass-fail {st['n_first_pass_fail']}")
        assert st["first_pass"] == 2 and not V.stats_problems(st, len(q), "clamp"), st
        np.testing.assert_array_equal(ii.numpy(), V.oracle_knn(q, y, 10, "euclidean")[1])
        if r == 20:
            assert st["n_first_pass_fail"] > 0, st


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cosine", "manhattan"])
def test_rows_over_the_input_limit_are_refused_by_name(ctx, metric):
    """|x|^2 <= 1e30 is the input limit (scikit-learn accepts such rows): the MFMA metrics and one metric
    of the VALU kernel, from DeviceMatrix and from Kiez.fit, query side and index side."""
    from kiez_amd import Kiez
    from kiez_amd import _native as N
    for dtype in (np.float32, np.float64):
        q, y = V.limit(True, 100, 300, 64, dtype, 5)
        q_ok, _ = V.limit(False, 100, 300, 64, dtype, 5)
        with pytest.raises(ValueError, match=r"\|x\|\^2 > 1e30"):
            N.DeviceMatrix(ctx, y, metric)
        N.DeviceMatrix(ctx, q_ok, metric)          # just under: accepted
        for s, t in ((q_ok, y), (y, q_ok)):       # a hubness-reduced fit indexes both sides
            with pytest.raises(ValueError, match=r"\|x\|\^2 > 1e30"):
                Kiez(n_candidates=5, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness="CSLS").fit(s, t)
        # without a reduction fit() indexes the target only (as the reference does): an over-limit target is refused by fit(),
        # an over-limit source by the search that first uploads it
        with pytest.raises(ValueError, match=r"\|x\|\^2 > 1e30"):
            Kiez(n_candidates=5, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}).fit(q_ok, y)
        kz = Kiez(n_candidates=5, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}).fit(y, q_ok)
        with pytest.raises(ValueError, match=r"\|x\|\^2 > 1e30"):
            kz.kneighbors(5)


def _kiez(ctx, s, t, metric, hub, kw, shared, k=5, n_candidates=10):
    """(dist, ind, stats) of Kiez(...).fit(s, t).kneighbors(k) with the shared sweep forced (`dual_force` 1) or off (`dual_stride` 0)."""
    from kiez_amd import Kiez
    ctx.set_option("dual_force", 1)
    ctx.set_option("dual_stride", 1 if shared else 0)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kz = Kiez(n_candidates=n_candidates, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hub, hubness_kwargs=dict(kw))
            d, i = kz.fit(s, t).kneighbors(k)
        return d, i, kz.algorithm.last_stats, kz.algorithm.last_stats_reverse
    finally:
        ctx.set_option("dual_force", 0)
        ctx.set_option("dual_stride", 1)


@pytest.mark.parametrize("case", FITS, ids=lambda c: c["id"])
def test_shared_sweep_and_inherited_images_in_a_fit(ctx, case):
    """Kiez(hubness="CSLS") with the shared sweep forced against two searches, bit for bit, and against kiez_pipeline.  Without the
    sweep the fit searches target -> source first: the target is then packed with the SOURCE's centre and scale, and serves as the
    index of the second search with that image (2^10 / 2^20 times larger: clamped rows on the index side)."""
    from oracle import kiez_oracle as O
    s, t = V.make_fit(case)
    metric = case["metric"]
    d1, i1, st1, rev1 = _kiez(ctx, s, t, metric, "CSLS", {}, shared=True)
    d0, i0, st0, rev0 = _kiez(ctx, s, t, metric, "CSLS", {}, shared=False)
    # both fits go through kz_knn_dual (with `dual_stride` 0 it runs the two searches itself): the larger side is its query side,
    # `last_stats` that direction, `last_stats_reverse` the other one
    n_a, n_b = max(len(s), len(t)), min(len(s), len(t))
    for st, n_rows in ((st1, n_a), (rev1, n_b), (st0, n_a), (rev0, n_b)):
        print("RATIO fit", case["id"], f"dual={st['dual']} tier={V.TIER_NAMES[st['first_pass']]} ratio={st['max_err_ratio']:.4f}",
              "first-pass-fail", st["n_first_pass_fail"], "of", n_rows)
        assert st["n_first_pass_fail"] <= n_rows and not V.stats_problems(st, n_rows, "fit"), st
    assert st1["dual"] == 1 and rev1["dual"] == 1 and st0["dual"] == 0 and rev0["dual"] == 0, (st1, rev1, st0, rev0)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)
    od, oi = O.kiez_pipeline(s, t, 10, 5, metric, 2, "CSLS", {})
    np.testing.assert_array_equal(i0, oi)
    # (the suite's rtol; its absolute 1e-6 belongs to unit-scale data and is scaled with the values here)
    np.testing.assert_allclose(d0, od, rtol=1e-5, atol=1e-6 * float(np.abs(od).max()))
    if case["e"] is not None:       # the unscaled fit: same indices, CSLS times exactly 2^e / 4^e, through the sweep and without it
        e = case["e"]
        sb, tb = np.ldexp(s, -e).astype(case["dtype"]), np.ldexp(t, -e).astype(case["dtype"])
        for shared, (ds, is_) in ((True, (d1, i1)), (False, (d0, i0))):
            db, ib, stb, _ = _kiez(ctx, sb, tb, metric, "CSLS", {}, shared=shared)
            np.testing.assert_array_equal(is_, ib)
            np.testing.assert_array_equal(ds, db * np.float32(V.pow2_factor(metric, e)))
            if shared:
                assert stb["dual"] == st1["dual"] == 1, (stb, st1)


@pytest.mark.parametrize("r,d,dtype", V.REUSE_CASES)
def test_a_matrix_searched_with_an_inherited_centre_and_scale(ctx, r, d, dtype):
    """One index searched first by a same-scale query matrix and then by one 2^r times larger (it inherits the index's centre and
    scale); then the two directions between a matrix and one 2^r times larger, the small one first (the larger is packed with the
    small one's centre and then serves as the INDEX with that image: every row clamped)."""
    from kiez_amd import _native as N
    q, y, big = V.reuse_inputs(r, d, dtype)
    for metric in ("euclidean", "cosine"):
        ym = N.DeviceMatrix(ctx, y, metric)
        for name, x in (("same scale", q), ("larger", big)):
            xm = N.DeviceMatrix(ctx, x, metric)
            dd, ii, st = N.knn(ctx, xm, ym, 10)
            print("RATIO reuse", f"r={r} d={d} {metric} {name} ratio={st['max_err_ratio']:.4f} first-pass-fail {st['n_first_pass_fail']}")
            assert not V.stats_problems(st, len(x), name), st
            np.testing.assert_array_equal(ii.numpy(), V.oracle_knn(x, y, 10, metric)[1], err_msg=name)
        # xm = the larger matrix, packed with y's centre: now the index
        dd, ii, st = N.knn(ctx, ym, xm, 10)
        print("RATIO reuse", f"r={r} d={d} {metric} larger as index ratio={st['max_err_ratio']:.4f} first-pass-fail {st['n_first_pass_fail']}")
        assert not V.stats_problems(st, len(y), "larger as index"), st
        np.testing.assert_array_equal(ii.numpy(), V.oracle_knn(y, big, 10, metric)[1])
        np.testing.assert_allclose(dd.numpy(), V.oracle_knn(y, big, 10, metric)[0], rtol=1e-9, atol=0)


@pytest.mark.parametrize("e,metric,d", [(-40, "euclidean", 64), (40, "sqeuclidean", 200)])
@pytest.mark.parametrize("tag", ["none", "csls", "ls", "nicdm", "mp_normal", "dsl", "mp_empiric"])
def test_hubness_kinds_at_2_to_the_minus_40_and_2_to_the_40(ctx, tag, e, metric, d):
    """Six-way equivariance of the reference (tests/test_value_regimes.py): no reduction, CSLS and DSL times exactly 2^e / 4^e, LS,
    NICDM and MP-normal bit-identical to the unscaled fit.  MP-empiric's `+ 1e-6` fill is absolute: against the oracle at the scale
    itself.  (float32 outputs: the final cast commutes with a power of two.)"""
    from oracle import kiez_oracle as O
    hub, kw = HUB[tag]
    s0, t0 = V.base_pair(1500, 2000, d, np.float32, 53)
    s, t = np.ldexp(s0, e), np.ldexp(t0, e)
    ds, is_, _, _ = _kiez(ctx, s, t, metric, hub, kw, shared=True)
    if tag == "mp_empiric":
        od, oi, mid = O.kiez_pipeline(s, t, 10, 5, metric, 2, hub, kw, return_intermediates=True)
        keep = ~knife_edge_rows(mid["ind_s2t"])
        for r in np.flatnonzero(~keep):
            assert knife_edge_topk_ok(od[r], oi[r], ds[r], is_[r], r, 10, mid["ind_t2s"]), f"knife-edge row {r}"
        # A second knife edge that exists at large scale only: where `+ 1e-6` is below half an ulp of the reverse list's last distance
        # the fill IS that distance, and for a query i that is the last reverse neighbour of its candidate c the reference compares
        # d(s_i, t_c) of the forward pass with the SAME pair's value of the reverse pass -- equal in exact arithmetic, decided by the
        # last bit of its BLAS.  Such rows are the reference's own coin toss: left out (none at 2^-40, where the fill dominates).
        last_d, last_i = mid["dist_t2s"][:, -1], mid["ind_t2s"][:, -1]
        absorbed = last_d + 1e-6 == last_d
        cand = mid["ind_s2t"]
        toss = ((last_i[cand] == np.arange(len(cand))[:, None]) & absorbed[cand]).any(axis=1)
        print("mp_empiric: rows on the absorbed-fill knife edge:", int(toss.sum()), "of", len(toss))
        assert not (toss.any() and e < 0)
        # ... of the index comparison.  What is determinate about them is still checked: the neighbours come from the row's candidate
        # list, the values lie in [0, 1], and a returned candidate whose OWN reverse list does not end in the query (only that
        # candidate's count hangs on the coin toss) carries the oracle's value
        ends_in_query = (last_i[cand] == np.arange(len(cand))[:, None]) & absorbed[cand]
        for r in np.flatnonzero(toss & keep):
            assert set(is_[r]) <= set(cand[r]) and len(set(is_[r])) == len(is_[r]), r
            assert ((ds[r] >= 0.0) & (ds[r] <= 1.0)).all(), (r, ds[r])
            for pos, c in enumerate(is_[r]):
                j = int(np.flatnonzero(cand[r] == c)[0])
                if not ends_in_query[r, j]:
                    np.testing.assert_allclose(ds[r, pos], mid["transformed"][r, j], rtol=1e-5, atol=1e-6, err_msg=f"row {r} candidate {c}")
        keep &= ~toss
        np.testing.assert_array_equal(is_[keep], oi[keep])
        assert keep.sum() > 0.5 * len(keep)
        np.testing.assert_allclose(ds[keep], od[keep], rtol=1e-5, atol=1e-6)     # (values in [0, 1] at any scale)
        return
    db, ib, _, _ = _kiez(ctx, s0, t0, metric, hub, kw, shared=True)
    factor = V.pow2_factor(metric, e) if tag in ("none", "csls", "dsl") else 1.0
    np.testing.assert_array_equal(is_, ib)
    np.testing.assert_array_equal(ds, db * np.float32(factor))
    od, oi = O.kiez_pipeline(s0, t0, 10, 5, metric, 2, hub, kw)
    np.testing.assert_array_equal(ib, oi)


def test_the_draw_on_which_the_oracle_misorders_a_pair(ctx):
    """offset(1e5), d = 200, float64, seed 1036: the numpy oracle's expansion |q|^2 - 2 q.y + |y|^2 orders the 10th and 11th
    neighbour of row 320 against exact arithmetic although they are 2.3 ulps of |q|^2 + |y|^2 apart (proven on the CPU,
    tests/test_value_regimes.py) -- against THAT order the 2-ulp rule of the tie-tolerant comparison would fail a device that is
    right.  So this draw is compared with the order of the exact-difference squared distances (value_regimes.exact_order), under the
    same rule: a position may differ only inside a run of neighbours less than 2 ulps apart, in at most 5 % of the rows."""
    q, y = V.offset(V.OFFSET_TIES, 500, 4000, 200, np.float64, 1036)
    res = V.run_three(ctx, q, y, 10, "sqeuclidean")
    assert not V.three_problems(res, len(q), "run")
    ex = V.exact_order(q, y, 10, "sqeuclidean")
    needed, wrong = V.tie_tolerant_rows(q, y, 10, "sqeuclidean", ex, res[0][1])
    print("rows that differ from the exact order:", needed, "outside a run of near-ties:", wrong)
    assert not wrong and len(needed) <= 0.05 * len(q), (needed, wrong)
    np.testing.assert_array_equal(res[0][1][320], ex[320, :10])


def test_fixed_seed_slice_of_the_value_fuzzer():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz_values.py"), "20", "707"], capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    print(r.stdout)
    assert r.returncode == 0, tail
    assert "cases 20 bad 0" in r.stdout.splitlines()[-1], tail
