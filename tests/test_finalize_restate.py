"""tests/finalize_restate.py against what does not restate it.

  * the two list layouts: a launch's offsets are distinct and fill their region's block;
  * the verdict: approximate keys key_j + delta_j, |delta_j| <= eps, for ALL index rows, lists as a correct first pass leaves them
    (per range the KP best above the floor) -- then "certified => the candidates' float64 top-k is the whole index's, ties by id" must
    hold for every row and both builds' rules, and the cases must exercise both branches (20 % .. 80 % uncertified, at most 5 % of the
    rows within 0.05 eps of the verdict's edge): the same cases tests/test_gpu_finalize_direct.py runs on the kernels;
  * the crafted scenarios: each says what it is built to say, with |margin| >= 0.25, and its candidates' exact values are far apart
    outside the tie scenarios.
No GPU: the fp16 tier's bound is replaced by a number of the same size (its formula is checked against the kernel on the device).
"""
import numpy as np
import pytest

from tests import finalize_restate as R

TIE_SCENARIOS = ("all_equal", "dup_k")


@pytest.mark.parametrize("halves,contig", [(1, 1), (1, 0), (2, 0)])
@pytest.mark.parametrize("KP", [16, 128])
def test_list_offsets_fill_their_blocks(KP, halves, contig):
    lay = R.Layout([1, 3], [3, 5], halves, contig, KP)
    assert lay.base == [0, 128 * 3 * (KP if contig else 2 * KP)]
    seen = np.concatenate([lay.offsets(r) for r in range(3 * 128)])
    assert len(np.unique(seen)) == len(seen) and seen.min() == 0 and seen.max() < lay.n_list
    for r in (0, 127, 128, 383):
        o = lay.offsets(r)
        reg = lay.region(r)
        end = lay.base[reg + 1] if reg + 1 < len(lay.base) else lay.n_list
        assert len(o) == lay.entries(r) and lay.base[reg] <= o.min() and o.max() < end
    if contig or halves == 2:
        assert len(seen) == lay.n_list   # a bijection onto the whole block
    else:   # one list per (query, range) in a block of 64 columns: the columns of the second lane half stay unused
        assert len(seen) * 2 == lay.n_list and ((seen % 64) < 32).all()
    if not contig:   # the formula of the header: entry e of (row, piece, half h) at wave_base + e 64 + h 32 + row % 32
        assert lay.offsets(37)[KP * halves * 2 + 5] == lay.wave_base(37, 2) + 5 * 64 + 37 % 32
        assert lay.wave_base(128 + 37, 1) == lay.base[1] + ((37 >> 5) * 5 + 1) * KP * 64


def _tier_units(case, X, Y, K):
    """(eps per unit of the case's free factor, key scale, qref) per row.  Tier 0: the kernel's formula; tier 2 stand-in: the same size."""
    cosine = case.metric == "cosine"
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    y_max = float(np.sqrt((Y64 * Y64).sum(1)).max())
    unit = np.asarray([R.eps_tier0(1.0, float(np.sqrt((x * x).sum())), y_max, cosine) for x in X64])
    return unit, (2.0 ** -9 if case.tier == 2 else 1.0)


def _keys(case, X, Y):
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    V = R.exact_values(X, Y, case.metric)
    qref = (X.astype(np.float64) ** 2).sum(1)
    if tier_h and cosine:
        qref = np.ones(len(X))
    K = np.stack([R.exact_key(V[q], qref[q], cosine, tier_h) for q in range(len(X))])
    return V, qref, K


PROPERTY = [R.property_case(b, M) for b in R.PROPERTY_BUILDS for M in R.PROPERTY_M]


@pytest.mark.parametrize("case", PROPERTY, ids=repr)
def test_certified_rows_hold_the_whole_index_top_k(case):
    """The rows, seeds and (on the float32 tier) the eps of the GPU module's property cases of the same name."""
    M = case.geom(0)[0] * case.KP
    n_q, n_i = R.PROPERTY_ROWS, R.property_n_i(M)
    X, Y = R.property_data(1000 + M, n_q, n_i, case.d)
    V, qref, K = _keys(case, X, Y)
    unit, scale = _tier_units(case, X, Y, K)
    factor, rows = R.property_rows(K, unit, scale, case.geom(0), M, "wide" if case.build == R.BUILD_WIDE else "generic")
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    n_fail = {"generic": 0, "wide": 0}
    n_band = {"generic": 0, "wide": 0}
    for q, row in enumerate(rows):
        r = R.finalize_row(row["keys"], row["ids"], V[q], KP=case.KP, KS=case.KS, k=case.k, exclude_self=case.exclude_self, self_row=q, n_i=n_i,
                           eps=row["eps"], scale=scale, qref=qref[q], cosine=cosine, tier_h=tier_h,
                           list_floor=row["list_floor"] if row["list_floor"] > -R.INF else None, metric=case.metric)
        assert r["ratio"] <= 1.0
        want = R.brute_topk(V[q], case.k_eff)
        for build in ("generic", "wide"):
            if r["certified"][build]:
                assert np.array_equal(r["cand"][:case.k_eff], want), f"row {q} ({build}): certified, but not the whole index's top-k"
            else:
                n_fail[build] += 1
            n_band[build] += abs(r["margin"][build]) < 0.05
    build = "wide" if case.build == R.BUILD_WIDE else "generic"   # (the build the GPU module launches for this case)
    assert 0.2 * n_q <= n_fail[build] <= 0.8 * n_q, f"{build}: {n_fail[build]} of {n_q} rows uncertified"
    assert n_band[build] <= 0.05 * n_q, f"{build}: {n_band[build]} of {n_q} rows within 0.05 eps of the edge"


SCENARIO = [c for c in R.SCENARIO_CASES if c.elem == "float32" and c.d <= 64]


@pytest.mark.parametrize("case", SCENARIO, ids=repr)
def test_scenarios_say_what_they_are_built_to_say(case):
    n_q, n_i = 72, 2048
    Y, queries = R.scenario_data(7, n_q, n_i, case.d, case.metric)
    X = queries(None)
    V, qref, K = _keys(case, X, Y)
    unit, scale = _tier_units(case, X, Y, K)
    spread = K.max(1) - K.min(1)
    factor = 1e-3 * float(np.median(spread / unit))
    cosine, tier_h = case.metric == "cosine", case.tier == 2
    which = "wide" if case.build == R.BUILD_WIDE else "generic"
    seen = set()
    for q in range(n_q):
        region = q % 2
        geom = case.geom(region)
        names = R.scenario_names(geom, has_floor=case.floor, dual=case.dual, zero_level=not cosine)
        name = names[(q // 2) % len(names)]
        eps = factor * unit[q]
        min_gap = 200 * max(R.value_bound(X[q], y, case.d) for y in Y)

        def builder(q=q, eps=eps, geom=geom, min_gap=min_gap):
            return R.RowBuilder(V[q], qref[q], eps, scale, cosine, tier_h, geom, np.random.RandomState(q), min_gap=min_gap)
        row = R.scenario_or_fallback(builder, name, prefer=q, eps_pair=(eps, 2.0 * eps))
        name = row["name"]
        excl = row["excl_floor"] if row["excl_floor"] is not None else (np.float32(-R.INF) if case.dual else None)
        kw = dict(KP=case.KP, KS=case.KS, k=case.k, exclude_self=case.exclude_self, self_row=q, n_i=n_i, scale=scale, qref=qref[q], cosine=cosine,
                  tier_h=tier_h, list_floor=row["list_floor"], excl_floor=excl, metric=case.metric)
        r = R.finalize_row(row["keys"], row["ids"], V[q], eps=eps, **kw)
        assert r["certified"][which] == row["expect"], f"row {q}, {name}: margin {r['margin'][which]}, ratio {r['ratio']}"
        assert abs(r["margin"][which]) >= 0.25, f"row {q}, {name}: margin {r['margin'][which]}"
        if name == "violate":
            assert 1.5 <= r["ratio"] <= 1.56 and r["margin"][which] > 0.25
        else:
            assert r["ratio"] <= 0.96
        if name == "excl_between":   # the same lists under the reverse direction's larger eps: not certified
            r2 = R.finalize_row(row["keys"], row["ids"], V[q], eps=2.0 * eps, **kw)
            assert r["certified"][which] and not r2["certified"][which] and r2["margin"][which] <= -0.25
        if name not in TIE_SCENARIOS:
            gaps = np.diff(r["cval"])
            bound = max(R.value_bound(X[q], Y[j], case.d) for j in r["cand"])
            assert (gaps >= 100 * bound).all(), f"row {q}, {name}: exact values {gaps.min()} apart, bound {bound}"
        seen.add(name)
    assert seen == set(R.scenario_names(case.geom(0), has_floor=case.floor, dual=case.dual, zero_level=not cosine)) | set(
        R.scenario_names(case.geom(1), has_floor=case.floor, dual=case.dual, zero_level=not cosine))
