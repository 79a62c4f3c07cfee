"""Branches of kz_knn_impl's route (kz_route.h decides, kz_knn.hip executes) that no other suite pins by its stats.  Covered
elsewhere and therefore not repeated here: the short-list route and the long-k route taken as lists of 16 (k = 111 .. 320:
test_gpu_short_lists.py), the wide route and the tier probe's verdicts (test_gpu_wide_route.py, test_gpu_gates.py), the
speculative rescue (test_gpu_spec_rescue.py), the long-k route on lists of 128 and the exact-only calls (test_gpu_large_k.py,
test_gpu_longk.py).  Left for this file:

  * a TIER CHANGE BETWEEN TWO CHUNKS while the short-list route is active -- the route goes back to the one long list
    (kz_route_to_long) for the second chunk, and the first chunk's 4096 uncertified rows take the ladder after the fact;
  * a MORE-LISTS re-search: a handful of rows a K' = 16 pass could not certify, searched again with more lists of 16;
  * a handful of rows left by a SPLIT-BF16 pass going straight to the exact kernels (no float32-operand sweep).

Every case: the neighbours and distances are those of a float64 brute force in numpy (oracle.knn_exact, the reference's
sklearn_nearest_neighbors.py:96-101), bit for bit; the route fields of kz_knn_stats are the values the commit before the route
header produced on an MI355X (recorded there, written out here as literals).  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RESET = (("chunk_rows", 0), ("eps_scale", 1.0), ("short_ord_min_tiles", 48), ("spec_rows", 64), ("precision", 0))
ROUTE_FIELDS = ("list_len", "first_pass", "wide_lists", "n_splits")
COUNT_FIELDS = ("n_escalated_rows", "n_spec_rows", "n_range_rows", "n_fallback_rows")


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in RESET:
        c.set_option(name, value)


def _uniform(n, d, seed):
    return np.random.default_rng(seed).random((n, d)).astype(np.float32)


def _crowded(n_q, n_i, d, n_rows, n_near, seed):
    """Uniform rows, except that n_near index rows lie within 1e-4 of one point and n_rows query rows within 1e-3 of it: the fp16 and
    bf16 keys of the near rows coincide to within their rounding bound, so a list of 16 cannot certify the 10 nearest of those
    queries (the 16th key is no farther than the 10th); in float32 / float64 all distances are distinct."""
    rng = np.random.default_rng(seed)
    q, y = rng.random((n_q, d)).astype(np.float32), rng.random((n_i, d)).astype(np.float32)
    point = rng.random(d)
    y[rng.choice(n_i, n_near, replace=False)] = (point + 1e-4 * rng.standard_normal((n_near, d))).astype(np.float32)
    q[rng.choice(n_q, n_rows, replace=False)] = (point + 1e-3 * rng.standard_normal((n_rows, d))).astype(np.float32)
    return q, y


def _check(ctx, q, y, k, expect):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    qm, ym = N.DeviceMatrix(ctx, q, "euclidean"), N.DeviceMatrix(ctx, y, "euclidean")
    d1, i1, st = N.knn(ctx, qm, ym, k)
    got = {f: st[f] for f in ROUTE_FIELDS}
    got.update({f + " > 0": st[f] > 0 for f in COUNT_FIELDS})
    print("route stats:", {f: st[f] for f in ROUTE_FIELDS + COUNT_FIELDS + ("n_first_pass_fail",)})
    od, oi = O.knn_exact(q, y, k, "euclidean")
    np.testing.assert_array_equal(i1.numpy(), oi)
    np.testing.assert_array_equal(d1.numpy(), od)
    assert got == expect, (got, st)


def test_tier_change_between_two_chunks_on_the_short_list_route(ctx):
    """k = 30 on 71 index tiles with ranges of >= 8 tiles: 6 lists of 16 instead of one of 64.  eps_scale = 1e9 leaves every row
    of the first chunk (4096 of 8192) uncertified: they take the ladder after the fact, the second chunk starts at the float32
    operands with the one list of 64 -- the geometry the statistics report."""
    ctx.set_option("short_ord_min_tiles", 8)
    ctx.set_option("chunk_rows", 4096)
    ctx.set_option("eps_scale", 1e9)
    _check(ctx, _uniform(8192, 32, 1), _uniform(9000, 32, 2), 30, EXPECT["tier change"])


def test_a_handful_of_rows_of_a_list_of_sixteen_pass_get_more_lists(ctx):
    """100 of 4096 rows whose 40 nearest index rows share their fp16 key: more than the speculative rescue covers (64), at most
    KZ_ESC_SHORT_MAX_ROWS -- searched again with four or more lists of 16, k + 48 entries selected."""
    q, y = _crowded(4096, 9000, 32, 100, 40, 3)
    _check(ctx, q, y, 10, EXPECT["more lists"])


def test_a_handful_of_rows_left_by_split_bf16_go_to_the_exact_kernels(ctx):
    """precision = 2: the first pass runs on the split-bf16 operands; the 20 rows it cannot certify (at most KZ_K_EXACT_DIRECT_ROWS)
    skip the float32-operand kernel.  spec_rows = 0: not answered by the speculative rescue before the count is known."""
    ctx.set_option("precision", 2)
    ctx.set_option("spec_rows", 0)
    q, y = _crowded(4096, 9000, 32, 20, 40, 4)
    _check(ctx, q, y, 10, EXPECT["exact direct"])


# (recorded on an MI355X from the commit before kz_route.h existed; the counts behind the flags there: 4096 escalated + 8192 rows
#  to the exact kernels through the range re-search / 105 escalated, none further / 25 rows to the exact kernels)
EXPECT = {
    "tier change": {"list_len": 64, "first_pass": 2, "wide_lists": 0, "n_splits": 8, "n_escalated_rows > 0": True, "n_spec_rows > 0": False,
                    "n_range_rows > 0": True, "n_fallback_rows > 0": True},
    "more lists": {"list_len": 16, "first_pass": 2, "wide_lists": 0, "n_splits": 8, "n_escalated_rows > 0": True, "n_spec_rows > 0": False,
                   "n_range_rows > 0": False, "n_fallback_rows > 0": False},
    "exact direct": {"list_len": 16, "first_pass": 1, "wide_lists": 0, "n_splits": 8, "n_escalated_rows > 0": False, "n_spec_rows > 0": False,
                     "n_range_rows > 0": False, "n_fallback_rows > 0": True},
}
