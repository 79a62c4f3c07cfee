"""tests/analysis_restate.py against the reference's own golden hubness scores and against slower, more literal forms of itself:
the oracle is validated here, on the CPU, before tests/test_gpu_analysis_kernels.py judges a kernel by it."""
import json
import math

import numpy as np
import pytest

from tests import analysis_restate as AR
from tests.golden_util import GOLDEN


@pytest.fixture(scope="module")
def neighbors():
    return np.load(GOLDEN / "ref_nn_ind.npy")


@pytest.mark.parametrize("k", [2, 5, 10, 50])
def test_restatement_reproduces_the_reference_scores(k, neighbors):
    """The reference's expected_k{2,5,10,50}_hub_scores (1000 x 50 neighbour matrix, 1000 target samples, hub_size 2)."""
    exp = json.loads((GOLDEN / "ref_hub_scores.json").read_text())[str(k)]
    arrs = np.load(GOLDEN / "ref_hub_scores_arrays.npz")
    lo, hi = AR.minmax(neighbors, k)
    assert lo >= 0
    kocc = AR.k_occurrence(neighbors, k, max(neighbors.shape[0], hi + 1))
    m = AR.hubness_measures(kocc, k, 1000, hub_size=2.0)
    assert set(exp) <= set(m)
    for key, v in exp.items():
        assert m[key] == pytest.approx(v), key
    for key in ("antihubs", "hubs", "k_occurrence"):
        np.testing.assert_array_equal(m[key], arrs[f"k{k}__{key}"], err_msg=key)


def test_gini_sorted_form_against_the_double_loop():
    rng = np.random.default_rng(11)
    x = [int(v) for v in rng.integers(0, 1000, size=200)]
    x[3] = x[77] = 0
    x[5] = x[6]                                                   # ties
    want = sum(abs(a - b) for a in x for b in x)
    assert AR.gini_numerator(x) == want
    assert AR.kocc_stats(np.array(x), 7.5)["gini_num"] == want
    assert AR.gini_numerator([4]) == 0


def test_hit_positions_against_list_index():
    rng = np.random.default_rng(12)
    n, cols = 300, 7
    ind = rng.integers(0, 12, size=(n, cols)).astype(np.int64)    # few ids: the gold id is often there twice
    gold = rng.integers(0, 14, size=n).astype(np.int64)           # 12 and 13 are never there
    gold[::17] = AR.NO_GOLD
    want = [0] * (cols + 1)
    for r in range(n):
        if int(gold[r]) == AR.NO_GOLD:
            continue
        row = [int(v) for v in ind[r]]
        want[row.index(int(gold[r])) if int(gold[r]) in row else cols] += 1
    assert want[cols] > 0 and sum(want) == n - len(gold[::17])
    np.testing.assert_array_equal(AR.hit_positions(ind, gold), want)


def test_k_occurrence_minmax_and_select():
    ind = np.array([[0, 3, 9], [-1, 3, 9], [2, -5, 9]], dtype=np.int64)
    np.testing.assert_array_equal(AR.k_occurrence(ind, 2, 5), [1, 0, 1, 2, 0])
    with pytest.raises(ValueError):
        AR.k_occurrence(ind, 3, 9)
    np.testing.assert_array_equal(AR.k_occurrence(ind, 3, 10), [1, 0, 1, 2, 0, 0, 0, 0, 0, 3])
    assert AR.minmax(ind) == (-5, 9) and AR.minmax(ind, 2) == (-5, 3) and AR.minmax(ind, 1) == (-1, 2)
    kocc = np.array([0, 7, 8, 0, 15, 3])
    np.testing.assert_array_equal(AR.kocc_select(kocc, 0, 7.5), [0, 3])
    np.testing.assert_array_equal(AR.kocc_select(kocc, 1, 7.5), [2, 4])
    np.testing.assert_array_equal(AR.kocc_select(kocc, 1, 8.0), [2, 4])
    np.testing.assert_array_equal(AR.kocc_select(kocc, 1, 16.0), [])


def test_kocc_stats_on_a_literal_vector():
    kocc = np.array([3, 0, 5, 0, 2])                              # mean 2
    st = AR.kocc_stats(kocc, 3.0)
    assert [st[key] for key in AR.STAT_ORDER] == [10, 8.0, 18.0, 12.0, math.fsum(math.sqrt(v) for v in kocc), 5, 2, 8, 2, 52]
    assert st["mean"] == 2.0
    assert st["abs_terms"]["m3s"] == 44.0 and st["abs_terms"]["abs_dev"] == 8.0
    assert AR.sum_bound(5, 44.0) == 2.0 * 9 * 2.0 ** -53 * 44.0


def test_max_abs_diff_and_rank_stats():
    inf, nan = np.inf, np.nan
    assert AR.max_abs_diff([1.0, inf, 3.0], [2.5, inf, 3.0]) == 1.5
    assert AR.max_abs_diff([inf, nan], [inf, 1.0]) == 0.0
    assert AR.max_abs_diff([inf, 0.0], [-inf, 1.0]) == inf
    assert math.copysign(1.0, AR.max_abs_diff([-0.0], [0.0])) == 1.0
    hits, n_ranked, s, r, r_abs = AR.rank_stats([0, -1, 4, 1, -7], [0, 1, 2, 2 ** 62])
    assert (hits, n_ranked, s) == ([0, 1, 2, 3], 3, 8) and r == r_abs == math.fsum([1.0, 0.2, 0.5])
