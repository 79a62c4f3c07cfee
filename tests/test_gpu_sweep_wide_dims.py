"""The count and emit sweeps at text-encoder widths, d = 497 .. 2048: gold_ranks / radius_neighbors / radius_counts (route="sweep") on
the wide-row builds (32 .. 64 slices, one workgroup per CU) and the parity-split kernel (80 .. 128 slices, kz_knn_cntx16.h).

The checks are those of the narrow widths (`check` of test_gpu_gold_ranks_sweep / test_gpu_radius_sweep): a plain numpy float64
reference whose data precondition is asserted on the CPU, route="exact" byte for byte, route_taken == 1, and on this benign data no
fallback rows, no overflow and max_err_ratio <= 1.

Shapes: 200 queries are a full tile plus a tile whose upper 64-query half holds 8 real rows (the parity-split kernel's pad-query
half); 4097 index rows end in a tile of one real row."""
import ctypes as C

import pytest

from tests.test_gpu_gold_ranks_sweep import check as check_ranks
from tests.test_gpu_radius_sweep import check as check_radius

pytestmark = pytest.mark.gpu
# every build once: 32, 40, 48, 56, 64 slices (wide rows), 80, 96, 112, 128 (parity split)
WIDTHS = list(zip((497, 640, 768, 896, 1024, 1025, 1536, 1792, 2048), ("euclidean", "sqeuclidean", "cosine") * 3))


@pytest.mark.parametrize("d,metric", WIDTHS)
def test_ranks_every_build(d, metric):
    check_ranks(200, 4097, d, metric, seed=d)


@pytest.mark.parametrize("d,metric", WIDTHS)
def test_radius_every_build(d, metric):
    check_radius(200, 4097, d, metric, seed=d)


@pytest.mark.parametrize("d", [768, 1536])
def test_index_of_one_tile_plus_one_row(d):
    check_ranks(200, 129, d, "cosine", seed=d)
    check_radius(65, 129, d, "cosine", seed=d)


@pytest.mark.parametrize("d,metric", [(896, "cosine"), (1792, "euclidean")])
def test_several_index_ranges_per_query_tile(d, metric):
    from kiez_amd import _native as N
    n, qt, pc, ln = C.c_int(0), (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    # (one workgroup on each of 256 CUs: the plan the sweep's launcher makes for these builds; 199 rows carry a gold id)
    for n_q in (199, 200):
        assert N.load().kz_knn_plan(n_q, 4097, 1, 256, 0, 1, C.byref(n), qt, pc, ln) == 0 and min(pc[:n.value]) >= 2
    check_ranks(200, 4097, d, metric, seed=d)
    check_radius(200, 4097, d, metric, seed=d)
