"""Where the fp16 sweep kernels copy their index slices from.  kz_knn_cand_h64_kernel addresses the LDS-DMA copy of a barrier by a
compile-time offset from the current index tile's first slice, per barrier position, half tile and tile parity (kz_knn_h64.h);
a wrong constant is a copy from the wrong slice: keys of other rows, or of other features.  Short index ranges that start and end
on odd and on even index tiles, odd and even slice counts, units with and without their second query tile, the 32-query kernel
beside the 64-query one, ordinary searches and the shared sweep -- indices and distance bits against the oracle and against the
other kernel.  Reference path: kiez/neighbors/exact/sklearn_nearest_neighbors.py:96-101 (kneighbors)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    yield c
    for name, value in (("h_q64", 2), ("dual_force", 0), ("force_splits", 0)):
        c.set_option(name, value)


# index rows -> tiles of 128 (ragged last tile), cut into ranges of at least 8 tiles by force_splits:
# (kz_plan.h: two ranges of ceil(tiles / 2) and the rest)
#   1029 = 9 tiles: one range [0, 9);   2048 = 16 tiles: [0, 8) + [8, 16): the second range starts on an EVEN tile;
#   2100 = 17 tiles: [0, 9) + [9, 17) and 2200 = 18 tiles: [0, 9) + [9, 18): it starts on an ODD tile; lengths 8 and 9 take both
#   exits of the two-body tile loop of an odd slice count; last tiles 8, 15, 16, 17 (2048 rows: a full last tile)
@pytest.mark.parametrize("n_i,splits", [(1029, 1), (2048, 2), (2100, 2), (2200, 2)])
@pytest.mark.parametrize("d", [64, 72, 128, 200])   # 4, 5, 8, 13 slices
def test_short_ranges_on_both_tile_parities(ctx, d, n_i, splits):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    rng = np.random.RandomState(1000 * d + n_i)
    y = rng.rand(n_i, d).astype(np.float32)
    q3 = rng.rand(300, d).astype(np.float32)   # three query tiles: the second 64-query unit has no second tile
    ym = N.DeviceMatrix(ctx, y, "euclidean")
    od, oi = O.knn_exact(q3, y, K, "euclidean")
    od_r, oi_r = O.knn_exact(y, q3, K, "euclidean")
    ctx.set_option("force_splits", splits)
    for n_q in (100, 300):   # one query tile, three
        qm = N.DeviceMatrix(ctx, q3[:n_q], "euclidean")
        got = {}
        for q64 in (0, 1):
            ctx.set_option("h_q64", q64)
            ctx.set_option("dual_force", 0)
            dist, ind, st = N.knn(ctx, qm, ym, K)
            assert st["first_pass"] == 2, st
            np.testing.assert_array_equal(ind.numpy(), oi[:n_q], err_msg=f"h_q64 {q64}, {n_q} queries")
            np.testing.assert_array_equal(dist.numpy(), od[:n_q], err_msg=f"h_q64 {q64}, {n_q} queries")
            ctx.set_option("dual_force", 1)
            (xd, xi, s_ab), (yd, yi, s_ba) = N.knn_dual(ctx, qm, ym, K)
            np.testing.assert_array_equal(xi.numpy(), oi[:n_q], err_msg=f"shared sweep, h_q64 {q64}, {n_q} queries")
            np.testing.assert_array_equal(xd.numpy(), od[:n_q], err_msg=f"shared sweep, h_q64 {q64}, {n_q} queries")
            if n_q == 300:
                np.testing.assert_array_equal(yi.numpy(), oi_r, err_msg=f"shared sweep, reverse, h_q64 {q64}")
                np.testing.assert_array_equal(yd.numpy(), od_r, err_msg=f"shared sweep, reverse, h_q64 {q64}")
            got[q64] = [a.numpy() for a in (dist, ind, xd, xi, yd, yi)]
        for a, b in zip(got[0], got[1]):   # ... and the two kernels against each other, bit for bit
            assert a.tobytes() == b.tobytes()
