"""tests/image_restate.py against itself and against torch: the restated layouts are bijections, the restated bf16 rounding is
torch's, and the split bound the bf16 tier relies on holds for the restated split.  No GPU."""
import math

import numpy as np
import pytest

from tests import image_restate as R


SHAPES = [(1, 1), (127, 17), (129, 20), (300, 33), (257, 260)]


def _check_bijection(off, live, size):
    """off [n_pad, k_pad]: a bijection onto [0, size); live [n_pad, k_pad]: the (row < n, k < d) positions -- everything else is padding."""
    flat = off.ravel()
    assert flat.min() == 0 and flat.max() == size - 1 and len(flat) == size
    assert len(np.unique(flat)) == size
    is_live = np.zeros(size, dtype=bool)
    is_live[off[live]] = True
    assert is_live.sum() == live.sum()
    return is_live


@pytest.mark.parametrize("n,d", SHAPES)
def test_f32_layout_is_a_bijection(n, d):
    npad, dpad = R.n_pad(n), R.kg(d) * 4
    row, k = R.grid(npad, dpad)
    off = R.f32_offset(row, k, d)
    live = (row < n) & (k < d)
    assert _check_bijection(off, live, npad * dpad).sum() == n * d
    # a row's four k of one k-group are contiguous, the 128 rows of a tile 4 elements apart, k-groups 512 apart
    assert off[0, 1] - off[0, 0] == 1 and off[1, 0] - off[0, 0] == 4
    if dpad > 4:
        assert off[0, 4] - off[0, 0] == 512


@pytest.mark.parametrize("n,d", SHAPES)
def test_bf16_layout_is_a_bijection(n, d):
    npad, dpad = R.n_pad(n), R.kg(d) * 4
    row, k = R.grid(npad, dpad)
    off = np.concatenate([R.bf_offset(row, k, d, 0), R.bf_offset(row, k, d, 1)], axis=1)
    live = np.concatenate([(row < n) & (k < d)] * 2, axis=1)
    assert _check_bijection(off, live, 2 * npad * dpad).sum() == 2 * n * d
    # planes hi(k 0-7), hi(k 8-15), lo(k 0-7), lo(k 8-15), 1024 elements each
    assert R.bf_offset(0, 8, d, 0) == 1024 and R.bf_offset(0, 0, d, 1) == 2048 and R.bf_offset(0, 8, d, 1) == 3072
    assert R.bf_offset(1, 0, d, 0) == 8


@pytest.mark.parametrize("n,d", SHAPES[1:] + [(130, 513), (129, 1040)])
def test_fp16_layout_is_a_bijection(n, d):
    assert R.h_slices_ok(R.kg(d))
    nsr = R.h_nsr(R.kg(d))
    npad = R.n_pad(n)
    row, k = R.grid(npad, 16 * nsr)
    off = R.h_offset(row, k, nsr)
    live = (row < n) & (k < d)
    assert _check_bijection(off, live, npad * nsr * 16).sum() == n * d
    assert R.h_offset(0, 8, nsr) == 1024 and R.h_offset(0, 16, nsr) == 2048 and R.h_offset(1, 0, nsr) == 8
    assert R.h_offset(128, 0, nsr) == nsr * 2048


def test_fp16_slice_counts():
    got = [R.h_nsr(R.kg(d)) for d in (17, 384, 497, 513, 1024, 1025, 2048)]
    assert got == [2, 24, 32, 40, 64, 80, 128]
    assert not R.h_slices_ok(R.kg(16)) and not R.h_slices_ok(R.kg(385)) and not R.h_slices_ok(R.kg(496))
    assert R.h_slices_ok(R.kg(497)) and R.h_slices_ok(R.kg(2048)) and not R.h_slices_ok(R.kg(2049))


@pytest.mark.parametrize("n,p", [(1000, 2), (1000, 3), (1000, 7), (1000, 1000), (10, 4), (7, 7), (129, 5)])
def test_dealt_rows_are_a_permutation_part_by_part(n, p):
    perm = R.dealt_perm(n, p)
    assert sorted(perm[:n].tolist()) == list(range(n)) and (perm[n:] == -1).all() and len(perm) == R.n_pad(n)
    want = [j for part in range(p) for j in range(part, n, p)]
    assert perm[:n].tolist() == want


def _torch_bf16_bits(x32):
    import torch
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bf16_rounding_is_torch_bfloat16():
    rng = np.random.RandomState(11)
    u = rng.randint(0, 2 ** 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    x = u.view(np.float32)
    x = x[np.isfinite(x)]
    np.testing.assert_array_equal(R.bf16_rn(x), _torch_bf16_bits(x))
    # every tie: low half 0x8000 under every finite upper half (even and odd kept bits, both signs, subnormals)
    upper = np.arange(2 ** 16, dtype=np.uint32)
    upper = upper[((upper >> 7) & 0xFF) != 0xFF]
    ties = ((upper << 16) | 0x8000).view(np.float32)
    got = R.bf16_rn(ties)
    np.testing.assert_array_equal(got, _torch_bf16_bits(ties))
    assert ((got & 1) == 0).all()           # ties go to the even neighbour


def _split_inputs(dtype):
    rng = np.random.RandomState(5)
    e = rng.randint(-100, 49, size=400_000)
    sign = np.where(rng.rand(len(e)) < 0.5, -1.0, 1.0)
    out = [sign * np.ldexp(1.0 + rng.rand(len(e)), e)]
    bits = 24 if dtype == np.float32 else 53
    exps = np.arange(-100, 49)
    ones = 2.0 - 2.0 ** (1 - bits)                         # all-ones significand
    out.append(np.ldexp(ones, exps))
    out.append(-np.ldexp(ones, exps))
    for b in range(bits):                                   # 1 + one significand bit
        out.append(np.ldexp(1.0 + 2.0 ** -b if b else 1.0, exps))
    out.append(np.array([2.0 ** -100, 2.0 ** 49, -2.0 ** 49]))
    x = np.concatenate(out).astype(dtype).astype(np.float64)
    return x[(np.abs(x) >= 2.0 ** -100) & (np.abs(x) <= 2.0 ** 49)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_split_bound_of_the_bf16_tier(dtype):
    x = _split_inputs(dtype)
    hi, lo = R.bf_split(x)
    err = np.abs((x - R.bf16_to_f64(hi)) - R.bf16_to_f64(lo))      # both differences are exact in float64
    assert (err <= R.SPLIT_BOUND * np.abs(x)).all(), float((err / np.abs(x)).max())
    assert (err > 0).any()


def test_scale_is_a_power_of_two_with_a_clamped_exponent():
    for amax, want in ((1.0, 2.0 ** 12), (0.999, 2.0 ** 13), (0.5, 2.0 ** 13), (4.0, 2.0 ** 10), (2.0 ** -120, 2.0 ** 100),
                       (2.0 ** 130, 2.0 ** -100), (0.0, 1.0), (3e5, 2.0 ** -6)):
        assert R.scale_of(amax) == want, amax
        if amax > 0 and 2.0 ** -80 < amax < 2.0 ** 80:
            assert 2.0 ** 12 <= amax * R.scale_of(amax) <= 2.0 ** 13


def test_fp16_pipeline_flushes_clamps_and_rounds():
    mu = np.zeros(8, dtype=np.float32)
    op = np.array([[2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -20), -2.0 ** -15, 65504.0, 1e6, -1e6, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]])
    v, h = R.h_pipeline(op, mu, 1.0)
    assert h.tolist() == [[2.0 ** -14, 0.0, 0.0, 65504.0, 65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -9]]
    assert not np.signbit(h[0, 2])
    c2, nh, nr = R.h_row_stats(v, h, 1.0)
    assert nr[0] >= 1e6 - 65504.0            # the clamped part is in the residual
    # exact_squares: the sum of squares of 53-bit values, correctly rounded
    from fractions import Fraction
    a = np.ldexp(np.random.RandomState(3).rand(50, 9), np.random.RandomState(4).randint(-40, 40, size=(50, 9)))
    a[0, :3] = [1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 2.0 ** -30]
    want = [float(sum(Fraction(t) ** 2 for t in row)) for row in a]
    assert R.fsum_rows(R.exact_squares(a)).tolist() == want
    assert [math.fsum(row * row) for row in a] != want        # (the rounded squares alone are not enough)
