"""Shared by tests/test_half_inputs.py and tests/test_gpu_half_inputs.py: the 2-byte element types in numpy.  float16 is numpy's own;
bfloat16 has no numpy dtype and travels as its uint16 bit patterns (the upper half of a float32, rounded to nearest even -- the
arithmetic of kz_bf16_rn in kiez_amd/csrc/kz_pack.hip, restated here on its own).  No GPU, no torch."""
import numpy as np

HALF_ELEMS = ("float16", "bfloat16")


def bf16_bits(x32):
    """uint16 bit patterns of float32 values rounded to bfloat16, ties to even (finite inputs)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    """float64 values of bfloat16 bit patterns (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def round_to(x32, elem):
    """float32 values rounded to `elem` -> (what goes to the device: float16 array / uint16 bits, the same values in float64)."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if elem == "float16":
        with np.errstate(over="ignore"):
            h = x32.astype(np.float16)
        return h, h.astype(np.float64)
    assert elem == "bfloat16", elem
    b = bf16_bits(x32)
    return b, bf16_widen(b)


def draw(n, d, elem, seed, kind="normal"):
    """n x d values drawn in float32 and rounded to `elem`: every value is representable.  kinds: 'normal' (standard normal),
    'grid' (a coarse grid: exact ties are common), 'tight' (clusters three orders of magnitude tighter than their distance from the
    centre, rows shuffled -- the data of bench.py's `cliff` workload: rows no approximate tier certifies)."""
    rng = np.random.default_rng(seed)
    if kind == "grid":
        x = rng.integers(-4, 5, size=(n, d)).astype(np.float32) * np.float32(0.25)
    elif kind == "tight":
        centres = np.random.default_rng(5).standard_normal((6, d)) * 3
        sc = 0.01 * 2.0 ** np.random.default_rng(6).integers(0, 4, 6)
        c = rng.integers(0, 6, n)
        x = (centres[c] + sc[c, None] * rng.standard_normal((n, d))).astype(np.float32)
    else:
        x = rng.standard_normal((n, d)).astype(np.float32)
    return round_to(x, elem)


def has_duplicate_rows(x64):
    return len(np.unique(np.ascontiguousarray(x64), axis=0)) != len(x64)
