"""Restatement of what kiez_amd/csrc/kz_pack.hip builds per matrix, in numpy float64 and plain Python (test infrastructure of
tests/test_image_restate.py and tests/test_gpu_images.py): the three operand layouts (struct comments of kz_common.h, DESIGN.md
section 2), kz_dealt_row, the bf16 split and the element pipeline of the fp16 image.  Nothing here reads the library.

Offsets are in ELEMENTS of the buffer's own type (float32, uint16, fp16); `row` and `k` broadcast.
"""
import math

import numpy as np

TILE = 128
KSLICE = 16
FP16_MIN_NORMAL = 2.0 ** -14
FP16_MAX = 65504.0
SPLIT_BOUND = 2.0 ** -16 * (1.0 + 2.0 ** -7)   # |x - hi - lo| <= SPLIT_BOUND |x| (kz_knn_bf16.h)


def n_pad(n):
    return (n + TILE - 1) // TILE * TILE


def kg(d):
    """4-wide k-groups of a row padded to a multiple of 16 features."""
    return (d + KSLICE - 1) // KSLICE * KSLICE // 4


def h_nsr(kg_):
    """Slices of the fp16 image (kz_h_nsr): d_pad / 16, a multiple of 8 beyond 32 and of 16 beyond 64."""
    s = kg_ // 4
    if s <= 32:
        return s
    return (s + 7) // 8 * 8 if s <= 64 else (s + 15) // 16 * 16


def h_slices_ok(kg_):
    s = kg_ // 4
    return 2 <= s <= 24 or 32 <= s <= 128


def f32_offset(row, k, d):
    """float32 image [tile][k / 4][128][4]."""
    row, k = np.asarray(row, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return (((row >> 7) * kg(d) + (k >> 2)) * TILE + (row & 127)) * 4 + (k & 3)


def bf_offset(row, k, d, lo):
    """split-bf16 image [tile][k / 16][hi0, hi1, lo0, lo1][128][8]; lo: 0 = the hi plane, 1 = the lo plane."""
    row, k = np.asarray(row, dtype=np.int64), np.asarray(k, dtype=np.int64)
    plane = ((k >> 3) & 1) + 2 * int(lo)
    return ((((row >> 7) * (kg(d) // 4) + (k >> 4)) * 4 + plane) * TILE + (row & 127)) * 8 + (k & 7)


def h_offset(row, k, nsr):
    """fp16 image [tile][slice][2][128][8]."""
    row, k = np.asarray(row, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return ((((row >> 7) * nsr + (k >> 4)) * 2 + ((k >> 3) & 1)) * TILE + (row & 127)) * 8 + (k & 7)


def grid(n_rows, n_k):
    return np.arange(n_rows, dtype=np.int64)[:, None], np.arange(n_k, dtype=np.int64)[None, :]


def dealt_row(rp, n, p):
    """kz_dealt_row: the matrix row at position rp of n rows dealt over p parts (part j = rows j, j + p, ...; the first n % p parts
    hold one row more)."""
    q, r = divmod(n, p)
    if rp < r * (q + 1):
        part, i = divmod(rp, q + 1)
    else:
        j2 = rp - r * (q + 1)
        part, i = r + j2 // q, j2 % q
    return part + p * i


def dealt_perm(n, p):
    """The permutation buffer of a dealt image: dealt_row on [0, n), -1 on [n, n_pad)."""
    out = np.full(n_pad(n), -1, dtype=np.int32)
    out[:n] = [dealt_row(rp, n, p) for rp in range(n)]
    return out


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------
def bf16_rn(x32):
    """float32 -> bf16 bits, round to nearest even on the bit pattern (finite inputs)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf_split(op64):
    """(hi bits, lo bits) of float64 operands: hi = bf16(float32(op)), lo = bf16(float32(op - hi))."""
    op64 = np.asarray(op64, dtype=np.float64)
    hi = bf16_rn(op64.astype(np.float32))
    lo = bf16_rn((op64 - bf16_to_f64(hi)).astype(np.float32))
    return hi, lo


# ---- operands and the fp16 pipeline --------------------------------------------------------------------------------------------
def operands(x, metric, sqn):
    """float64 operands of a matrix: x, or for cosine x / sqn[row] (sqn: the norms kz_norms_kernel stored, 1.0 for a zero row)."""
    x64 = np.asarray(x, dtype=np.float64)
    return x64 / np.asarray(sqn, dtype=np.float64)[:, None] if metric == "cosine" else x64


def scale_of(amax):
    """S = 2^(13 - e) with amax = f 2^e, f in [0.5, 1); the exponent clamped to +-100; 1.0 for amax = 0."""
    if not 0.0 < amax < 1e300:
        return 1.0
    _, e = math.frexp(amax)
    return math.ldexp(1.0, max(-100, min(100, 13 - e)))


def h_pipeline(op64, mu32, S):
    """(v float32 = the centred operand, fp16 values) of kz_pack_h_kernel: float32(op - mu), times S, flushed below 2^-14, clamped to
    +-65504, rounded to fp16."""
    v = (np.asarray(op64, dtype=np.float64) - np.asarray(mu32, dtype=np.float32).astype(np.float64)[None, :]).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        vs = v * np.float32(S)
    vs = np.where(np.abs(vs) < np.float32(FP16_MIN_NORMAL), np.float32(0.0), vs)
    vs = np.minimum(np.maximum(vs, np.float32(-FP16_MAX)), np.float32(FP16_MAX))
    return v, vs.astype(np.float16)


def fsum_rows(a):
    return np.array([math.fsum(r) for r in np.asarray(a, dtype=np.float64)], dtype=np.float64)


def exact_squares(a):
    """[rows, 2 k]: per element p = RN(a a) and the exact remainder a a - p (Dekker's product on Veltkamp halves), so that the
    math.fsum of a row is the correctly rounded sum of the exact squares whatever the width of a's significand."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        c = a * 134217729.0          # 2^27 + 1
        ah = c - (c - a)
        al = a - ah
        p = a * a
        e = ((ah * ah - p) + 2.0 * ah * al) + al * al
    e = np.where(np.isfinite(e), e, 0.0)
    return np.concatenate([p, e], axis=1)


def h_row_stats(v32, h16, S):
    """(|x_c|^2, |x_h|, |x_c - x_h|) per row from the centred operands and the fp16 values, sums by math.fsum.  (v is a float32 and
    x_h an 11-bit value: their squares are exact in float64; the residual's need not be.)"""
    v = v32.astype(np.float64)
    xh = h16.astype(np.float64) / S
    res = v - xh
    return fsum_rows(v * v), np.sqrt(fsum_rows(xh * xh)), np.sqrt(fsum_rows(exact_squares(res)))
