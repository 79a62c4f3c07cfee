"""float16 / bfloat16 rows, the parts that need no GPU: the ABI's two new element codes (additive: the version stays 7), the
binding's constants, the numpy restatement of bfloat16 the GPU tests draw their data with (against torch on CPU tensors, every tie
included, as tests/test_image_restate.py does for the operand image), and the metric gate of SklearnNN: which element type a
float16 array is stored as, decided without a device."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import half_inputs as H

ROOT = Path(__file__).resolve().parent.parent


def test_header_defines_the_half_element_types_and_keeps_the_abi_version():
    text = (ROOT / "include" / "kiez_amd.h").read_text()
    enums = dict(re.findall(r"\b(KZ_B?F(?:16|32|64))\s*=\s*(\d+)", text))
    assert enums == {"KZ_F32": "0", "KZ_F64": "1", "KZ_F16": "2", "KZ_BF16": "3"}, enums
    assert re.search(r"^#define KZ_ABI_VERSION 7$", text, re.M)   # purely additive


def test_native_exports_the_constants():
    from kiez_amd import _native as N
    assert (N.KZ_F32, N.KZ_F64, N.KZ_F16, N.KZ_BF16) == (0, 1, 2, 3)
    assert N.ELEM_CODES == {"float32": 0, "float64": 1, "float16": 2, "bfloat16": 3}
    assert N.ABI_VERSION == 7


def _torch_bf16_bits(x32):
    import torch
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bf16_helper_is_torch_bfloat16_ties_included():
    import torch
    rng = np.random.RandomState(3)
    x = rng.randint(0, 2 ** 32, size=200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[np.isfinite(x)]
    np.testing.assert_array_equal(H.bf16_bits(x), _torch_bf16_bits(x))
    upper = np.arange(2 ** 16, dtype=np.uint32)
    upper = upper[((upper >> 7) & 0xFF) != 0xFF]
    ties = ((upper << 16) | 0x8000).view(np.float32)       # low half exactly one half: every finite upper half, both signs, subnormals
    got = H.bf16_bits(ties)
    np.testing.assert_array_equal(got, _torch_bf16_bits(ties))
    assert ((got & 1) == 0).all()
    # the widening is exact, and the same as torch's
    bits = np.arange(2 ** 16, dtype=np.uint16)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    t = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(torch.float64).numpy()
    np.testing.assert_array_equal(H.bf16_widen(bits), t)
    b, w = H.round_to(x[:1000], "bfloat16")
    np.testing.assert_array_equal(H.bf16_bits(w.astype(np.float32)), b)    # representable: rounding again changes nothing


@pytest.mark.parametrize("metric,p,elem,want", [
    ("euclidean", 2, "float16", "float16"), ("sqeuclidean", 2, "float16", "float16"), ("cosine", 2, "bfloat16", "bfloat16"),
    ("minkowski", 2, "float16", "float16"), ("euclidean", 2, "bfloat16", "bfloat16"),
    ("manhattan", 2, "float16", "float64"), ("minkowski", 3, "float16", "float64"), ("chebyshev", 2, "bfloat16", "float64"),
    ("correlation", 2, "float16", "float64"), ("jaccard", 2, "float16", "float32"), ("yule", 2, "bfloat16", "float32"),
    ("euclidean", 2, "float32", "float32"), ("manhattan", 2, "float64", "float64"), ("euclidean", 2, "int32", "float64"),
    ("jaccard", 2, "bool", "float32"),
])
def test_metric_gate_routes_half_rows_without_a_device(metric, p, elem, want):
    from kiez_amd.neighbors import SklearnNN
    nn = SklearnNN(metric=metric, p=p, metric_params={"V": [1.0]} if metric == "seuclidean" else None)
    assert nn._storage(elem) == want
    assert nn._ctx is None      # no device was asked for


def test_prepare_keeps_float16_for_euclidean_and_widens_for_manhattan():
    from kiez_amd.neighbors import SklearnNN
    x = np.arange(12, dtype=np.float16).reshape(3, 4)
    assert SklearnNN(metric="euclidean")._prepare(x).dtype == np.float16
    got = SklearnNN(metric="manhattan")._prepare(x)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, x.astype(np.float64))
    assert SklearnNN(metric="euclidean")._prepare(x, "float64").dtype == np.float64      # (an index of another type: widened, never narrowed)
