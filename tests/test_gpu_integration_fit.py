"""The two-call binding INTEGRATION.md shows (section 2: `MI355XFit` over `ctypes`, kz_fit / kz_kneighbors / kz_fitted_destroy) is
EXECUTED here as it stands in the document -- only the path of the shared library is substituted, as tests/test_gpu_integration_stub.py
does for the search stub -- and compared with the facade for CSLS, two-sided and single-source: the same bytes."""
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _block_source():
    text = (ROOT / "INTEGRATION.md").read_text()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "class MI355XFit" in b]
    assert len(blocks) == 1 and "class MI355XNN" not in blocks[0], "the two-call binding is a block of its own"
    block = blocks[0]
    for call in ("kz_fit(", "kz_kneighbors(", "kz_fitted_destroy("):
        assert "_lib." + call in block, call
    assert "kz_knn(" not in block and "kz_csls" not in block and "kz_select_topk" not in block, "the block binds the two calls, not the primitives"
    block = block.replace('C.CDLL("libkiez_amd.so")', f'C.CDLL({str(ROOT / "kiez_amd" / "libkiez_amd.so")!r})')
    assert "kiez_amd/libkiez_amd.so" in block
    return block


def test_the_documented_two_call_binding_equals_the_facade():
    from kiez_amd import Kiez
    ns = {}
    exec(compile(_block_source(), "INTEGRATION.md#MI355XFit", "exec"), ns)
    MI355XFit = ns["MI355XFit"]
    rng = np.random.RandomState(11)
    for metric, dtype in (("euclidean", np.float64), ("cosine", np.float32)):
        s, t = rng.rand(260, 20).astype(dtype), rng.rand(330, 20).astype(dtype)
        out = np.float32 if metric == "cosine" else np.float64
        for target in (t, None):
            facade = Kiez(n_candidates=8, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness="CSLS").fit(s, target)
            bound = MI355XFit(n_candidates=8, metric=metric, hubness="csls").fit(s, target)
            try:
                for k in (8, 3):
                    want_d, want_i = facade.kneighbors(k)
                    got_d, got_i = bound.kneighbors(k, out)
                    what = f"{metric} {'two-sided' if target is not None else 'single-source'} k={k}"
                    assert got_i.dtype == want_i.dtype and got_i.tobytes() == want_i.tobytes(), what + ": ids"
                    assert got_d.dtype == want_d.dtype and got_d.tobytes() == want_d.tobytes(), what + ": distances"
            finally:
                bound.close()
    # no reduction through the same two calls
    s, t = rng.rand(100, 12), rng.rand(90, 12)
    plain = Kiez(n_candidates=5, algorithm="SklearnNN", algorithm_kwargs={"metric": "sqeuclidean"}).fit(s, t)
    bound = MI355XFit(n_candidates=5, metric="sqeuclidean", hubness=None).fit(s, t)
    try:
        want_d, want_i = plain.kneighbors(5)
        got_d, got_i = bound.kneighbors(5)
        assert got_i.tobytes() == want_i.tobytes() and got_d.tobytes() == want_d.tobytes()
    finally:
        bound.close()
