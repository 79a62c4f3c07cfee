"""Shared sweep with MODEL THRESHOLDS (kz_knn_dual.h): the event thresholds of b's rows come from a straight-line fit of a probe's
k-th key on |t_c|^2 instead of a sample sweep.  A threshold decides which pairs are filed as events, never an answer: forced onto
benign data, onto data the model is wrong for, with thresholds so low that the log overflows and so high that no pair is an event,
both directions stay IDENTICAL -- indices and float64 distances, bit for bit -- to two ordinary kz_knn searches.  In automatic
mode the gate takes the route on uniform rows of the smallest size that passes the size gates and refuses it on clustered rows.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SRC_NONE, SRC_SAMPLE, SRC_NESTED, SRC_MODEL = 0, 1, 2, 3   # kz_knn_stats.thresh_source


@pytest.fixture()
def ctx():
    from kiez_amd import _native as N
    c = N.Context.get()
    c.set_option("dual_force", 1)   # the test shapes are far below the size at which the shared sweep pays
    c.set_option("dual_model", 2)
    yield c
    for name, value in (("dual_force", 0), ("dual_model", 1), ("dual_model_shift", 0.0), ("floor_margin", 1.3), ("dual_stride", 1), ("chunk_rows", 0),
                        ("eps_scale", 1.0), ("precision", 0), ("dual_max_gb", 0), ("dual_overlap", 1), ("dual_rank", 0)):
        c.set_option(name, value)


def _uniform(n, d, seed):
    return np.random.default_rng(seed).random((n, d)).astype(np.float32)


def _clusters(n, d, seed, n_clusters=12):
    """Tight gaussian clusters stored cluster by cluster: |t_c|^2 says which cluster a row is in, not how near its neighbours are."""
    rng = np.random.default_rng(seed)
    centres = np.random.default_rng(99).standard_normal((n_clusters, d)) * 4   # (the same centres on both sides)
    sizes = np.full(n_clusters, n // n_clusters)
    sizes[: n - sizes.sum()] += 1
    spread = 0.02 * (1 + np.arange(n_clusters))   # (every cluster its own density: no line through the k-th keys)
    return np.concatenate([centres[c] + spread[c] * rng.standard_normal((sizes[c], d)) for c in range(n_clusters)]).astype(np.float32)


def _both_ways(ctx, a, b, k, metric="euclidean"):
    """(two kz_knn searches, the forced shared sweep, its statistics): the options the test has set apply to the shared sweep only."""
    from kiez_amd import _native as N
    am, bm = N.DeviceMatrix(ctx, a, metric), N.DeviceMatrix(ctx, b, metric)
    d_ab, i_ab, _ = N.knn(ctx, am, bm, k)
    d_ba, i_ba, _ = N.knn(ctx, bm, am, k)
    (xd, xi, s_ab), (yd, yi, s_ba) = N.knn_dual(ctx, am, bm, k)
    return (d_ab.numpy(), i_ab.numpy(), d_ba.numpy(), i_ba.numpy()), (xd.numpy(), xi.numpy(), yd.numpy(), yi.numpy()), s_ab, s_ba


def _assert_same(sep, dual):
    for name, x, y in zip(("dist a->b", "ind a->b", "dist b->a", "ind b->a"), sep, dual):
        np.testing.assert_array_equal(y, x, err_msg=name)


@pytest.mark.parametrize("na,nb,d,k", [
    (6000, 3000, 40, 10),    # K' = 16, reverse lists of 32
    (6000, 3000, 24, 50),    # lists longer than 16, reverse lists of 128; the probe keeps 110 < 6 k neighbours: saturated rows
    (2000, 5000, 40, 10),    # a smaller than b
    (5003, 3001, 40, 10),    # ragged last tile on both sides (5003 = 39 x 128 + 11, 3001 = 23 x 128 + 57)
])
def test_forced_model_thresholds_on_uniform_rows(ctx, na, nb, d, k):
    a, b = _uniform(na, d, 1), _uniform(nb, d, 2)
    assert na % 128 and nb % 128
    sep, dual, s_ab, s_ba = _both_ways(ctx, a, b, k)
    print(f"model thresholds {na} x {nb} x {d}, k {k}: events per row {s_ba['n_events'] / nb:.1f}, model mean / max {s_ab['model_mean_events']:.1f} / "
          f"{s_ab['model_max_events']}, overflowing rows {s_ba['n_overflow_rows']}, searched again {s_ba['n_escalated_rows']} + {s_ba['n_fallback_rows']}")
    _assert_same(sep, dual)
    assert s_ab["dual"] == 1 and s_ab["thresh_source"] == SRC_MODEL, s_ab
    assert s_ba["dual"] == 1 and s_ba["thresh_source"] == SRC_MODEL, s_ba
    assert s_ab["max_err_ratio"] < 1.0 and s_ba["max_err_ratio"] < 1.0
    assert s_ba["probe_ms"] > 0 and s_ba["n_events"] >= k * nb * 0.99   # (the margin keeps every probe row at k events or more)


def test_forced_model_on_data_it_is_wrong_for(ctx):
    """Cluster-ordered tight clusters of different density: rows whose threshold is too high come up short of events, rows whose
    threshold is too low overflow their buffer -- both come back through the list of uncertified rows and are searched again."""
    a, b = _clusters(4000, 32, 3), _clusters(3000, 32, 4)
    sep, dual, s_ab, s_ba = _both_ways(ctx, a, b, 10)
    print(f"hostile: events per row {s_ba['n_events'] / len(b):.1f}, overflowing rows {s_ba['n_overflow_rows']}, first-pass failures "
          f"{s_ba['n_first_pass_fail']}, searched again {s_ba['n_escalated_rows']} + {s_ba['n_fallback_rows']}, reverse from the sweep {s_ba['dual']}")
    _assert_same(sep, dual)
    assert s_ab["thresh_source"] == SRC_MODEL
    assert s_ba["n_escalated_rows"] + s_ba["n_fallback_rows"] > 0   # (fails if the hostile case silently stopped being hostile)


def test_thresholds_so_low_that_the_log_overflows(ctx):
    """A huge margin: nearly every pair is an event, the log of passed groups overflows, the reverse direction is answered the
    ordinary way."""
    ctx.set_option("floor_margin", 1e6)
    a, b = _uniform(6000, 40, 1), _uniform(3000, 40, 2)
    sep, dual, s_ab, s_ba = _both_ways(ctx, a, b, 10)
    _assert_same(sep, dual)
    assert s_ab["dual"] == 1 and s_ab["thresh_source"] == SRC_MODEL
    assert s_ba["dual"] == 0   # (the ordinary search's statistics: the log overflowed)


def test_thresholds_at_infinity_leave_no_events(ctx):
    """The opposite edge: no pair is an event, every row of b is uncertified and searched again."""
    ctx.set_option("dual_model_shift", 1e300)
    a, b = _uniform(6000, 40, 1), _uniform(3000, 40, 2)
    sep, dual, s_ab, s_ba = _both_ways(ctx, a, b, 10)
    _assert_same(sep, dual)
    assert s_ab["dual"] == 1 and s_ab["thresh_source"] == SRC_MODEL
    assert s_ba["n_events"] == 0
    assert s_ba["n_escalated_rows"] + s_ba["n_fallback_rows"] >= len(b)


# ---- the gate, automatic mode ------------------------------------------------------------------------------------------------
# The smallest uniform shape that passes the size gates: the probes need 2 n^2 d / 1e12 >= 12 model-ms, and the nested sample --
# whose place the model takes -- sweep / stride >= 2 model-ms with stride = sqrt(sweep / (n rank 1e-7)) at rank 8: n >= 232 000 at
# d = 200, k = 10 (kz_knn_dual).  240 000: 23 model-ms.
GATE_N, GATE_D, GATE_K = 240_000, 200, 10


def _gmm_rows(seed, rows, d):
    """bench.synth_rows("gmm", seed, rows, d), row for row (bench.py imports torch, which must not be loaded behind the library: the
    recipe is repeated here): 256 cluster centres common to both sides, spread 0.35, every row L2-normalised, rows in random order."""
    rng = np.random.RandomState(seed)
    out = np.empty((rows, d), dtype=np.float32)
    centres = np.random.RandomState(6).standard_normal((256, d)).astype(np.float32)
    for b in range(0, rows, 100_000):
        m = min(100_000, rows - b)
        x = centres[rng.randint(0, 256, m)] + np.float32(0.35) * rng.standard_normal((m, d)).astype(np.float32)
        out[b:b + m] = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    return out


def _gate_call(kind):
    from kiez_amd import _native as N
    from oracle import kiez_oracle as O
    ctx = N.Context.get()
    for name, value in (("dual_force", 0), ("dual_model", 1), ("dual_model_shift", 0.0), ("floor_margin", 1.3)):
        ctx.set_option(name, value)
    if kind == "uniform":
        a, b = _uniform(GATE_N, GATE_D, 5), _uniform(GATE_N, GATE_D, 6)
    else:
        a, b = _gmm_rows(5, GATE_N, GATE_D), _gmm_rows(6, GATE_N, GATE_D)
    am, bm = N.DeviceMatrix(ctx, a, "euclidean"), N.DeviceMatrix(ctx, b, "euclidean")
    (xd, xi, s_ab), (yd, yi, s_ba) = N.knn_dual(ctx, am, bm, GATE_K)
    print(f"gate, {kind}: thresh_source {s_ab['thresh_source']}, forward fit r2 {s_ab['floor_r2']:.4f}, model mean / max events {s_ab['model_mean_events']:.1f} / "
          f"{s_ab['model_max_events']}, events per row {s_ba['n_events'] / GATE_N:.1f}, reverse probe {s_ba['probe_ms']:.2f} ms, searched again "
          f"{s_ba['n_escalated_rows']} + {s_ba['n_fallback_rows']}")
    rows = np.arange(256) * (GATE_N // 256)
    # (float32 rows, euclidean: the oracle's float64 distances are float32-representable, 2^-24 relative: 1e-6 is ~16 of those steps)
    for got_d, got_i, q, idx in ((xd, xi, a, b), (yd, yi, b, a)):
        od, oi = O.knn_exact(q[rows], idx, GATE_K, "euclidean")
        np.testing.assert_array_equal(got_i.numpy()[rows], oi)
        np.testing.assert_allclose(got_d.numpy()[rows], od, rtol=1e-6, atol=0)
    return s_ab, s_ba


def test_gate_takes_the_model_on_uniform_rows():
    s_ab, s_ba = _gate_call("uniform")
    assert s_ab["dual"] == 1 and s_ba["dual"] == 1
    assert s_ab["thresh_source"] == SRC_MODEL and s_ba["thresh_source"] == SRC_MODEL, s_ab


def test_gate_refuses_the_model_on_clustered_rows():
    s_ab, s_ba = _gate_call("gmm")
    assert s_ab["dual"] == 1
    assert s_ab["thresh_source"] == SRC_NESTED, s_ab
    assert s_ba["probe_ms"] == 0   # (the pre-gate refused before the reverse probe ran)
