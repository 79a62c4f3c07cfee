"""kz_fit / kz_kneighbors -- one native call per fit and per kneighbors -- through `_native.fit` / `Fitted.kneighbors` and through
the facade's opt-in `hubness_kwargs={"native_fit": True}`, against the facade WITHOUT the flag on the same context (the present
pipeline of primitives, pinned to the reference by the goldens).  Equality is on bytes for distances and ids: the native calls
run the same searches and the same arithmetic.

300 x 200 and 200 x 300 rows so that kz_knn_dual's "larger matrix first" swap runs both ways; K = 10, k in 1 / 5 / 10 and then a
second kneighbors with another k on the same object (no second search); every kind; float64 euclidean, float32 sqeuclidean and
float32 cosine (float32 output, the cast last); the shared sweep forced on and off, and `shared_sweep = 0`, where the forward search
happens at the first kneighbors; single source through the split (n = 257) and through two self searches (K = 110); K = 130, beyond
the fused kernel."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 24
SHAPES = ((300, 200), (200, 300))
METRICS = (("euclidean", np.float64), ("sqeuclidean", np.float32), ("cosine", np.float32))
# (facade name, its constructor arguments, the native kind's name)
REDUCTIONS = (("CSLS", {}, "HUB_CSLS"), ("LocalScaling", {"method": "standard"}, "HUB_LS"), ("LocalScaling", {"method": "nicdm"}, "HUB_NICDM"),
              ("MutualProximity", {"method": "normal"}, "HUB_MP_NORMAL"), ("MutualProximity", {"method": "empiric"}, "HUB_MP_EMPIRIC"))


@pytest.fixture(scope="module")
def ctx():
    from kiez_amd import _native as N
    return N.Context.get()


def _data(ns, nt, dtype, seed=0):
    rng = np.random.RandomState(seed)
    return rng.rand(ns, D).astype(dtype), (rng.rand(nt, D).astype(dtype) if nt else None)


def _kiez(metric, hubness, kwargs, K=10, native=False, shared=True):
    from kiez_amd import Kiez
    kw = dict(kwargs)
    if native:
        kw["native_fit"] = True
    k = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=hubness, hubness_kwargs=kw)
    k.hubness._shared_sweep = shared
    return k


def _same(got, want, what):
    for g, w, name in zip(got, want, ("distances", "ids")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differ in {np.count_nonzero(g != w)} entries"


def _fitted_arrays(h):
    """The fitted attributes a reduction exposes, as numpy arrays by name."""
    names = ("r_dist_train_", "r_ind_train_", "_r_train_dev", "r_dist_t_to_s_", "r_ind_t_to_s_", "_r_t_dev", "neigh_dist_t_to_s_",
             "neigh_ind_t_to_s_", "_dist_t2s_dev", "_ind_t2s_dev", "mu_t_to_s_", "sd_t_to_s_", "_mu_dev", "_sd_dev")
    out = {n: getattr(h, n).numpy() for n in names if hasattr(h, n)}
    if hasattr(h, "n_train"):
        out["n_train"] = np.asarray(h.n_train)
    return out


@pytest.mark.parametrize("metric,dtype", METRICS, ids=[m for m, _ in METRICS])
@pytest.mark.parametrize("shape", SHAPES, ids=["300x200", "200x300"])
def test_facade_opt_in_equals_the_default_pipeline_on_bytes(ctx, shape, metric, dtype):
    from kiez_amd import _native as N
    s, t = _data(*shape, dtype)
    out_dtype = np.float32 if (metric == "cosine" and dtype == np.float32) else np.float64
    for name, kwargs, kind_name in REDUCTIONS:
        for force in (1, 0):
            ctx.set_option("dual_force", force)
            try:
                ref = _kiez(metric, name, kwargs).fit(s, t)
                nat = _kiez(metric, name, kwargs, native=True).fit(s, t)
                what = f"{name}{kwargs} {metric} {shape} dual_force={force}"
                assert nat.hubness._native_fit is True and nat.hubness._fitted is not None and ref.hubness._fitted is None
                info = nat.hubness._fitted.info
                assert info["search"] == N.FIT_SEARCH_DUAL and info["hubness"] == getattr(N, kind_name) and info["forward_ready"] == 1
                assert info["larger_first"] == (1 if shape[0] >= shape[1] else 0)
                assert info["tail"] == (N.FIT_TAIL_EMPIRIC if kind_name == "HUB_MP_EMPIRIC" else N.FIT_TAIL_FUSED)
                # which route ran inside kz_knn_dual -- the shared sweep or two searches -- is the library's verdict (at these sizes:
                # two searches, forced or not; test_the_shared_sweep_itself has the sizes at which the sweep runs): the fitted object
                # reports what the default path's statistics report
                want_dual = ref.algorithm.last_stats["dual"]
                assert ref.algorithm.last_stats_reverse["dual"] == want_dual
                assert info["stats_forward"]["dual"] == want_dual and info["stats_reverse"]["dual"] == want_dual, what
                assert nat.algorithm.last_stats["dual"] == want_dual and nat.algorithm.last_stats_reverse["dual"] == want_dual
                a, b = _fitted_arrays(ref.hubness), _fitted_arrays(nat.hubness)
                assert set(a) == set(b) and a, (what, set(a) ^ set(b))
                for key in a:
                    assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), f"{what}: fitted attribute {key}"
                for k in (1, 5, 10, 3):   # (3: a second k after the lists are kept -- no search)
                    got = nat.kneighbors(k)
                    assert got[0].dtype == out_dtype
                    _same(got, ref.kneighbors(k), f"{what} k={k}")
                assert nat.hubness._fitted.info["n_searches"] == 1
            finally:
                ctx.set_option("dual_force", 0)


@pytest.mark.parametrize("shape", ((1500, 2000), (2000, 1500)), ids=["1500x2000", "2000x1500"])
def test_the_shared_sweep_itself(ctx, shape):
    """The sizes of smoke(): with `dual_force` 1 kz_knn_dual runs the shared sweep (below ~1000 index rows it never does), without it
    two searches; `Fitted.info` says which, and the results are the default path's either way, for every kind."""
    from kiez_amd import _native as N
    rng = np.random.RandomState(8)
    s, t = rng.rand(shape[0], 50).astype(np.float32), rng.rand(shape[1], 50).astype(np.float32)
    for force in (1, 0):
        ctx.set_option("dual_force", force)
        try:
            for name, kwargs, _kind in REDUCTIONS:
                ref = _kiez("euclidean", name, kwargs).fit(s, t)
                nat = _kiez("euclidean", name, kwargs, native=True).fit(s, t)
                info = nat.hubness._fitted.info
                assert ref.algorithm.last_stats["dual"] == force, "the default path's route is not what dual_force asks for"
                assert info["search"] == N.FIT_SEARCH_DUAL and info["larger_first"] == (1 if shape[0] >= shape[1] else 0)
                assert info["stats_forward"]["dual"] == force and info["stats_reverse"]["dual"] == force
                assert nat.algorithm.last_stats["dual"] == force and nat.algorithm.last_stats_reverse["dual"] == force
                for k in (10, 4):
                    _same(nat.kneighbors(k), ref.kneighbors(k), f"{name}{kwargs} {shape} dual_force={force} k={k}")
                assert nat.hubness._fitted.info["n_searches"] == 1
        finally:
            ctx.set_option("dual_force", 0)


@pytest.mark.parametrize("kind_name", ["HUB_NONE"] + [r[2] for r in REDUCTIONS])
def test_abi_objects_without_shared_sweep_and_none(ctx, kind_name):
    """`_native.fit` itself: KZ_HUB_NONE (ABI only: one kz_knn per kneighbors), and shared_sweep = 0, where fit runs the reverse search
    alone and the first kneighbors the forward one; .state() views against the facade's attributes."""
    from kiez_amd import _native as N
    kind = getattr(N, kind_name)
    s, t = _data(300, 200, np.float64, seed=1)
    sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
    f = N.fit(ctx, sm, tm, kind, 10, shared_sweep=False)
    info = f.info
    assert (info["n_source"], info["n_target"], info["n_candidates"], info["single_source"], info["shared_sweep"]) == (300, 200, 10, 0, 0)
    if kind == N.HUB_NONE:
        ref = _kiez("euclidean", None, {})
        ref.fit(s, t)
        assert info["search"] == N.FIT_SEARCH_NONE and info["tail"] == N.FIT_TAIL_KNN and info["n_searches"] == 0
        assert f.state("reverse_dist") is None and f.state("forward_dist") is None and f.state("state_a") is None
        for k in (1, 5, 10):
            od, oi = f.kneighbors(k)
            _same((od.numpy(), oi.numpy()), ref.kneighbors(k), f"none k={k}")
            od32, _ = f.kneighbors(k, np.float32)
            assert od32.dtype == np.float32 and od32.numpy().tobytes() == od.numpy().astype(np.float32).tobytes()
        assert f.info["n_searches"] == 6
    else:
        name, kwargs = next((r[0], r[1]) for r in REDUCTIONS if r[2] == kind_name)
        ref = _kiez("euclidean", name, kwargs, shared=False)
        ref.fit(s, t)
        assert info["search"] == N.FIT_SEARCH_REVERSE and info["forward_ready"] == 0 and info["n_searches"] == 1
        assert f.state("forward_dist") is None and f.state("forward_ind") is None
        rd, ri = f.state("reverse_dist"), f.state("reverse_ind")
        assert rd.shape == ri.shape == (200, 10)
        rev = ref.algorithm.kneighbors_device(k=10, query=t, s_to_t=False)
        assert rd.numpy().tobytes() == rev[0].numpy().tobytes() and ri.numpy().tobytes() == rev[1].numpy().tobytes()
        n_state = {"HUB_MP_NORMAL": 2, "HUB_MP_EMPIRIC": 0}.get(kind_name, 1)
        assert (f.state("state_a") is not None) == (n_state >= 1) and (f.state("state_b") is not None) == (n_state == 2)
        for k in (5, 10, 1):
            od, oi = f.kneighbors(k)
            _same((od.numpy(), oi.numpy()), ref.kneighbors(k), f"{kind_name} shared_sweep=0 k={k}")
        after = f.info
        assert after["forward_ready"] == 1 and after["n_searches"] == 2, "the forward search runs once, at the first kneighbors"
        assert after["stats_forward"]["dual"] == 0 and after["stats_reverse"]["dual"] == 0
        fwd = ref.algorithm.kneighbors_device(k=10)
        assert f.state("forward_dist").numpy().tobytes() == fwd[0].numpy().tobytes()
        assert f.state("forward_ind").numpy().tobytes() == fwd[1].numpy().tobytes()
    with pytest.raises(ValueError, match="unknown state"):
        f.state("nope")
    f.close()
    f.close()   # (idempotent)
    with pytest.raises(ValueError, match="closed"):
        f.kneighbors(1)


def test_facade_without_shared_sweep(ctx):
    from kiez_amd import _native as N
    s, t = _data(200, 300, np.float32, seed=2)
    for name, kwargs, _ in REDUCTIONS:
        ref = _kiez("cosine", name, kwargs, shared=False).fit(s, t)
        nat = _kiez("cosine", name, kwargs, native=True, shared=False).fit(s, t)
        assert nat.hubness._fitted.info["search"] == N.FIT_SEARCH_REVERSE and nat.hubness._fitted.info["forward_ready"] == 0
        for k in (10, 5):
            got = nat.kneighbors(k)
            assert got[0].dtype == np.float32
            _same(got, ref.kneighbors(k), f"{name}{kwargs} cosine float32 shared_sweep=0 k={k}")
        assert nat.hubness._fitted.info["n_searches"] == 2


@pytest.mark.parametrize("n,K,search", [(257, 10, "FIT_SEARCH_SPLIT"), (300, 110, "FIT_SEARCH_REVERSE")], ids=["split", "two-self-searches"])
def test_single_source(ctx, n, K, search):
    from kiez_amd import _native as N
    s, _ = _data(n, 0, np.float64, seed=3)
    for name, kwargs, _kind in REDUCTIONS:
        ref = _kiez("euclidean", name, kwargs, K=K).fit(s)
        nat = _kiez("euclidean", name, kwargs, K=K, native=True).fit(s)
        info = nat.hubness._fitted.info
        assert info["single_source"] == 1 and info["search"] == getattr(N, search) and info["n_target"] == n
        assert info["forward_ready"] == (1 if search == "FIT_SEARCH_SPLIT" else 0)
        a, b = _fitted_arrays(ref.hubness), _fitted_arrays(nat.hubness)
        assert set(a) == set(b)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), f"{name}{kwargs} single source n={n} K={K}: fitted attribute {key}"
        for k in (K, 5):
            _same(nat.kneighbors(k), ref.kneighbors(k), f"{name}{kwargs} single source n={n} K={K} k={k}")
        assert nat.hubness._fitted.info["n_searches"] == (1 if search == "FIT_SEARCH_SPLIT" else 2)


def test_beyond_the_fused_kernel(ctx):
    """K = 130 candidates: kz_rescale_select runs the kernel sequence inside the call."""
    from kiez_amd import _native as N
    s, t = _data(300, 300, np.float64, seed=4)
    ref = _kiez("euclidean", "CSLS", {}, K=130).fit(s, t)
    nat = _kiez("euclidean", "CSLS", {}, K=130, native=True).fit(s, t)
    info = nat.hubness._fitted.info
    assert info["tail"] == N.FIT_TAIL_FUSED and info["fused"] == 0 and info["n_candidates"] == 130
    for k in (130, 7):
        _same(nat.kneighbors(k), ref.kneighbors(k), f"CSLS K=130 k={k}")


def test_whole_index_calls_after_an_opt_in_fit(ctx):
    s, t = _data(300, 200, np.float64, seed=5)
    gold = np.arange(300, dtype=np.int64) % 200
    for name, kwargs, kind_name in REDUCTIONS:
        if kind_name == "HUB_MP_EMPIRIC":
            continue   # (no value outside the list: no rank over the whole index, with or without the flag)
        ref = _kiez("euclidean", name, kwargs).fit(s, t)
        nat = _kiez("euclidean", name, kwargs, native=True).fit(s, t)
        assert nat.gold_ranks(gold, reduced=True).tobytes() == ref.gold_ranks(gold, reduced=True).tobytes(), f"{name}{kwargs}: gold_ranks"
        _same(nat.kneighbors_whole_index(5), ref.kneighbors_whole_index(5), f"{name}{kwargs}: kneighbors_whole_index")
        _same(nat.kneighbors(5), ref.kneighbors(5), f"{name}{kwargs}: kneighbors after the whole-index calls")


def test_k_warnings_and_the_flag_is_ignored_elsewhere(ctx):
    """`_set_k_if_needed` warns as ever before the native call; reductions without a native fit ignore the flag."""
    from kiez_amd.hubness_reduction import DisSimLocal, InvertedSoftmax, NoHubnessReduction
    s, t = _data(300, 200, np.float64, seed=6)
    ref = _kiez("euclidean", "CSLS", {}).fit(s, t)
    nat = _kiez("euclidean", "CSLS", {}, native=True).fit(s, t)
    with pytest.warns(UserWarning, match="k > n_candidates"):
        got = nat.kneighbors(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same(got, ref.kneighbors(11), "k above n_candidates")
        with pytest.warns(UserWarning, match="No k supplied"):
            got = nat.kneighbors()
        _same(got, ref.kneighbors(), "k = None")
    for cls, kw, metric in ((NoHubnessReduction, {}, "euclidean"), (DisSimLocal, {}, "sqeuclidean"), (InvertedSoftmax, {}, "euclidean")):
        a = _kiez(metric, cls, kw).fit(s, t)
        b = _kiez(metric, cls, kw, native=True).fit(s, t)
        assert b.hubness._fitted is None
        _same(b.kneighbors(5), a.kneighbors(5), f"{cls.__name__} ignores native_fit")
    plain = _kiez("euclidean", "CSLS", {})
    assert plain.hubness._native_fit is False and type(plain.hubness)._native_fit is False


def test_refusals(ctx):
    from kiez_amd import _native as N
    s, t = _data(300, 200, np.float64, seed=7)
    sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
    for kind in (N.HUB_CSLS, N.HUB_LS, N.HUB_NICDM, N.HUB_MP_NORMAL, N.HUB_MP_EMPIRIC):
        with pytest.raises(ValueError, match="single candidate"):
            N.fit(ctx, sm, tm, kind, 1)
    N.fit(ctx, sm, tm, N.HUB_NONE, 1).close()                       # (no reduction: one candidate is a search like any other)
    with pytest.raises(ValueError, match="exceeds the rows of a side"):
        N.fit(ctx, sm, tm, N.HUB_CSLS, 201)
    with pytest.raises(ValueError, match="exceeds n - 1"):
        N.fit(ctx, sm, None, N.HUB_CSLS, 300)
    with pytest.raises(ValueError, match="unknown hubness kind"):
        N.fit(ctx, sm, tm, 6, 10)
    f = N.fit(ctx, sm, tm, N.HUB_CSLS, 10)
    made = []

    def alloc(shape, dtype):
        a = ctx.to_device(np.full(shape, 7, dtype=dtype))
        made.append(a)
        return a

    for k in (0, 11, -1):
        with pytest.raises(ValueError, match="kz_kneighbors"):
            f.kneighbors(k, alloc=alloc)
    with pytest.raises(ValueError, match="out_dtype"):
        f.kneighbors(5, np.int64)
    ctx.sync()
    assert len(made) == 6 and all((a.numpy() == 7).all() for a in made), "a refused kneighbors wrote into its outputs"
    # a precomputed pair
    rows, cols = N.DeviceMatrix.precomputed(ctx, np.abs(s @ t.T))
    with pytest.raises(NotImplementedError, match="precomputed"):
        N.fit(ctx, rows, cols, N.HUB_CSLS, 10)
    # float32 beside float64, another metric, another width
    with pytest.raises(ValueError, match="disagree"):
        N.fit(ctx, sm, N.DeviceMatrix(ctx, t.astype(np.float32), "euclidean"), N.HUB_CSLS, 10)
    with pytest.raises(ValueError, match="disagree"):
        N.fit(ctx, sm, N.DeviceMatrix(ctx, t, "cosine"), N.HUB_CSLS, 10)
    with pytest.raises(ValueError, match="disagree"):
        N.fit(ctx, sm, N.DeviceMatrix(ctx, t[:, :20].copy(), "euclidean"), N.HUB_CSLS, 10)
    # the facade falls back to the present pipeline where the plan refuses: a k that is clamped, precomputed input
    small_s, small_t = s[:8], t[:6]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = _kiez("euclidean", "CSLS", {}).fit(small_s, small_t)
        nat = _kiez("euclidean", "CSLS", {}, native=True).fit(small_s, small_t)
        assert nat.hubness._fitted is None
        _same(nat.kneighbors(3), ref.kneighbors(3), "clamped k: the present pipeline")
        dm = np.abs(s @ t.T)
        ref = _kiez("precomputed", "CSLS", {}).fit(dm)
        nat = _kiez("precomputed", "CSLS", {}, native=True).fit(dm)
        assert nat.hubness._fitted is None
        _same(nat.kneighbors(5), ref.kneighbors(5), "precomputed input: the present pipeline")
