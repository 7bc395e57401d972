"""Black-box search (avae_search_sample / avae_search_update, search / refine_motion) on a real MI355X (include/avae.h, DESIGN.md
section 25) against tests/search_reference.py.

1. the sampler and 2. the update against the float64 definition, within 4x the restatement's own worst error over the same inputs
(|err| / (|ref| + 1) per quantity, variances relative to the problem's largest), bit reproducibility and independence; 3. the loop;
4. refine_motion on the small fp32 model of test_gpu_render.py; 5. edges and errors of the C ABI.  The ``*_classes_*`` tests sweep
the tile and ownership classes of the two kernels (search_reference.SAMPLE_CLASS_SHAPES, UPDATE_CLASS_SHAPES, class_options; each
test's docstring names them).  The measured pairs are in README.md and DESIGN.md section 25."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as M
import render_reference as RR
import search_reference as S
from conftest import make_arch, synth_batch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V, ema=None):
    key = "ema" if ema else "m"
    if key not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS[key] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3, ema=ema)
    return _MODELS[key]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(model, a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(model.device)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(model):
    return C.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)


def _err(model):
    return model._L.avae_last_error(model._h).decode()


def _sample(model, mean, var, R, seed=5, iteration=3, offset=0, proj=None, rc_want=0, P=None, n=None, G=None, g=None, out=True):
    """avae_search_sample -> x [P, R, n] as NumPy (prefilled with -7)"""
    P = mean.shape[0] if P is None else P
    n = mean.shape[1] if n is None else n
    ts = [_dev(model, a) for a in (mean, var) + (proj if proj is not None else (None, None))]
    G = (proj[0].shape[0] if proj is not None else 0) if G is None else G
    g = (proj[0].shape[1] if proj is not None else 0) if g is None else g
    x = torch.full((max(P, 1), max(R, 1), max(n, 1)), -7.0, device=model.device)
    rc = model._L.avae_search_sample(model._h, _p(ts[0]), _p(ts[1]), P, R, n, seed, iteration, offset, _p(ts[2]), _p(ts[3]), G, g,
                                     _p(x) if out else None, _stream(model))
    torch.cuda.synchronize()
    assert (rc == 0) == (rc_want == 0), (rc, _err(model))
    return x.cpu().numpy()


def _options(V, opt):
    from vae_assoc_amd import _capi
    o = _capi.SearchOptions()
    o.weighting, o.cov_update = _capi.SEARCH_IDS[opt["weighting"]], _capi.SEARCH_IDS[opt["cov_update"]]
    o.eliteness, o.learning_rate, o.tol = opt["eliteness"], opt["lr"], opt["tol"]
    o.rel_lower, o.abs_lower, o.abs_upper = opt["rel_lower"], opt["abs_lower"], opt["abs_upper"]
    return o


HIST = ("avg_cost", "min_cost", "moved")


def _update(V, model, x, cost, st, opt, want=HIST, stream=None):
    """avae_search_update on copies of the state -> (new state as NumPy, history dict as NumPy; outputs prefilled with -7)"""
    P, R, n = x.shape
    d = dict(mean=_dev(model, st["mean"]), var=_dev(model, st["var"]), n_applied=_dev(model, st["n_applied"], np.int32),
             frozen=_dev(model, st["frozen"], np.int32), best_cost=_dev(model, st["best_cost"]), best_x=_dev(model, st["best_x"]))
    h = {k: torch.full((P,), -7.0, device=model.device) for k in want}
    xs, cs, o = _dev(model, x), _dev(model, cost), _options(V, opt)
    torch.cuda.synchronize()
    s = _stream(model) if stream is None else C.c_void_p(stream.cuda_stream)
    rc = model._L.avae_search_update(model._h, _p(xs), _p(cs), P, R, n, C.byref(o), _p(d["mean"]), _p(d["var"]), _p(d["n_applied"]),
                                     _p(d["frozen"]), _p(d["best_cost"]), _p(d["best_x"]), _p(h.get("avg_cost")), _p(h.get("min_cost")),
                                     _p(h.get("moved")), s)
    assert rc == 0, _err(model)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}, {k: v.cpu().numpy() for k, v in h.items()}


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return float((np.abs(got[ok] - ref[ok]) / (np.abs(ref[ok]) + 1.0)).max()) if ok.any() else 0.0


def _var_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = ref.max(1)
    return float((np.abs(got - ref).max(1) / np.where(top > 0, top, 1.0)).max())     # (all zero: one rollout about its own mean)


# ------------------------------------------------------------------------------------------------ 1. the sampler
def _sample_case(shape, seed=0, groups=S.SAMPLE_GROUPS):
    P, R, n = shape
    rng = np.random.default_rng(seed)
    mean, var = rng.standard_normal((P, n)).astype(np.float32), (0.05 + rng.random((P, n))).astype(np.float32)
    proj = None
    if n in groups:
        G, g = groups[n]
        proj = ((rng.standard_normal((G, g, g)) / np.sqrt(g)).astype(np.float32), rng.standard_normal((P, n)).astype(np.float32))
    return mean, var, proj


def _check_sample(model, shape, mean, var, proj):
    """the 4x rule without and with the map, the last problem alone with its problem_offset, repetition, other draws"""
    P, R, n = shape
    for pr in (None,) + ((proj,) if proj is not None else ()):
        r64, r32 = S.sample(mean, var, 5, 3, R, 0, pr), S.sample_restated(mean, var, 5, 3, R, 0, pr)
        got = _sample(model, mean, var, R, proj=pr)
        own, err = _rel(r32, r64), _rel(got, r64)
        print("sample %s%s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, " mapped" if pr else "", err, own))
        assert got.shape == r64.shape and err <= 4.0 * own
        # a problem alone with its problem_offset, repetition
        last = _sample(model, mean[-1:], var[-1:], R, offset=P - 1, proj=None if pr is None else (pr[0], pr[1][-1:]))
        assert _same(last, got[-1:]) and _same(_sample(model, mean, var, R, proj=pr), got)
        # another iteration, seed or offset is another draw in every row
        for kw in (dict(iteration=4), dict(seed=6), dict(offset=1), dict(seed=5 + (1 << 32))):
            assert (_sample(model, mean, var, R, proj=pr, **kw) != got).any(-1).all(), kw


@pytest.mark.parametrize("shape", S.SAMPLE_SHAPES)
def test_sample_against_the_definition(V, shape):
    _check_sample(_model(V), shape, *_sample_case(shape))


@pytest.mark.parametrize("shape", S.SAMPLE_CLASS_SHAPES)
def test_sample_classes_against_the_definition(V, shape):
    """The tile classes of k_search_sample (search_reference.SAMPLE_CLASS_SHAPES; a tile is 1024 / (4 ceil(n / 4)) rows):
    (3, 100, 3) 256-row tiles that straddle problems, the one quad partial; (4, 1024, 2) R = 1024; (2, 5, 1024) 256 full quads, one
    row a tile; (2, 3, 1021) the last quad partial; (1, 7, 513) 129 quads; (2, 9, 340) tiles of 3 rows; (3, 6, 128) with (G, g) =
    (2, 64), the largest g; (7, 50, 5) g = 1 with G = n; (2, 17, 64) G = 1 with g = n; n = 1024 with (16, 64).  Next to the checks of
    the workload shapes: a variance of zero gives the mean, bit for bit, and with a map the map of the mean within 4x."""
    model = _model(V)
    P, R, n = shape
    mean, var, proj = _sample_case(shape, groups=S.SAMPLE_CLASS_GROUPS)
    assert (proj is not None) == (n in S.SAMPLE_CLASS_GROUPS)
    _check_sample(model, shape, mean, var, proj)
    zero = np.zeros_like(var)
    got = _sample(model, mean, zero, R)
    assert _same(got, np.broadcast_to(mean[:, None, :], (P, R, n)))
    if proj is not None:
        r64, r32 = S.sample(mean, zero, 5, 3, R, 0, proj), S.sample_restated(mean, zero, 5, 3, R, 0, proj)
        got = _sample(model, mean, zero, R, proj=proj)
        own, err = _rel(r32, r64), _rel(got, r64)
        print("sample %s mapped, var = 0: kernel %.3e, restatement %.3e (bound 4x)" % (shape, err, own))
        assert err <= 4.0 * own and _same(got, np.broadcast_to(got[:, :1], got.shape))


def test_sample_moments(V):
    model = _model(V)
    rng = np.random.default_rng(1)
    P, R, n = 3, 1024, 6
    mean, var = rng.standard_normal((P, n)).astype(np.float32), (0.05 + rng.random((P, n))).astype(np.float32)
    x = _sample(model, mean, var, R, seed=11, iteration=0).astype(np.float64)
    se = np.sqrt(var / R)
    assert (np.abs(x.mean(1) - mean) < 5.0 * se).all()
    assert (np.abs(x.var(1) - var) < 5.0 * var * np.sqrt(2.0 / R)).all()


# ------------------------------------------------------------------------------------------------ 2. the update
def _check_update(V, model, shape, cases, seed=2):
    """``cases``: [(family, options, rel)] (rel: search_reference.class_options).  n_applied and frozen equal to both references,
    the best rollout bitwise the restatement's, every history entry written, untouched problems unchanged, the 4x rule on the rest"""
    P, R, n = shape
    rng = np.random.default_rng(seed)
    own = dict(mean=0.0, var=0.0, avg_cost=0.0, min_cost=0.0, moved=0.0)
    err = dict(own)
    for family, opt, rel in cases:
        x, c, st = S.update_case(P, R, n, family, rng)
        if rel is not None:
            opt = S.with_abs_lower(x, c, st, opt, rel)
        d64, h64 = S.update(x, c, st, opt)
        d32, h32 = S.update_restated(x, c, st, opt)
        got, hg = _update(V, model, x, c, st, opt)
        for k in ("n_applied", "frozen"):
            assert np.array_equal(got[k], d64[k]) and np.array_equal(got[k], d32[k]), (family, opt, k)
        assert _same(got["best_cost"], d32["best_cost"]) and _same(got["best_x"], d32["best_x"]), (family, opt)
        for k in HIST:
            assert not (hg[k] == -7.0).any(), (family, k)                          # every entry is written
            own[k], err[k] = max(own[k], _rel(h32[k], h64[k])), max(err[k], _rel(hg[k], h64[k]))
        own["mean"], err["mean"] = max(own["mean"], _rel(d32["mean"], d64["mean"])), max(err["mean"], _rel(got["mean"], d64["mean"]))
        own["var"], err["var"] = max(own["var"], _var_err(d32["var"], d64["var"])), max(err["var"], _var_err(got["var"], d64["var"]))
        untouched = d64["n_applied"] == 0                                          # all NaN: bit for bit what it was
        assert _same(got["mean"][untouched], st["mean"][untouched].astype(np.float32))
        assert _same(got["var"][untouched], st["var"][untouched].astype(np.float32))
    for k in own:
        print("update %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, k, err[k], own[k]))
        assert err[k] <= 4.0 * own[k], k


@pytest.mark.parametrize("shape", S.UPDATE_SHAPES)
def test_update_against_the_definition(V, shape):
    _check_update(V, _model(V), shape, [(family, opt, None) for family, opt in S.option_grid()])


@pytest.mark.parametrize("shape", S.UPDATE_CLASS_SHAPES)
def test_update_classes_against_the_definition(V, shape):
    """The ownership classes of k_search_update (search_reference.UPDATE_CLASS_SHAPES; a thread owns the rollouts and the dimensions
    i, i + 256, ...): (1, 257, 257) one rollout and one dimension past the first trip; (3, 256, 256) exactly one trip; (1, 1024,
    1024) four of each; (2, 255, 1) one thread without a rollout, one dimension; (2, 2, 513) two rollouts, a third dimension for
    thread 0.  Over the option grid of the workload shapes and search_reference.class_options: PI-BB with eliteness 2000 (exp
    underflows, the w == 0 skip) and 0; CEM keeping one rollout with its own covariance rule and abs_lower alone; CMA-ES keeping
    more than there are, a NaN among them, abs_upper alone; learning rate 0 with rel_lower 0.5; every bound 0; rel_lower * vmax
    just below and just above abs_lower."""
    _check_update(V, _model(V), shape, [(family, opt, None) for family, opt in S.option_grid()] + S.class_options())


def test_update_alone_frozen_streams_and_optional_outputs_give_the_same_bits(V):
    model = _model(V)
    rng = np.random.default_rng(3)
    P, R, n = 5, 7, 63
    x, c, st = S.update_case(P, R, n, "one_nan", rng)
    st["frozen"][1] = 1
    c[3] = np.nan
    for opt in (S.options(), S.options(weighting=S.CEM, eliteness=3, cov_update=S.CEM, lr=0.5, abs_lower=0.01, abs_upper=0.8)):
        got, hg = _update(V, model, x, c, st, opt)
        for p in (1, 3):                                                           # frozen / all NaN
            assert _same(got["mean"][p], st["mean"][p].astype(np.float32)) and _same(got["var"][p], st["var"][p].astype(np.float32))
            assert got["n_applied"][p] == 0 and all(np.isnan(hg[k][p]) for k in HIST)
        assert got["n_applied"].tolist() == [1, 0, 1, 0, 1] and got["frozen"].tolist() == [0, 1, 0, 0, 0]
        assert got["best_cost"][1] == min(st["best_cost"][1], np.nanmin(c[1]))     # a frozen problem still keeps the best it saw
        for p in range(P):                                                         # a problem alone
            one = {k: (v[p:p + 1] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
            alone, ha = _update(V, model, x[p:p + 1], c[p:p + 1], one, opt)
            assert all(_same(alone[k], got[k][p:p + 1]) for k in alone) and all(_same(ha[k], hg[k][p:p + 1]) for k in HIST), p
        side = torch.cuda.Stream(device=model.device)
        again, hs = _update(V, model, x, c, st, opt, stream=side)
        side.synchronize()
        assert all(_same(again[k], got[k]) for k in got) and all(_same(hs[k], hg[k]) for k in HIST)
        bare, hb = _update(V, model, x, c, st, opt, want=("moved",))
        assert all(_same(bare[k], got[k]) for k in got) and _same(hb["moved"], hg["moved"])


# ------------------------------------------------------------------------------------------------ 3. the loop
def _norm_cost(x, idx):
    return torch.linalg.vector_norm(x, dim=1)


QUADRATIC = [dict(n=2, x0=5.0, var0=1.0, R=10, iters=40, bound=0.01), dict(n=20, x0=1.0, var0=0.01, R=20, iters=60, bound=0.1)]


@pytest.mark.parametrize("case", QUADRATIC, ids=["n2", "n20"])
def test_search_converges_on_the_norm_cost(V, case):
    model = _model(V)
    x0 = torch.full((3, case["n"]), case["x0"], device=model.device)
    res = model.search(_norm_cost, x0, case["var0"], n_rollouts=case["R"], n_iters=case["iters"], tol=0.0, seed=0)
    ratio = (torch.linalg.vector_norm(res["mean"], dim=1) / torch.linalg.vector_norm(x0, dim=1)).cpu().numpy()
    print("n = %d: |mean| / |x0| = %s (bound %g)" % (case["n"], ratio, case["bound"]))
    assert (ratio < case["bound"]).all() and (res["n_applied"] == case["iters"]).all()
    assert torch.isfinite(res["avg_cost"]).all() and res["avg_cost"].shape == (case["iters"], 3)
    assert (res["best_cost"] <= res["min_cost"].min(0).values).all()


def test_search_continues_chunks_and_does_not_synchronise(V):
    model = _model(V)
    P, n, R = 5, 20, 20
    x0 = torch.from_numpy(np.random.default_rng(4).standard_normal((P, n)).astype(np.float32)).to(model.device)
    kw = dict(n_rollouts=R, tol=0.0, seed=7)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                        # a host round trip inside the loop raises
    try:
        whole = model.search(_norm_cost, x0, 0.01, n_iters=10, **kw)
        first = model.search(_norm_cost, x0, 0.01, n_iters=4, **kw)
        both = model.search(_norm_cost, None, None, n_iters=6, state=first["state"], **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    keys = ("mean", "var", "best_x", "best_cost", "n_applied")
    assert all(_same(whole[k], both[k]) for k in keys) and whole["state"]["iteration"] == both["state"]["iteration"] == 10
    for k in HIST:
        assert _same(whole[k], torch.cat([first[k], both[k]]))
    assert first["state"]["iteration"] == 4                                        # (the state handed in is not the one updated)
    keep = model._motion_chunk
    try:
        type(model)._motion_chunk = R                                              # one problem per cost call
        seen = []
        small = model.search(lambda x, idx: (seen.append((tuple(x.shape), idx)), _norm_cost(x, idx))[1], x0, 0.01, n_iters=10, **kw)
    finally:
        type(model)._motion_chunk = keep
    assert len(seen) == 10 * P and seen[1][0] == (R, n) and (seen[1][1] == 1).all()
    assert all(_same(whole[k], small[k]) for k in keys + HIST)
    # NumPy in gives NumPy out
    as_np = model.search(_norm_cost, x0.cpu().numpy(), 0.01, n_iters=10, **kw)
    assert isinstance(as_np["mean"], np.ndarray) and all(_same(whole[k], as_np[k]) for k in keys + HIST)
    with pytest.raises(ValueError):
        model.search(lambda x, idx: _norm_cost(x, idx)[:-1], x0, 0.01, n_iters=1, **kw)


def test_search_freezes_and_keeps_the_best(V):
    model = _model(V)
    x0 = torch.tensor([[5.0, 5.0], [1e-9, 0.0], [1.0, -2.0]], device=model.device)
    var0 = torch.tensor([[1.0, 1.0], [1e-20, 1e-20], [1.0, 1.0]], device=model.device)
    res = model.search(_norm_cost, x0, var0, n_rollouts=6, n_iters=4, covar_bounds=None, tol=1e-6, seed=1)
    assert res["n_applied"].tolist() == [4, 1, 4] and res["state"]["frozen"].tolist() == [0, 1, 0]
    moved = res["moved"].cpu().numpy()
    assert np.isfinite(moved[0]).all() and np.isnan(moved[1:, 1]).all() and np.isfinite(moved[:, [0, 2]]).all()
    assert np.isnan(res["avg_cost"].cpu().numpy()[1:, 1]).all()
    once = model.search(_norm_cost, x0, var0, n_rollouts=6, n_iters=1, covar_bounds=None, tol=1e-6, seed=1)
    assert _same(once["mean"][1], res["mean"][1]) and _same(once["var"][1], res["var"][1])        # frozen: unchanged from then on
    # best_cost never rises along continued runs
    best, st = [], None
    for k in (1, 2, 3):
        r = model.search(_norm_cost, x0, var0, n_rollouts=6, n_iters=k, covar_bounds=None, tol=0.0, seed=2, state=st)
        st = r["state"]
        best.append(r["best_cost"].cpu().numpy())
        assert _same(r["best_cost"], _norm_cost(r["best_x"], None))
    assert (best[1] <= best[0]).all() and (best[2] <= best[1]).all() and st["iteration"] == 6


# ------------------------------------------------------------------------------------------------ 4. refine_motion
def _writer():
    from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    fx = RR.fixture()
    chain = KinematicChain(fx["joints"])
    mean = np.zeros((7, 21))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(147, 0.012))
    return basis, chain, StrokeCanvas()


def _pictures(model, basis, chain, canvas, P=3, seed=5):
    """P pictures drawn from the model's own decoded motions"""
    z = np.random.default_rng(seed).standard_normal((P, NZ)).astype(np.float32)
    return model.draw_motion(model.generate(z)[1], basis, chain, canvas)["image"]


def _tile(a, R):
    return np.repeat(a, R, axis=0)


@pytest.mark.parametrize("space", ["latent", "params"])
def test_refine_motion_is_search_around_writing_cost(V, space):
    model = _model(V)
    basis, chain, canvas = _writer()
    P, R = 3, 5
    img = _pictures(model, basis, chain, canvas, P)
    res = model.refine_motion(img, basis, chain, canvas, space=space, n_rollouts=R, n_iters=2, seed=9, tol=0.0)
    assert res["params"].shape == (P, 147) and res["image"].shape == (P, 784) and res["avg_cost"].shape == (2, P)
    assert (res["n_applied"] == 2).all() and np.isfinite(res["avg_cost"]).all()
    zt = model.transform(img, 0)
    start = model.generate(zt)[1]
    # initial and final are writing_cost at the start and at params
    for name, params in (("initial", start), ("final", res["params"])):
        c = model.writing_cost(params, basis, chain, canvas, img, target_latent=zt, height=res["height"])
        assert all(_same(res[name][k], c[k]) for k in ("cost", "img_l2", "height_l2", "latent_l2")), name
        if name == "final":
            assert _same(res["image"], c["image"])
    own = model.writing_cost(start, basis, chain, canvas, img)                     # the height: the initial motion's own mean height
    assert _same(own["cost"], res["initial"]["cost"])
    # iteration 0's average cost is the mean of writing_cost over the candidates avae_search_sample gives for that seed
    proj = None
    if space == "latent":
        mean0, var0 = zt, np.full((P, NZ), 0.01, np.float32)
        assert _same(res["z"], res["mean"]) and _same(res["params"], model.generate(res["z"])[1])
    else:
        mean0, var0 = start, np.tile((0.001 / basis.param_std ** 2).astype(np.float32), (P, 1))
        traj0 = model.motion_eval(start, basis)["trajectory"]
        A, b = basis.projection([0.0], traj0[:, 0, :].reshape(P, 7, 1))
        proj = (A.astype(np.float32), b.astype(np.float32))
        assert res["z"] is None and _same(res["params"], res["mean"])
    x = _sample(model, mean0, var0, R, seed=9, iteration=0, proj=proj).reshape(P * R, -1)
    cand = model.generate(x)[1] if space == "latent" else x
    c = model.writing_cost(cand, basis, chain, canvas, _tile(img, R), target_latent=_tile(zt, R), height=_tile(res["height"], R))
    want = (c["cost"].reshape(P, R).astype(np.float64).sum(1) / R).astype(np.float32)
    assert _same(res["avg_cost"][0], want) and _same(res["min_cost"][0], c["cost"].reshape(P, R).min(1))
    if space == "params":
        # the refined motion starts where the initial one does: within 4x what the float32 restatement of projection + evaluation
        # leaves on the raw candidates of iteration 0
        raw = _sample(model, mean0, var0, R, seed=9, iteration=0)
        x32 = S.sample_restated(mean0, var0, 9, 0, R, 0, proj).reshape(P * R, -1)
        assert np.abs(x32 - x).max() < 1e-5 and np.abs(raw.reshape(P * R, -1) - x).max() > 1e-3
        sc, sh = basis.scale_shift()
        phi = basis.eval_matrices()[0][:1]
        s32 = M.eval32(x32, phi, 7, sc, sh, basis.limits)[0][:, 0, :]
        own_err = RR.rel_err(s32, _tile(traj0[:, 0, :], R))
        got = model.motion_eval(res["params"], basis)["trajectory"][:, 0, :]
        err = RR.rel_err(got, traj0[:, 0, :])
        print("anchored start: refined %.3e, restatement %.3e (bound 4x)" % (err, own_err))
        assert err <= 4.0 * own_err
        free = model.refine_motion(img, basis, chain, canvas, space="params", n_rollouts=R, n_iters=2, seed=9, tol=0.0, anchor_start=False)
        assert RR.rel_err(model.motion_eval(free["params"], basis)["trajectory"][:, 0, :], traj0[:, 0, :]) > 10.0 * own_err
    # device tensors in give device tensors out, the same bits
    dev = model.refine_motion(torch.from_numpy(img).to(model.device), basis, chain, canvas, space=space, n_rollouts=R, n_iters=2, seed=9,
                              tol=0.0)
    assert torch.is_tensor(dev["params"]) and _same(dev["params"], res["params"]) and _same(dev["final"]["cost"], res["final"]["cost"])


def test_a_candidate_that_cannot_be_drawn_costs_nan_and_moves_nothing_else(V):
    model = _model(V)
    basis, chain, canvas = _writer()
    P, R = 3, 5
    img = torch.from_numpy(_pictures(model, basis, chain, canvas, P)).to(model.device)
    zt = model.transform(img, 0)
    start = model.generate(zt)[1]
    h = model.writing_cost(start, basis, chain, canvas, img)["path"] @ torch.from_numpy(canvas.plane[2].astype(np.float32)).to(model.device)
    h = h.mean(1)
    costs = []

    def price(broken):
        def f(cand, idx):
            if broken:
                cand = cand.clone()
                cand[3, 5] = float("nan")                                          # problem 0, rollout 3: its path is not finite
            c = model.writing_cost(cand, basis, chain, canvas, img[idx], target_latent=zt[idx], height=h[idx])["cost"]
            costs.append(c)
            return c
        return f
    kw = dict(n_rollouts=R, n_iters=1, seed=3, tol=0.0)
    bad = model.search(price(True), start, 0.001, **kw)
    good = model.search(price(False), start, 0.001, **kw)
    cb, cg = costs[0].cpu().numpy(), costs[1].cpu().numpy()
    assert np.isnan(cb[3]) and np.isfinite(np.delete(cb, 3)).all() and _same(np.delete(cb, 3), np.delete(cg, 3))
    for k in ("mean", "var", "best_x", "best_cost"):
        assert _same(bad[k][1:], good[k][1:]) and torch.isfinite(bad[k]).all(), k
    assert not _same(bad["mean"][0], good["mean"][0]) and (bad["n_applied"] == 1).all()
    # ... and the update is the one of the other four rollouts
    x = _sample(model, start.cpu().numpy(), np.full((P, 147), 0.001, np.float32), R, seed=3, iteration=0)
    st = S.new_state(start.cpu().numpy(), 0.001)
    want, _ = _update(V, model, x, cb.reshape(P, R), st, S.options(tol=0.0))
    assert _same(want["mean"], bad["mean"]) and _same(want["var"], bad["var"])


def test_refine_motion_inside_averaged(V):
    model = _model(V, ema=0.9)
    basis, chain, canvas = _writer()
    rng = np.random.default_rng(6)
    X = synth_batch(rng, B, (784, 147), (True, False))
    model.partial_fit(X, rng.standard_normal((B, NZ)).astype(np.float32))
    img = _pictures(model, basis, chain, canvas, 2)
    live = model.refine_motion(img, basis, chain, canvas, n_rollouts=4, n_iters=1, seed=1)
    with model.averaged():
        avg = model.refine_motion(img, basis, chain, canvas, n_rollouts=4, n_iters=1, seed=1)
        zt = model.transform(img, 0)
        c = model.writing_cost(model.generate(zt)[1], basis, chain, canvas, img, target_latent=zt, height=avg["height"])
    assert _same(avg["initial"]["cost"], c["cost"]) and not _same(avg["initial"]["cost"], live["initial"]["cost"])
    assert np.isfinite(avg["final"]["cost"]).all() and (avg["n_applied"] == 1).all()


# ------------------------------------------------------------------------------------------------ 5. edges and errors
def test_c_abi_errors_name_the_argument_and_launch_nothing(V):
    model = _model(V)
    mean, var, proj = _sample_case((2, 20, 147))
    ok = dict(mean=mean, var=var, R=20)
    for kw, needle in ((dict(P=-1), "P"), (dict(R=0), "R"), (dict(R=1025), "R"), (dict(n=0), "n"), (dict(n=1025), "n"),
                       (dict(iteration=-1), "iteration"), (dict(offset=-1), "problem_offset"), (dict(offset=(1 << 32) - 1), "problem_offset"),
                       (dict(mean=None, P=2, n=147), "mean_dev"), (dict(var=None), "var_dev"), (dict(out=False), "x_dev"),
                       (dict(proj=(proj[0], None), G=7, g=21), "proj"), (dict(proj=(None, proj[1]), G=7, g=21), "proj"),
                       (dict(proj=proj, G=7, g=20), "G * g"), (dict(proj=proj, G=1, g=147), "g"), (dict(proj=proj, G=0, g=21), "G * g")):
        got = _sample(model, **dict(ok, rc_want=1, **kw))
        assert needle in _err(model), (kw, _err(model))
        assert (got == -7.0).all(), kw
    assert (_sample(model, mean, var, 20, P=0) == -7.0).all()                      # P == 0 is a no-op
    assert (_sample(model, mean[:1], var[:1], 20, offset=(1 << 32) - 1) != -7.0).all()
    # the update
    x, c, st = S.update_case(2, 5, 4, "spread", np.random.default_rng(0))
    d = dict(x=_dev(model, x), cost=_dev(model, c), mean=_dev(model, st["mean"]), var=_dev(model, st["var"]),
             n_applied=_dev(model, st["n_applied"], np.int32), frozen=_dev(model, st["frozen"], np.int32),
             best_cost=_dev(model, st["best_cost"]), best_x=_dev(model, st["best_x"]))
    before = {k: v.clone() for k, v in d.items()}

    def call(P=2, R=5, n=4, opt=None, no_opt=False, **nulls):
        o = _options(V, S.options() if opt is None else opt)
        a = {k: (None if nulls.get(k) else _p(v)) for k, v in d.items()}
        return model._L.avae_search_update(model._h, a["x"], a["cost"], P, R, n, None if no_opt else C.byref(o), a["mean"], a["var"],
                                           a["n_applied"], a["frozen"], a["best_cost"], a["best_x"], None, None, None, _stream(model))
    bad_opts = [(dict(weighting=S.PIBB, eliteness=-1.0), "eliteness"), (dict(weighting=S.CEM, eliteness=2.5), "eliteness"),
                (dict(weighting=S.CMAES, eliteness=0.0), "eliteness"), (dict(lr=1.5), "learning_rate"), (dict(lr=float("nan")), "learning_rate"),
                (dict(rel_lower=1.5), "rel_lower"), (dict(abs_upper=float("inf")), "abs_upper"), (dict(tol=-1.0), "tol"),
                (dict(tol=float("nan")), "tol")]
    for kw, needle in [(dict(P=-1), "P"), (dict(R=0), "R"), (dict(R=1025), "R"), (dict(n=0), "n"), (dict(n=1025), "n"),
                       (dict(no_opt=True), "opt")] + [(dict(**{k: True}), k + "_dev") for k in d] \
            + [(dict(opt=S.options(**o)), nd) for o, nd in bad_opts]:
        assert call(**kw) != 0, kw
        assert needle in _err(model), (kw, _err(model))
    for wid, cid, needle in ((3, 0, "weighting"), (-1, 0, "weighting"), (0, 2, "cov_update")):
        o = _options(V, S.options())
        o.weighting, o.cov_update = wid, cid
        a = {k: _p(v) for k, v in d.items()}
        assert model._L.avae_search_update(model._h, a["x"], a["cost"], 2, 5, 4, C.byref(o), a["mean"], a["var"], a["n_applied"], a["frozen"],
                                           a["best_cost"], a["best_x"], None, None, None, _stream(model)) != 0
        assert needle in _err(model)
    assert call(P=0) == 0
    torch.cuda.synchronize()
    assert all(_same(before[k], d[k]) for k in d)                                   # nothing was launched
    assert call() == 0                                                              # the history outputs are optional
    torch.cuda.synchronize()
    assert (d["n_applied"] == 1).all() and not _same(before["mean"], d["mean"])
