"""Gradients through the writing chain (avae_stroke_render_vjp / avae_motion_fk_vjp / avae_motion_eval_vjp / avae_rows_adam and
render_strokes_vjp / motion_fk_vjp / motion_eval_vjp / rows_adam / writing_cost_grad / descend_motion) on a real MI355X
(include/avae.h) against tests/render_grad_reference.py.

Every kernel against the float64 definition, within 4x the float32 restatement's own worst error over the same inputs (the rule
of test_gpu_motion.py), the error of a row taken relative to the largest |gradient| of that row.  The renderer's fixtures are the
general-position families (letter, scribble, outlier) on which test_render_grad_cpu.py shows the float32 and float64 decisions to
be equal, so both sides differentiate the same piece; the tie families are checked for what does not hang on a tie-break.  Then
bit reproducibility, the forward outputs' bits, non-finite rows, and descend_motion."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as MR
import render_grad_reference as G
import render_reference as RR
import vae_assoc_amd.vae_assoc as VA
from conftest import make_arch

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


def _model(V):
    """one small fp32 relu model (the c5_small-sized nets of the other GPU tests), shared by every test here"""
    if "m" not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS["m"] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3)
    return _MODELS["m"]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _canvas(shape, params, plane):
    from vae_assoc_amd.kinematics import StrokeCanvas
    return StrokeCanvas(half_width=params[0], size=shape[1], supersample=shape[2], margin=params[1], plane=np.asarray(plane, np.float64))


_call = G.call


def _cotangents(c, subset):
    """the cotangents of a subset of (image, img_l2, height_l2) -> keyword arguments of the three implementations"""
    N = len(c["path"])
    return dict(g_image=c["g_image"] if "image" in subset else None,
                g_img_l2=np.full(N, G.W_COST[0], np.float32) if "img_l2" in subset else None,
                g_height_l2=np.full(N, G.W_COST[1], np.float32) if "height_l2" in subset else None)


ALL = ("image", "img_l2", "height_l2")


def _three_ways(model, shape, params, c, subset=ALL):
    """-> (kernel, float64 definition, float32 restatement) gradients [N, T, 3] of one call"""
    T, H, ss = shape
    r, mg = np.float32(params[0]), np.float32(params[1])
    kw = _cotangents(c, subset)
    tg = c["target"] if "img_l2" in subset else None
    hg = c["height"] if "height_l2" in subset else None
    got = VA.render_strokes_vjp(model, c["path"], _canvas(shape, params, c["plane"]), target=tg, height=hg, **kw)["grad_path"]
    r64 = G.render_vjp64(c["path"], c["plane"], r, mg, H, ss, tg, hg, **kw)
    r32 = G.render_vjp32(c["path"], c["plane"], r, mg, H, ss, tg, hg, **kw)
    return got, r64, r32


# ------------------------------------------------------------------------------------------------ 1. the renderer's reverse pass
@pytest.mark.parametrize("shape", G.GPU_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_render_vjp_against_the_definition(V, shape):
    model = _model(V)
    own = got = 0.0
    for params, c in G.gpu_calls(shape):
        g, r64, r32 = _three_ways(model, shape, params, c)
        assert g.shape == r64.shape and np.isfinite(g).all()
        own, got = max(own, float(G.grad_err(r32, r64).max())), max(got, float(G.grad_err(g, r64).max()))
    print("render vjp %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, got, own))
    assert got <= 4.0 * own
    if shape[0] == 1:                                     # T = 1: the image part is exactly 0
        c = _call(shape, ("letter",), False)
        g, _, _ = _three_ways(model, shape, G.GPU_PARAMS[0], c, ("image", "img_l2"))
        assert not g.any()


SUBSETS = [s for s in (("image",), ("img_l2",), ("height_l2",), ("image", "img_l2"), ("image", "height_l2"), ("img_l2", "height_l2"), ALL)]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s))
def test_render_vjp_every_subset_of_cotangents(V, subset):
    model = _model(V)
    shape = G.SUBSET_CALL[0]
    c = _call(*G.SUBSET_CALL)
    g, r64, r32 = _three_ways(model, shape, G.GPU_PARAMS[0], c, subset)
    own, got = float(G.grad_err(r32, r64).max()), float(G.grad_err(g, r64).max())
    print("render vjp %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, "+".join(subset), got, own))
    assert got <= 4.0 * own


def test_render_vjp_call_of_65_rows(V):
    model = _model(V)
    shape = G.MANY_CALL[0]
    c = _call(*G.MANY_CALL)
    g, r64, r32 = _three_ways(model, shape, G.GPU_PARAMS[0], c)
    own, got = float(G.grad_err(r32, r64).max()), float(G.grad_err(g, r64).max())
    print("render vjp %s x 65: kernel %.3e, restatement %.3e (bound 4x)" % (shape, got, own))
    assert got <= 4.0 * own


def _raw_vjp(model, c, shape, params, want_forward, subset=ALL, stream=None):
    """avae_stroke_render_vjp itself, with or without the forward outputs -> dict of device tensors"""
    T, H, ss = shape
    N = len(c["path"])
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)   # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                                                                     # noqa: E731
    kw = _cotangents(c, subset)
    path, plane, tg, hg = dev(c["path"]), dev(c["plane"]), dev(c["target"]), dev(c["height"])
    gi, gl, gh = dev(kw["g_image"]), dev(kw["g_img_l2"]), dev(kw["g_height_l2"])
    out = dict(grad_path=torch.full((N, T, 3), 7.0, device=model.device))
    if want_forward:
        out.update(image=torch.empty((N, H * H), device=model.device), window=torch.empty((N, 3), device=model.device),
                   img_l2=torch.empty(N, device=model.device), height_l2=torch.empty(N, device=model.device),
                   objective=torch.empty(N, device=model.device))
    s = C.c_void_p((stream or torch.cuda.current_stream(model.device)).cuda_stream)
    rc = model._L.avae_stroke_render_vjp(model._h, p(path), N, T, p(plane), float(np.float32(params[0])), float(np.float32(params[1])),
                                         H, ss, p(tg), p(hg), p(gi), p(gl), p(gh), p(out["grad_path"]), p(out.get("image")),
                                         p(out.get("window")), p(out.get("img_l2")), p(out.get("height_l2")), p(out.get("objective")), s)
    assert rc == 0, model._L.avae_last_error(model._h)
    return out


def test_forward_outputs_are_the_forward_kernels_bits(V):
    """on request the reverse pass writes image, window, img_l2, height_l2: bitwise render_strokes', every family, both pens"""
    model = _model(V)
    shape = (100, 28, 4)
    for params in G.GPU_PARAMS:
        c = _call(shape, G.GRAD_FAMILIES + G.TIE_FAMILIES, False, seed=2)
        fwd = model.render_strokes(c["path"], _canvas(shape, params, c["plane"]), target=c["target"], height=c["height"])
        out = _raw_vjp(model, c, shape, params, True)
        for k in ("image", "window", "img_l2", "height_l2"):
            assert _same(out[k], fwd[k]), k
        obj = G.W_COST[0] * fwd["img_l2"].astype(np.float64) + G.W_COST[1] * fwd["height_l2"].astype(np.float64)
        assert np.abs(out["objective"].cpu().numpy() - obj).max() <= 1e-6 * np.abs(obj).max()
        assert np.isfinite(out["grad_path"].cpu().numpy()).all()
        lean = _raw_vjp(model, c, shape, params, False)
        assert _same(lean["grad_path"], out["grad_path"])                # whichever optional outputs are asked for


def test_tie_families_are_finite_and_sum_to_zero_in_the_plane(V):
    """dot, lines, repeated points, diagonal, frame: the gradient is finite, and the in-plane part sums to 0 over the points (to
    the restatement's own rounding)"""
    model = _model(V)
    shape = (100, 28, 4)
    for params in G.GPU_PARAMS:
        c = _call(shape, G.TIE_FAMILIES, False, seed=4)
        g = VA.render_strokes_vjp(model, c["path"], _canvas(shape, params, c["plane"]), target=c["target"],
                                     **_cotangents(c, ("image", "img_l2")))["grad_path"].astype(np.float64)
        assert np.isfinite(g).all()
        pl = c["plane"].astype(np.float64)
        assert np.abs(g @ pl[2]).max() <= 1e-5 * max(np.abs(g).max(), 1e-30) * np.abs(pl).max()          # nothing along the normal
        for i in range(len(g)):                                         # against what the sums are made of: the samples' pulls
            pull = G.render_vjp64_row(c["path"][i], pl, params[0], params[1], shape[1], shape[2], c["target"][i], None,
                                      c["g_image"][i], G.W_COST[0], None).get("pull", 0.0) * np.abs(pl[:2]).max()
            assert np.abs(g[i].sum(0)).max() <= 1e-5 * pull + 1e-30, (G.TIE_FAMILIES[i], g[i].sum(0), pull)


def test_a_nan_row_stays_in_its_own_row(V):
    model = _model(V)
    shape = (100, 28, 4)
    c = _call(shape, ("letter", "scribble", "outlier", "letter"), False, seed=6)
    clean = _raw_vjp(model, c, shape, G.GPU_PARAMS[0], True)
    bad = dict(c, path=c["path"].copy())
    bad["path"][2, 17, 1] = np.nan
    out = _raw_vjp(model, bad, shape, G.GPU_PARAMS[0], True)
    for k, v in out.items():
        v, w = v.cpu().numpy(), clean[k].cpu().numpy()
        assert np.isnan(v[2]).all(), k
        keep = [0, 1, 3]
        assert _same(v[keep], w[keep]), k
    # a non-finite cotangent: the image part of its own row, nothing else
    poisoned = dict(c, g_image=c["g_image"].copy())
    poisoned["g_image"][1, 5] = np.inf
    out = _raw_vjp(model, poisoned, shape, G.GPU_PARAMS[0], False)["grad_path"].cpu().numpy()
    assert np.isnan(out[1]).all() and _same(out[[0, 2, 3]], clean["grad_path"].cpu().numpy()[[0, 2, 3]])


def test_a_rows_gradient_is_the_same_bits_alone_among_65_on_two_streams_and_again(V):
    model = _model(V)
    shape = (100, 28, 4)
    c = _call(shape, (G.GRAD_FAMILIES * 22)[:65], True, seed=8)
    many = _raw_vjp(model, c, shape, G.GPU_PARAMS[0], False)["grad_path"]
    again = _raw_vjp(model, c, shape, G.GPU_PARAMS[0], True)["grad_path"]
    assert _same(many, again)
    for i in (0, 31, 64):
        one = {k: (v if k == "plane" else v[i:i + 1]) for k, v in c.items()}
        assert _same(_raw_vjp(model, one, shape, G.GPU_PARAMS[0], False)["grad_path"][0], many[i])
    side = torch.cuda.Stream(device=model.device)
    with torch.cuda.stream(side):
        other = _raw_vjp(model, c, shape, G.GPU_PARAMS[0], False, stream=side)["grad_path"]
    side.synchronize()
    assert _same(other, many)


# ------------------------------------------------------------------------------------------------ 2. forward kinematics, reversed
@pytest.mark.parametrize("shape", RR.FK_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_fk_vjp_against_the_definition(V, shape):
    model = _model(V)
    c = RR.fk_case(shape)
    g = np.random.default_rng([9] + list(shape)).standard_normal(c["traj"].shape[:2] + (3,)).astype(np.float32)
    got = VA.motion_fk_vjp(model, c["traj"], c["chain"], g)
    r64, r32 = G.fk_vjp64(c["traj"], c["frames"], c["axes"], g), G.fk_vjp32(c["traj"], c["frames"], c["axes"], g)
    own, err = float(G.grad_err(r32, r64).max()), float(G.grad_err(got, r64).max())
    print("fk vjp %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, err, own))
    assert got.shape == r64.shape and err <= 4.0 * own
    assert _same(VA.motion_fk_vjp(model, c["traj"][:1], c["chain"], g[:1])[0], got[0])


# ------------------------------------------------------------------------------------------------ 3. motion decoding, reversed
# ((D, Kb, T), rows, variant): every shape, rows 1, 4, 5 and 300 (the row tile is 4), every variant
# (300 rows of limits that bind go with the short shape: among the 210,000 points of 300 rows at T = 100 one always lies within
# float32's reach of a limit, where the two precisions may differ on whether it passes)
EVAL_CASES = [((1, 1, 1), 1, "plain"), ((1, 1, 1), 5, "limits"), ((3, 9, 2), 4, "scaled"), ((3, 9, 2), 300, "all"),
              ((7, 21, 100), 1, "anchor1"), ((7, 21, 100), 5, "all"), ((7, 21, 100), 4, "limits"), ((7, 21, 100), 300, "scaled"),
              ((7, 21, 100), 5, "plain"), ((16, 64, 257), 5, "all"), ((16, 64, 257), 4, "scaled"), ((16, 64, 257), 1, "limits")]


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: "%d-%d-%d r%d %s" % (c[0] + c[1:]))
def test_eval_vjp_against_the_definition(V, case):
    from vae_assoc_amd.motion import MotionBasis
    model = _model(V)
    shape, rows, variant = case
    D, Kb, T = shape
    c = MR.case(shape, rows, variant)
    g = np.random.default_rng([10, D, Kb, T, rows]).standard_normal((rows, T, D)).astype(np.float32)
    kw = MR.eval_kw(c)
    ok64, clear = G.eval_pass(c["params"], c["phi"], D, **kw)
    ok32, _ = G.eval_pass(c["params"], c["phi"], D, dt=np.float32, **kw)
    assert np.array_equal(ok64, ok32) and clear > 1e-5, "the fixture sits on a limit: pick another seed"
    if c["limits"] is not None and T > 1:
        assert not ok64.all() and ok64.any()                            # limits that bind, and not everywhere
    r64, r32 = G.eval_vjp64(c["params"], c["phi"], D, g, **kw), G.eval_vjp32(c["params"], c["phi"], D, g, **kw)
    # the kernel through the C ABI, on the case's own matrices
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)   # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                                                                     # noqa: E731
    t = {k: dev(c[k]) for k in ("params", "phi", "scale", "shift", "limits", "gain", "target")}
    gd, out = dev(g), torch.empty((rows, D * Kb), device=model.device)
    model._call("avae_motion_eval_vjp", p(t["params"]), rows, D, Kb, T, p(t["phi"]), p(t["scale"]), p(t["shift"]), p(t["limits"]),
                p(t["gain"]), p(t["target"]), c["nc"], p(gd), p(out))
    got = out.cpu().numpy()
    own, err = float(G.grad_err(r32, r64).max()), float(G.grad_err(got, r64).max())
    print("eval vjp %s rows %d %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, rows, variant, err, own))
    assert err <= 4.0 * own
    if variant == "plain" and shape == (7, 21, 100):                    # the Python surface, a basis without standardisation
        basis = MotionBasis(n_basis=Kb - 1, n_dof=D, n_points=T)
        assert _same(VA.motion_eval_vjp(model, c["params"], basis, g), got)


def test_eval_vjp_keeps_a_nan_parameter_in_its_joint(V):
    model = _model(V)
    shape, rows = (7, 21, 100), 5
    D, Kb, T = shape
    c = MR.case(shape, rows, "all")
    g = np.random.default_rng(12).standard_normal((rows, T, D)).astype(np.float32)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)   # noqa: E731

    def run(params):
        t = {k: dev(c[k]) for k in ("phi", "scale", "shift", "limits", "gain", "target")}
        pd, gd, out = dev(params), dev(g), torch.empty((rows, D * Kb), device=model.device)
        model._call("avae_motion_eval_vjp", pd.data_ptr(), rows, D, Kb, T, t["phi"].data_ptr(), t["scale"].data_ptr(),
                    t["shift"].data_ptr(), t["limits"].data_ptr(), t["gain"].data_ptr(), t["target"].data_ptr(), c["nc"],
                    gd.data_ptr(), out.data_ptr())
        return out.cpu().numpy().reshape(rows, D, Kb)
    clean = run(c["params"])
    bad = c["params"].copy()
    bad[2, 3 * Kb + 4] = np.nan
    out = run(bad)
    assert np.isfinite(out).all() and not out[2, 3].any()               # every point of (row 2, joint 3) fails lo <= q <= hi
    keep = np.ones((rows, D), bool)
    keep[2, 3] = False
    assert _same(out[keep], clean[keep])


# ------------------------------------------------------------------------------------------------ 4. Adam, a row a problem
@pytest.mark.parametrize("shape", ((1, 1), (3, 20), (2, 147), (65, 1000)), ids=lambda s: "%d-%d" % s)
def test_rows_adam_against_the_definition(V, shape):
    model = _model(V)
    P, n = shape
    rng = np.random.default_rng([13, P, n])
    x = rng.standard_normal((P, n)).astype(np.float32)
    st = None
    st32 = G.fresh_adam(x, np.float32)
    own = got = 0.0
    for step, max_norm in enumerate((None, 0.5, None, 2.0)):
        g = (rng.standard_normal((P, n)) * (3.0 if step == 1 else 1.0)).astype(np.float32)
        if P > 1 and step == 2:
            g[1, n // 2] = np.inf                                       # a row that must stay as it is
        cost = rng.random(P).astype(np.float32) + (0.0 if step < 3 else 10.0)           # the last step improves nothing
        kw = dict(lr=0.05, max_norm=max_norm, cost=cost)
        x64, s64, f64 = G.rows_adam64(x, g, {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in st32.items()}, **kw)
        x32, s32, f32 = G.rows_adam32(x, g, st32, **kw)
        out = VA.rows_adam(model, x, g, state=st, **kw)
        xg, st = out["x"], out["state"]
        assert np.array_equal(out["status"], f64) and np.array_equal(f32, f64)
        for name, a32, a64, ag in (("x", x32, x64, xg), ("m", s32["m"], s64["m"], st["m"].cpu().numpy()),
                                   ("v", s32["v"], s64["v"], st["v"].cpu().numpy())):
            own, got = max(own, float(G.grad_err(a32, a64).max())), max(got, float(G.grad_err(ag, a64).max()))
        assert np.array_equal(st["t"].cpu().numpy(), s64["t"])
        assert _same(st["best_x"], s32["best_x"]) and _same(st["best_cost"], s32["best_cost"])      # copies: exact
        if P > 1 and step == 2:
            assert out["status"][1] == 2 and _same(xg[1], x[1])
        # the next step starts from the restatement's state on both sides, so every step is compared on equal inputs
        x, st32 = x32, s32
        st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(model.device) for k, v in s32.items()}
    print("rows_adam %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, got, own))
    assert got <= 4.0 * own


# ------------------------------------------------------------------------------------------------ 5. the model level
def _letters():
    """four seeded letters: parameters, the pictures they write, and a perturbed start (render_grad_reference.DESCENT)"""
    basis, chain, canvas = G.writer()
    true, start = G.descent_fixture()
    return basis, chain, canvas, true, start


def test_writing_cost_grad_is_draw_motions_bits_and_the_definitions_gradient(V):
    model = _model(V)
    basis, chain, canvas, true, start = _letters()
    target = model.draw_motion(true, basis, chain, canvas)["image"]
    out = VA.writing_cost_grad(model, start, basis, chain, canvas, target)
    traj = model.motion_eval(start, basis)["trajectory"]
    height = (model.motion_fk(traj, chain).astype(np.float64) @ canvas.plane[2]).mean(1).astype(np.float32)
    drawn = model.draw_motion(start, basis, chain, canvas, target=target, height=height)
    dev = VA.writing_cost_grad(model, torch.from_numpy(start).to(model.device), basis, chain, canvas,
                                  torch.from_numpy(target).to(model.device))
    for k in ("img_l2", "image"):                                       # (these two do not depend on the height)
        assert _same(out[k], drawn[k]) and _same(dev[k], drawn[k]), k
    assert _same(dev["grad"], out["grad"])
    given = VA.writing_cost_grad(model, start, basis, chain, canvas, target, height=height)
    for k in ("img_l2", "height_l2", "image"):
        assert _same(given[k], drawn[k]), k
    assert _same(given["cost"], (np.float32(0.3) * (drawn["img_l2"] + np.float32(10.0) * drawn["height_l2"])).astype(np.float32))
    ref = G.chain64(start, basis, chain, canvas, target, height)
    own = float(G.grad_err(G.chain32(start, basis, chain, canvas, target, height), ref["grad"]).max())
    err = float(G.grad_err(given["grad"], ref["grad"]).max())
    print("writing_cost_grad: kernel chain %.3e, restated chain %.3e (bound 4x)" % (err, own))
    assert err <= 4.0 * own
    assert np.abs(given["cost"] - ref["cost"]).max() <= 1e-4 * np.abs(ref["cost"]).max()


def test_descend_motion_halves_the_cost_and_continues_bit_for_bit(V):
    """four seeded letters, the targets drawings of known parameters, the start perturbed: lr and n_iters are the ones
    test_render_grad_cpu.py shows the float64 loop to more than halve every row's cost with"""
    model = _model(V)
    basis, chain, canvas, true, start = _letters()
    target = model.draw_motion(true, basis, chain, canvas)["image"]
    kw = dict(init=start, lr=G.DESCENT["lr"], anchor_start=False)
    full = VA.descend_motion(model, target, basis, chain, canvas, n_iters=G.DESCENT["n_iters"], **kw)
    h = full["history"]
    print("descend_motion: cost %s -> %s (best %s)" % (np.round(h[0], 4), np.round(h[-1], 4), np.round(full["best_cost"], 4)))
    assert h.shape == (G.DESCENT["n_iters"] + 1, 4) and np.isfinite(h).all() and not full["status"].any()
    assert (h[-1] < 0.5 * h[0]).all() and (full["best_cost"] <= h.min(0)).all()
    first = VA.descend_motion(model, target, basis, chain, canvas, n_iters=8, **kw)
    rest = VA.descend_motion(model, target, basis, chain, canvas, n_iters=G.DESCENT["n_iters"] - 8, state=first["state"], lr=G.DESCENT["lr"])
    for k in ("params", "best_params", "best_cost", "cost", "image", "best_image", "status"):
        assert _same(rest[k], full[k]), k
    assert _same(np.concatenate([first["history"][:8], rest["history"]]), h)
    for k in ("m", "v", "t", "best_x", "best_cost"):
        assert _same(rest["state"]["adam"][k], full["state"]["adam"][k]), k
    # the anchored start: every trajectory starts where the first one did
    anchored = VA.descend_motion(model, target, basis, chain, canvas, init=start, n_iters=3, lr=G.DESCENT["lr"])
    t0 = model.motion_eval(start, basis)["trajectory"][:, 0]
    t1 = model.motion_eval(anchored["params"], basis, anchor=dict(phases=[0.0], target=t0[:, :, None]))["trajectory"][:, 0]
    assert np.abs(t1 - t0).max() < 1e-5 and np.isfinite(anchored["history"]).all()
