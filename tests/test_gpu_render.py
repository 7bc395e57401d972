"""Pen-path kinematics and stroke rendering (avae_motion_fk / avae_stroke_render, motion_fk / render_strokes / draw_motion /
writing_cost / cycle_error) on a real MI355X (include/avae.h) against tests/render_reference.py.

1. forward kinematics and 2. the renderer against the float64 definition, within 4x the float32 restatement's own worst error over
the same inputs (the rule of test_gpu_motion.py; |err| / (|ref| + 1) per quantity, the image in absolute terms); 3. bit
reproducibility and independence; 4. non-finite paths; 5. edges and errors of the C ABI; 6. the model level.

The shapes, path families and planes are render_reference's: FK (rows, T, D) = (1, 1, 1), (3, 2, 3), (5, 100, 7) on the fixture chain
inside its joint limits and (2, 257, 16) on a random chain; the renderer at (T, H, ss) = (1, 28, 4), (2, 28, 1), (100, 28, 4),
(100, 28, 8), (1024, 64, 2), (7, 5, 4), calls of 1 to 5 rows.  The ``*_classes_*`` tests sweep the classes of shape the kernels'
control flow distinguishes (render_reference.FK_CLASS_SHAPES, RENDER_CLASS_SHAPES, RENDER_CLASS_PARAMS; each test's docstring
names them).  The measured pairs are in README.md and DESIGN.md section 24."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_reference as R
from conftest import make_arch, synth_batch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
RW, MG = float(np.float32(R.HALF_WIDTH)), float(np.float32(R.MARGIN))


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


def _dev(model, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(model):
    return C.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)


def _err(model):
    return model._L.avae_last_error(model._h).decode()


def _fk(model, traj, frames, axes):
    rows, T, D = traj.shape
    out = torch.full((rows, T, 3), -7.0, device=model.device)
    ts = [_dev(model, x) for x in (traj, frames, axes)]
    rc = model._L.avae_motion_fk(model._h, _p(ts[0]), rows, T, D, _p(ts[1]), _p(ts[2]), _p(out), _stream(model))
    assert rc == 0, _err(model)
    return out.cpu().numpy()


OUTPUTS = ("image", "window", "img_l2", "height_l2")


def _render(model, path, plane, H, ss, target=None, height=None, want=OUTPUTS, r=RW, margin=MG, rc_want=0, T=None, rows=None):
    """avae_stroke_render -> dict of the NumPy outputs asked for (``want``), each prefilled with -7"""
    N = path.shape[0] if rows is None else rows
    T = path.shape[1] if T is None else T
    shapes = dict(image=(max(N, 1), H * H), window=(max(N, 1), 3), img_l2=(max(N, 1),), height_l2=(max(N, 1),))
    out = {k: torch.full(shapes[k], -7.0, device=model.device) for k in want}
    ts = [_dev(model, x) for x in (path, plane, target, height)]
    rc = model._L.avae_stroke_render(model._h, _p(ts[0]), N, T, _p(ts[1]), r, margin, H, ss, _p(ts[2]), _p(ts[3]),
                                     _p(out.get("image")), _p(out.get("window")), _p(out.get("img_l2")), _p(out.get("height_l2")),
                                     _stream(model))
    torch.cuda.synchronize()
    assert (rc == 0) == (rc_want == 0), (rc, _err(model))
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 1. forward kinematics
@pytest.mark.parametrize("shape", R.FK_SHAPES)
def test_fk_against_the_definition(V, shape):
    model = _model(V)
    c = R.fk_case(shape)
    r64, r32 = R.fk64(c["traj"], c["frames"], c["axes"]), R.fk32(c["traj"], c["frames"], c["axes"])
    got = _fk(model, c["traj"], c["frames"], c["axes"])
    own, err = R.rel_err(r32, r64), R.rel_err(got, r64)
    print("fk %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, err, own))
    assert got.shape == r64.shape and err <= 4.0 * own
    # the Python call, a row alone, repetition
    chain = c["chain"]
    again = model.motion_fk(c["traj"], chain)
    assert isinstance(again, np.ndarray) and _same(again, got)
    assert _same(model.motion_fk(torch.from_numpy(c["traj"][-1:]).to(model.device), chain), got[-1:])


@pytest.mark.parametrize("shape,wild", [(s, False) for s in R.FK_CLASS_SHAPES] + [(R.FK_WILD, True)])
def test_fk_classes_against_the_definition(V, shape, wild):
    """The tile and row-length classes of k_motion_fk (render_reference.FK_CLASS_SHAPES): (1, 256, 2) one tile of exactly 256 points,
    LDS rows of D | 1 = 3; (4, 64, 4) 256 points over four rows, rows of 5; (2, 256, 8) exactly two tiles, rows of 9; (3, 171, 15)
    513 points: a third tile of one point, the odd D = 15.  (5, 100, 7) with angles uniform in +-4 pi: sincosf past +-pi, which
    the limits of the other cases never reach.  The 4x rule, the bits of a repeat and of the last row alone."""
    model = _model(V)
    c = R.fk_case(shape, wild=wild)
    assert not wild or np.abs(c["traj"]).max() > 3.0 * np.pi
    r64, r32 = R.fk64(c["traj"], c["frames"], c["axes"]), R.fk32(c["traj"], c["frames"], c["axes"])
    got = _fk(model, c["traj"], c["frames"], c["axes"])
    own, err = R.rel_err(r32, r64), R.rel_err(got, r64)
    print("fk %s%s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, " wild" if wild else "", err, own))
    assert got.shape == r64.shape and err <= 4.0 * own
    assert _same(_fk(model, c["traj"], c["frames"], c["axes"]), got)
    assert _same(_fk(model, c["traj"][-1:], c["frames"], c["axes"]), got[-1:])
    assert _same(model.motion_fk(c["traj"], c["chain"]), got)


def test_fk_seed_pose_lands_on_the_block_center(V):
    from vae_assoc_amd.kinematics import KinematicChain
    model, fx = _model(V), R.fixture()
    chain = KinematicChain(fx["joints"])
    tip = model.motion_fk(np.array(fx["seed_pos"], dtype=np.float32).reshape(1, 1, 7), chain)
    assert tip.shape == (1, 1, 3) and np.abs(tip[0, 0] - np.array(fx["block_center"])).max() < 1e-3
    assert model.motion_fk(np.zeros((0, 4, 7), np.float32), chain).shape == (0, 4, 3)


# ------------------------------------------------------------------------------------------------ 2. the renderer
@pytest.mark.parametrize("shape", R.RENDER_SHAPES)
def test_render_against_the_definition(V, shape):
    model = _model(V)
    T, H, ss = shape
    own, got = dict.fromkeys(OUTPUTS, 0.0), dict.fromkeys(OUTPUTS, 0.0)
    for name, plane, path, height, target, r64, r32 in R.render_refs(shape):
        g = _render(model, path, plane, H, ss, target, height)
        e_own, e_got = R.render_errors(r32, r64), R.render_errors(g, r64)
        for k in OUTPUTS:
            own[k], got[k] = max(own[k], e_own[k]), max(got[k], e_got[k])
    for k in OUTPUTS:
        print("render %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, k, got[k], own[k]))
    for k in OUTPUTS:
        assert got[k] <= 4.0 * own[k], k


CLASS_CASES = [(s, p) for s in R.RENDER_CLASS_SHAPES for p in R.class_params(s)]
CLASS_IDS = ["%d-%d-%d r%g m%g" % (s + p) for s, p in CLASS_CASES]


@pytest.mark.parametrize("shape,params", CLASS_CASES, ids=CLASS_IDS)
def test_render_classes_against_the_definition(V, shape, params):
    """The classes k_stroke_render's control flow distinguishes (render_reference.RENDER_CLASS_SHAPES), by the 64-pixel chunks of
    step 4, the passes of step 5 and T against the 256 threads: (3, 1, 8) one pixel; (256, 8, 2) exactly one full chunk;
    (257, 16, 1) 4 chunks, thread 0 owns two points; (258, 20, 4) 7 chunks, 257 segments; (513, 23, 2) 9 chunks; (2, 64, 1)
    64 chunks, ss = 1, 256 pixels a pass; (100, 64, 8) H ss = 512, 32 pixels a pass.  Each with (half_width, margin) = the
    writer's, a hairline without margin and a broad pen in a wide margin (the culling threshold depends on r / delta and the
    margin), every family and the two that leave the culling to the distance test (``diagonal``, ``frame``), under both planes.

    a. the 4x rule on every output; b. no pixel the restatement (which does not cull) inks is exactly +0 in the kernel's image;
    c. on the definition alone: a row with fewer than half its pixels inked (at H = 1 the one pixel is inked: nothing can be
    culled and the condition is that it is), and where H H ss > 256 a row whose inked pixels x ss exceed 256, so step 5 takes a
    second pass.  At margin 3 the ink box spans a quarter of the window, at most (H / 4 + 2)^2 pixels; at H <= 23 that is one pass
    whatever the path and at (2, 64, 1) a two-point path cannot fill it: the second condition is asserted for margins below 1."""
    model = _model(V)
    T, H, ss = shape
    r, mg = float(np.float32(params[0])), float(np.float32(params[1]))
    refs = R.class_refs(shape, params)
    share, items = R.class_coverage(shape, refs)
    assert share < 0.5 if H > 1 else share == 1.0, share
    if H * H * ss > R.THREADS and mg < 1.0:
        assert items > R.THREADS, items
    own, got = dict.fromkeys(OUTPUTS, 0.0), dict.fromkeys(OUTPUTS, 0.0)
    for name, plane, path, height, target, r64, r32 in refs:
        g = _render(model, path, plane, H, ss, target, height, r=r, margin=mg)
        e_own, e_got = R.render_errors(r32, r64), R.render_errors(g, r64)
        for k in OUTPUTS:
            own[k], got[k] = max(own[k], e_own[k]), max(got[k], e_got[k])
        lost = (r32["image"] != 0.0) & (_bits(g["image"]) == 0)
        assert not lost.any(), (name, np.argwhere(lost)[:4])
    for k in OUTPUTS:
        print("render %s r=%g margin=%g %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, r, mg, k, got[k], own[k]))
    for k in OUTPUTS:
        assert got[k] <= 4.0 * own[k], k


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("params", R.RENDER_CLASS_PARAMS[:2], ids=["writer", "margin0"])
@pytest.mark.parametrize("shape", [(257, 16, 1), R.RENDER_BIG])
def test_class_rows_outputs_and_streams_give_the_same_bits(V, shape, params):
    """A row alone, an output alone and a second stream at (257, 16, 1) (4 chunks, two points for thread 0) and (100, 64, 8)
    (32 pixels a pass, lists of thousands of items), with the writer's margin and with none"""
    model = _model(V)
    T, H, ss = shape
    kw = dict(r=float(np.float32(params[0])), margin=float(np.float32(params[1])))
    name, plane, path, height = R.class_batches(shape)[0]
    target = R.class_target(shape, name, path.shape[0])
    full = _render(model, path, plane, H, ss, target, height, **kw)
    for i in range(path.shape[0]):
        one = _render(model, path[i:i + 1], plane, H, ss, target[i:i + 1], height[i:i + 1], **kw)
        assert all(_same(one[k], full[k][i:i + 1]) for k in OUTPUTS), (shape, i)
    for k in OUTPUTS:
        assert _same(_render(model, path, plane, H, ss, target, height, want=(k,), **kw)[k], full[k]), (shape, k)
    side = torch.cuda.Stream(device=model.device)
    with torch.cuda.stream(side):
        other = _render(model, path, plane, H, ss, target, height, **kw)
    assert all(_same(other[k], full[k]) for k in OUTPUTS)
    assert (full["image"] > 0).any(1).all() and not (full["image"] == -7.0).any()


def test_rows_outputs_streams_and_repetition_give_the_same_bits(V):
    model = _model(V)
    for shape in ((100, 28, 4), (7, 5, 4), (1024, 64, 2)):
        T, H, ss = shape
        name, plane, path, height, target, _, _ = R.render_refs(shape)[0]                     # five rows, one of every family
        full = _render(model, path, plane, H, ss, target, height)
        for i in range(path.shape[0]):                                                         # a row alone
            one = _render(model, path[i:i + 1], plane, H, ss, target[i:i + 1], height[i:i + 1])
            assert all(_same(one[k], full[k][i:i + 1]) for k in OUTPUTS), (shape, i)
        for k in OUTPUTS:                                                                      # an output alone
            assert _same(_render(model, path, plane, H, ss, target, height, want=(k,))[k], full[k]), (shape, k)
        assert all(_same(_render(model, path, plane, H, ss, target, height)[k], full[k]) for k in OUTPUTS)
        side = torch.cuda.Stream(device=model.device)
        with torch.cuda.stream(side):
            other = _render(model, path, plane, H, ss, target, height)
        assert all(_same(other[k], full[k]) for k in OUTPUTS)
        # a target equal to the image
        assert not _render(model, path, plane, H, ss, full["image"], None, want=("img_l2",))["img_l2"].any()


def test_nonfinite_rows_are_nan_and_touch_nothing_else(V):
    model = _model(V)
    T, H, ss = 100, 28, 4
    name, plane, path, height, target, _, _ = R.render_refs((T, H, ss))[0]
    clean = _render(model, path, plane, H, ss, target, height)
    bad = path.copy()
    bad[1, 37, 2] = np.nan
    bad[3, 99, 0] = -np.inf
    g = _render(model, bad, plane, H, ss, target, height)
    for k in OUTPUTS:
        assert np.isnan(g[k][[1, 3]]).all(), k
        assert _same(g[k][[0, 2, 4]], clean[k][[0, 2, 4]]), k
    only = _render(model, bad, plane, H, ss, want=("window",))
    assert np.isnan(only["window"][[1, 3]]).all() and _same(only["window"][[0, 2, 4]], clean["window"][[0, 2, 4]])


# ------------------------------------------------------------------------------------------------ 5. edges and errors
def test_c_abi_errors_name_the_argument_and_launch_nothing(V):
    model = _model(V)
    name, plane, path, height, target, _, _ = R.render_refs((7, 5, 4))[0]
    ok = dict(path=path, plane=plane, H=5, ss=4, target=target, height=height)
    for kw, needle in ((dict(rows=-1), "rows"), (dict(T=0), "T"), (dict(T=1025), "T"), (dict(H=0), "H"), (dict(H=65), "H"),
                       (dict(ss=3), "ss"), (dict(ss=0), "ss"), (dict(ss=16), "ss"), (dict(r=0.0), "half_width"),
                       (dict(r=-1.0), "half_width"), (dict(r=float("nan")), "half_width"), (dict(margin=-0.5), "margin"),
                       (dict(margin=float("nan")), "margin"), (dict(path=None, rows=5, T=7), "path_dev"), (dict(plane=None), "plane_dev"),
                       (dict(want=()), "output"), (dict(target=None), "target_dev"), (dict(height=None), "height_dev")):
        g = _render(model, **dict(ok, rc_want=1, **kw))
        assert needle in _err(model), (kw, _err(model))
        assert all((v == -7.0).all() for v in g.values()), kw
    # without the output that needs it, a missing target or height is fine; rows == 0 is a no-op
    g = _render(model, path, plane, 5, 4, want=("image", "window"))
    assert (g["image"] != -7.0).all() and (g["window"] != -7.0).all()
    g = _render(model, path, plane, 5, 4, target, height, rows=0)
    assert all((v == -7.0).all() for v in g.values())
    # forward kinematics
    c = R.fk_case((3, 2, 3))
    ts = [_dev(model, x) for x in (c["traj"], c["frames"], c["axes"])]
    out = torch.full((3, 2, 3), -7.0, device=model.device)
    for args, needle in (((_p(ts[0]), -1, 2, 3, _p(ts[1]), _p(ts[2]), _p(out)), "rows"), ((_p(ts[0]), 3, 0, 3, _p(ts[1]), _p(ts[2]), _p(out)), "T"),
                         ((_p(ts[0]), 3, 1025, 3, _p(ts[1]), _p(ts[2]), _p(out)), "T"), ((_p(ts[0]), 3, 2, 0, _p(ts[1]), _p(ts[2]), _p(out)), "D"),
                         ((_p(ts[0]), 3, 2, 17, _p(ts[1]), _p(ts[2]), _p(out)), "D"), ((None, 3, 2, 3, _p(ts[1]), _p(ts[2]), _p(out)), "traj_dev"),
                         ((_p(ts[0]), 3, 2, 3, None, _p(ts[2]), _p(out)), "frames_dev"), ((_p(ts[0]), 3, 2, 3, _p(ts[1]), None, _p(out)), "axes_dev"),
                         ((_p(ts[0]), 3, 2, 3, _p(ts[1]), _p(ts[2]), None), "path_dev")):
        assert model._L.avae_motion_fk(model._h, *args, _stream(model)) != 0
        assert needle in _err(model), (needle, _err(model))
    assert model._L.avae_motion_fk(model._h, _p(ts[0]), 0, 2, 3, _p(ts[1]), _p(ts[2]), _p(out), _stream(model)) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ------------------------------------------------------------------------------------------------ 6. the model level
def _writer(seed=0, rows=6):
    """a basis whose parameters stay inside the fixture's joint limits around the writer's seed pose, the chain, the canvas, and
    ``rows`` standardised parameter rows"""
    from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    fx = R.fixture()
    chain = KinematicChain(fx["joints"])
    mean = np.zeros((7, 21))
    mean[:, -1] = fx["seed_pos"]
    # a spread of 0.012 rad per basis weight: strokes of a letter's size, 3 to 6 plane units across
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(147, 0.012))
    params = np.random.default_rng(seed).standard_normal((rows, 147)).astype(np.float32)
    return basis, chain, StrokeCanvas(), params


def test_draw_motion_is_bitwise_the_three_calls(V):
    model = _model(V)
    basis, chain, canvas, params = _writer()
    target = np.random.default_rng(1).random((6, 784)).astype(np.float32)
    d = model.draw_motion(params, basis, chain, canvas, target=target, height=0.25)
    traj = model.motion_eval(params, basis)["trajectory"]
    path = model.motion_fk(traj, chain)
    r = model.render_strokes(path, canvas, target=target, height=np.full(6, 0.25, np.float32))
    assert _same(d["trajectory"], traj) and _same(d["path"], path) and all(_same(d[k], r[k]) for k in OUTPUTS)
    assert d["image"].shape == (6, 784) and np.isfinite(d["image"]).all() and (d["image"].sum(1) > 1.0).all()
    # the drawing is the definition's drawing of that path
    ref = R.render64(path, canvas.plane.astype(np.float32), RW, MG, 28, 4)
    assert np.abs(d["image"] - ref["image"]).max() < 1e-4 and R.rel_err(d["window"], ref["window"]) < 1e-5
    bare = model.draw_motion(torch.from_numpy(params).to(model.device), basis, chain, canvas)
    assert torch.is_tensor(bare["image"]) and bare["img_l2"] is None and bare["height_l2"] is None and _same(bare["image"], d["image"])


def test_writing_cost_is_its_terms(V):
    model = _model(V)
    basis, chain, canvas, params = _writer(seed=2)
    goal = model.draw_motion(params[:1], basis, chain, canvas)["image"][0]                    # one picture for every candidate
    w = (0.3, 10.0, 0.7)
    c = model.writing_cost(params, basis, chain, canvas, goal)
    d = model.draw_motion(params, basis, chain, canvas)
    plane = canvas.plane.astype(np.float32)
    height = (torch.from_numpy(d["path"]).to(model.device) @ torch.from_numpy(plane[2]).to(model.device)).mean(1).cpu().numpy()
    r = model.render_strokes(d["path"], canvas, target=goal, height=height)
    assert _same(c["image"], d["image"]) and _same(c["path"], d["path"]) and _same(c["trajectory"], d["trajectory"])
    assert _same(c["img_l2"], r["img_l2"]) and np.abs(c["height_l2"] - r["height_l2"]).max() <= 1e-6 * (1.0 + r["height_l2"].max())
    z, zt = model.transform(d["image"], 0), model.transform(goal[None], 0)
    lat = np.linalg.norm(z.astype(np.float64) - zt.astype(np.float64), axis=1)
    assert np.abs(c["latent_l2"] - lat).max() <= 1e-5 * (1.0 + lat.max())
    want = w[0] * (r["img_l2"].astype(np.float64) + w[1] * r["height_l2"]) + w[2] * lat
    assert np.abs(c["cost"] - want).max() <= 1e-5 * (1.0 + np.abs(want).max())
    assert c["img_l2"][0] == 0.0 and c["latent_l2"][0] < 1e-5 and (c["img_l2"][1:] > 0.1).all()   # the first candidate drew the goal
    assert (c["height_l2"] >= 0).all() and c["cost"].shape == (6,)
    # an explicit latent target and height, other weights
    c2 = model.writing_cost(params, basis, chain, canvas, goal, target_latent=zt[0] + 1.0, height=0.2, weights=(1.0, 0.0, 2.0))
    lat2 = np.linalg.norm(z.astype(np.float64) - (zt + 1.0), axis=1)
    r2 = model.render_strokes(d["path"], canvas, target=goal, height=0.2)
    assert _same(c2["height_l2"], r2["height_l2"]) and np.abs(c2["latent_l2"] - lat2).max() <= 1e-5 * (1.0 + lat2.max())
    assert np.abs(c2["cost"] - (r["img_l2"] + 2.0 * lat2)).max() <= 1e-5 * (1.0 + np.abs(lat2).max() * 2)


def test_cycle_error_on_a_small_model(V):
    model = _model(V)
    basis, chain, canvas, params = _writer(seed=3, rows=B)
    X = synth_batch(np.random.default_rng(4), B, (784, 147), (True, False))
    X[1] = params
    out = model.cycle_error(X, basis, chain, canvas)
    for part in ("predicted", "own"):
        assert out[part]["img_l2"].shape == (B,) and out[part]["latent_l2"].shape == (B,) and out[part]["image"].shape == (B, 784)
        assert all(np.isfinite(v).all() for v in out[part].values()) and (out[part]["img_l2"] > 0).all()
    d = model.draw_motion(X[1], basis, chain, canvas, target=X[0])
    assert _same(out["own"]["image"], d["image"]) and _same(out["own"]["img_l2"], d["img_l2"])
    lat = np.linalg.norm(model.transform(d["image"], 0).astype(np.float64) - model.transform(X[0], 0).astype(np.float64), axis=1)
    assert np.abs(out["own"]["latent_l2"] - lat).max() <= 1e-5 * (1.0 + lat.max())
    pred = model.predict_motion([X[0], None], basis)["trajectory"]
    p = model.render_strokes(model.motion_fk(pred, chain), canvas, target=X[0])
    assert _same(out["predicted"]["image"], p["image"]) and _same(out["predicted"]["img_l2"], p["img_l2"])
    assert model.cycle_error([X[0], None], basis, chain, canvas)["own"] is None
    with pytest.raises(ValueError):
        model.cycle_error(X, basis, chain, canvas, source=1)
