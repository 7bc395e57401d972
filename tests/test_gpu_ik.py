"""Pose, Jacobian and inverse kinematics (avae_motion_pose / avae_motion_ik, motion_pose / motion_ik / strokes_to_motion /
refine_pen_path) on a real MI355X (include/avae.h) against tests/ik_reference.py.

1. the pose kernel and 2. the solver step for step (``tol = 0``: no early-stop decision can differ) against the float64 definition,
within 4x the float32 restatement's own worst error over the same inputs (the rule of test_gpu_motion.py; |err| / (|ref| + 1) per
quantity); 3. the contract at the default options; 4. bit reproducibility and independence; 5. non-finite and unreachable
targets, edges and errors of the C ABI; 6. the composed calls; 7. every joint count class from the inside (D < DC) and every branch
of the solver: the shrink, status 2 by a zero pivot and by a step that is not finite, huge targets, zero steps, a seed on its
target, a pinned joint and a seed outside the box.  The shapes and variants are tests/ik_cases.py's; the measured pairs are in
README.md and DESIGN.md section 26."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_cases as IC
import ik_reference as K
import render_reference as R
from conftest import make_arch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
OUTPUTS = ("trajectory", "residual", "rot_residual", "iterations", "status")


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V):
    """one small fp32 relu model (the nets of test_gpu_render.py), shared by every test here"""
    if "m" not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS["m"] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3)
    return _MODELS["m"]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


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


def _pose(model, traj, frames, axes, want=("position", "rotation", "jacobian")):
    """avae_motion_pose -> dict of the NumPy outputs asked for, each prefilled with -7"""
    rows, T, D = traj.shape
    tails = dict(position=(3,), rotation=(3, 3), jacobian=(6, D))
    out = {k: torch.full((rows, T) + tails[k], -7.0, device=model.device) for k in want}
    ts = [_dev(model, x) for x in (traj, frames, axes)]
    rc = model._L.avae_motion_pose(model._h, _p(ts[0]), rows, T, D, _p(ts[1]), _p(ts[2]), _p(out.get("position")),
                                   _p(out.get("rotation")), _p(out.get("jacobian")), _stream(model))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ik(model, c, want=OUTPUTS, rows=None, **opt):
    """avae_motion_ik on a case of ik_cases (``rows``: a slice of its rows) -> dict of the NumPy outputs asked for, prefilled with
    -7; ``rot_residual`` comes back None where the case has no goal"""
    sl = slice(None) if rows is None else rows
    path, seed, orient = c["path"][sl], c["seed"][sl], c["orient"]
    if orient is not None and orient.ndim == 3:
        orient = orient[sl]
    N, T, D = path.shape[0], path.shape[1], seed.shape[1]
    o = dict(n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5)
    o.update(opt)
    shapes = dict(trajectory=(N, T, D), residual=(N, T), rot_residual=(N, T), iterations=(N, T), status=(N, T))
    out = {k: torch.full(shapes[k], -7, device=model.device, dtype=torch.int32 if k in ("iterations", "status") else torch.float32)
           for k in want if not (k == "rot_residual" and orient is None)}
    ts = [_dev(model, x) for x in (path, c["frames"], c["axes"], seed, orient, c["limits"])]
    rc = model._L.avae_motion_ik(model._h, _p(ts[0]), N, T, D, _p(ts[1]), _p(ts[2]), _p(ts[3]), _p(ts[4]),
                                 0 if orient is None else (1 if orient.ndim == 2 else N), _p(ts[5]), o["n_iters"], o["tol"],
                                 o["rot_tol"], o["damping"], o["max_step"], _p(out.get("trajectory")), _p(out.get("residual")),
                                 _p(out.get("rot_residual")), _p(out.get("iterations")), _p(out.get("status")), _stream(model))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if "rot_residual" in want and orient is None:
        res["rot_residual"] = None
    return res


# ------------------------------------------------------------------------------------------------ 1. pose and Jacobian
@pytest.mark.parametrize("shape", IC.POSE_SHAPES + IC.POSE_TILE_SHAPES)
def test_pose_against_the_definition(V, shape):
    """(rows, T, D) = (1, 1, 1), (3, 2, 3), (5, 100, 7) on the fixture arm and (2, 257, 16) on a random chain (the classes D <= 4,
    <= 8, <= 16 of the kernel), then 255, 256, 257 and 600 points: the edges of the 256-point tiles."""
    model = _model(V)
    c, r64, r32 = IC.pose_refs(shape)
    got = _pose(model, c["traj"], c["frames"], c["axes"])
    for k in ("position", "rotation", "jacobian"):
        own, err = IC.rel_err(r32[k], r64[k]), IC.rel_err(got[k], r64[k])
        print("pose %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, k, err, own))
        assert got[k].shape == r64[k].shape and err <= 4.0 * own, k
    # whichever outputs are asked for, a row alone, repetition, the Python call; the position against avae_motion_fk
    for want in (("position",), ("rotation",), ("jacobian",), ("position", "jacobian")):
        part = _pose(model, c["traj"], c["frames"], c["axes"], want)
        assert all(_same(part[k], got[k]) for k in want)
    last = _pose(model, c["traj"][-1:], c["frames"], c["axes"])
    assert all(_same(last[k], got[k][-1:]) for k in got)
    py = model.motion_pose(c["traj"], c["chain"], jacobian=True)
    assert all(isinstance(py[k], np.ndarray) and _same(py[k], got[k]) for k in got)
    assert model.motion_pose(torch.from_numpy(c["traj"]).to(model.device), c["chain"])["jacobian"] is None
    assert np.abs(model.motion_fk(c["traj"], c["chain"]) - got["position"]).max() < 1e-5


# ------------------------------------------------------------------------------------------------ 2. the solver, step for step
@pytest.mark.parametrize("variant", IC.VARIANTS, ids=["-".join(v) for v in IC.VARIANTS])
@pytest.mark.parametrize("shape", IC.IK_SHAPES)
def test_ik_steps_against_the_definition(V, shape, variant):
    """``tol = 0`` never stops, so 1 and 4 steps are taken at every point whatever the arithmetic: angles and residuals against the
    definition.  (1, 1, 1), (4, 5, 4): the class D <= 4 and its edge; (5, 100, 7), (65, 3, 7), (4, 5, 8): D <= 8 and its edge;
    (3, 2, 3), (300, 2, 3); (2, 257, 16): D <= 16 at its edge.  65 rows cross a wave (= a workgroup), 300 make five.  The damping
    is the default without a goal and 0.1 under one (ik_cases.STEP_DAMPING says why)."""
    model = _model(V)
    c = IC.case(shape, *variant)
    for n in (1, 4):
        opt = dict(n_iters=n, tol=0.0, damping=IC.STEP_DAMPING[variant[0]])
        r64, r32 = IC.solve(c, np.float64, **opt), IC.solve(c, np.float32, **opt)
        got = _ik(model, c, **opt)
        assert (got["status"] == 1).all() and (got["iterations"] == n).all() and (r64["status"] == 1).all()
        for k in ("trajectory", "residual", "rot_residual"):
            if r64[k] is None:
                assert got[k] is None
                continue
            own, err = IC.rel_err(r32[k], r64[k]), IC.rel_err(got[k], r64[k])
            print("ik %s %s n_iters=%d %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, variant, n, k, err, own))
            assert got[k].shape == r64[k].shape and np.isfinite(got[k]).all() and err <= 4.0 * own, (k, n)
        if variant[1] == "binding" and n == 4:
            lo, hi = c["limits"][0]
            assert ((got["trajectory"][..., 0] == lo) | (got["trajectory"][..., 0] == hi)).any(), "the box does not bind"
            assert (got["trajectory"][..., 0] >= lo).all() and (got["trajectory"][..., 0] <= hi).all()


# ------------------------------------------------------------------------------------------------ 3. the contract at the defaults
def _contract_cases():
    out = [(s, "none", lim) for s in IC.IK_SHAPES for lim in ("chain", "off")]
    out += [(s, g, "chain") for s in IC.IK_SHAPES if s[1] == 1 for g in ("one", "rows")]
    return out + [("letters", "one", "chain")]


def _residual64(c, traj):
    p = K.walk64(traj.reshape(-1, traj.shape[-1]), c["frames"], c["axes"])[0].reshape(traj.shape[:-1] + (3,))
    return np.linalg.norm(c["path"].astype(np.float64) - p, axis=-1)


@pytest.mark.parametrize("name", _contract_cases(), ids=lambda n: "-".join(map(str, n)))
def test_ik_contract_at_the_defaults(V, name):
    """tol = 1e-5, 20 steps: every point converges, the residual the kernel reports is the residual of the angles it returns
    (recomputed in float64, within 4x what the restatement's own report is off by), and the pen is where it was asked to be.  A
    goal that stays fixed while the arm moves on cannot be met along a path, so the goal variants are the one-point paths and
    the letters with the seed pose's orientation (ik_cases.letter_case)."""
    model = _model(V)
    c = IC.letter_case() if name[0] == "letters" else IC.case(*name)
    r32 = IC.solve(c, np.float32)
    own = np.abs(r32["residual"] - _residual64(c, r32["trajectory"])).max()
    got = _ik(model, c)
    assert (r32["status"] == 0).all(), "the case is not reachable at the defaults"
    assert (got["status"] == 0).all() and (got["iterations"] <= 20).all() and (got["iterations"] >= 0).all()
    true = _residual64(c, got["trajectory"])
    err = np.abs(got["residual"] - true).max()
    print("contract %s: iterations <= %d, |reported - float64 residual| kernel %.3e, restatement %.3e (bound 4x); tip error %.3e"
          % (name, got["iterations"].max(), err, own, true.max()))
    tol = float(np.float32(1e-5))
    assert err <= 4.0 * own and (got["residual"] < tol).all() and true.max() < tol + 4.0 * own
    fk = model.motion_fk(got["trajectory"], c["chain"])
    assert np.linalg.norm(fk.astype(np.float64) - c["path"], axis=-1).max() < tol + 4.0 * own
    if c["orient"] is not None:
        assert (got["rot_residual"] < float(np.float32(1e-4))).all()
    # the Python call is the C call
    py = model.motion_ik(c["path"], c["chain"], c["seed"], orientation=c["orient"],
                         limits=True if c["limits_mode"] == "chain" else None)
    assert all(_same(py[k], got[k]) for k in OUTPUTS if got[k] is not None) and py["converged"].all()
    assert (py["rot_residual"] is None) == (c["orient"] is None)


# ------------------------------------------------------------------------------------------------ 4. purity
def test_ik_rows_streams_outputs_and_chunks_change_no_bit(V):
    model = _model(V)
    for variant in (("none", "chain"), ("rows", "binding")):
        c = IC.case((300, 2, 3), *variant)
        got = _ik(model, c)
        assert _same(_ik(model, c)["trajectory"], got["trajectory"])                      # repetition
        for r in (0, 63, 64, 299):                                                        # a row alone, one among 300
            alone = _ik(model, c, rows=slice(r, r + 1))
            assert all(_same(alone[k], got[k][r:r + 1]) for k in OUTPUTS if got[k] is not None), r
        part = _ik(model, c, rows=slice(60, 130))                                         # other neighbours, another lane
        assert all(_same(part[k], got[k][60:130]) for k in OUTPUTS if got[k] is not None)
        only = _ik(model, c, want=("trajectory",))                                        # traj_dev alone
        assert _same(only["trajectory"], got["trajectory"])
        side = torch.cuda.Stream(device=model.device)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            other = _ik(model, c)
        assert all(_same(other[k], got[k]) for k in OUTPUTS if got[k] is not None)
        keep = model._motion_chunk
        kw = dict(orientation=c["orient"], limits=c["limits"])
        try:
            whole = model.motion_ik(c["path"], c["chain"], c["seed"], **kw)
            type(model)._motion_chunk = 64                                                # five chunks of 300 rows
            parts = model.motion_ik(c["path"], c["chain"], c["seed"], **kw)
        finally:
            type(model)._motion_chunk = keep
        assert all(_same(whole[k], got[k]) and _same(parts[k], got[k]) for k in OUTPUTS if got[k] is not None)
    # orientation='seed': folded on the host for host seeds, by avae_motion_pose for a device seed
    c = IC.letter_case()
    host = model.motion_ik(c["path"], c["chain"], c["seed"], orientation="seed")
    dev = model.motion_ik(torch.from_numpy(c["path"]).to(model.device), c["chain"], torch.from_numpy(c["seed"]).to(model.device),
                          orientation="seed")
    assert torch.is_tensor(dev["trajectory"]) and host["converged"].all() and bool(dev["converged"].all())
    assert np.abs(dev["trajectory"].cpu().numpy() - host["trajectory"]).max() < 1e-4
    one = model.motion_ik(c["path"], c["chain"], c["seed"][0], orientation="seed")
    assert _same(one["trajectory"], host["trajectory"])                                    # a [D] seed: one goal for every row
    goal = c["chain"].pose(c["seed"][0].astype(np.float64))[1]
    assert _same(model.motion_ik(c["path"], c["chain"], c["seed"], orientation=goal)["trajectory"], host["trajectory"])


# ------------------------------------------------------------------------------------------------ 5. edges
def test_ik_unreachable_and_non_finite_inputs_stay_in_their_row(V):
    model = _model(V)
    base = IC.case((5, 100, 7))
    clean = _ik(model, base)
    # row 2 is asked to write 2 m out of reach: finite angles, the cap, and the neighbours keep their bits
    far = dict(base, path=base["path"].copy())
    far["path"][2] += np.array([2.0, 0.0, 0.0], np.float32)
    got = _ik(model, far)
    assert np.isfinite(got["trajectory"]).all() and np.isfinite(got["residual"]).all()
    assert (got["status"][2] == 1).all() and (got["iterations"][2] == 20).all() and got["residual"][2].min() > 0.5
    r64 = K.ik(far["path"][2:3], far["frames"], far["axes"], far["seed"][2:3], limits=far["limits"])
    assert np.abs(got["residual"][2] - r64["residual"][0]).max() < 1e-3
    keep = [0, 1, 3, 4]
    assert all(_same(got[k][keep], clean[k][keep]) for k in OUTPUTS if clean[k] is not None)
    # a NaN point: NaN and status 3 there, the rest of the row as if the point were not in the path
    holed = dict(base, path=base["path"].copy())
    holed["path"][1, 40] = [0.8, np.nan, 0.2]
    holed["path"][3, 0, 2] = np.inf
    got = _ik(model, holed)
    for r, t in ((1, 40), (3, 0)):
        assert np.isnan(got["trajectory"][r, t]).all() and np.isnan(got["residual"][r, t])
        assert got["status"][r, t] == 3 and got["iterations"][r, t] == 0
        cut = dict(base, path=np.delete(base["path"][r:r + 1], t, axis=1), seed=base["seed"][r:r + 1])
        short = _ik(model, cut)
        assert all(_same(np.delete(got[k][r:r + 1], t, axis=1), short[k]) for k in OUTPUTS if short[k] is not None), (r, t)
    keep = [0, 2, 4]
    assert all(_same(got[k][keep], clean[k][keep]) for k in OUTPUTS if clean[k] is not None)
    # a NaN seed: the whole row
    sick = dict(base, seed=base["seed"].copy())
    sick["seed"][4, 6] = np.nan
    got = _ik(model, sick)
    assert np.isnan(got["trajectory"][4]).all() and np.isnan(got["residual"][4]).all() and (got["status"][4] == 3).all()
    assert all(_same(got[k][:4], clean[k][:4]) for k in OUTPUTS if clean[k] is not None)
    py = model.motion_ik(sick["path"], sick["chain"], sick["seed"])
    assert all(_same(py[k], got[k]) for k in OUTPUTS if got[k] is not None)
    assert py["converged"][:4].all() and not py["converged"][4].any()


def test_ik_c_abi_edges_and_errors(V):
    model = _model(V)
    L, h, s = model._L, model._h, _stream(model)
    c = IC.case((3, 2, 3), "rows", "chain")
    t = {k: _dev(model, c[k]) for k in ("path", "frames", "axes", "seed", "orient", "limits")}
    traj = torch.full((3, 2, 3), -7.0, device=model.device)
    pos = torch.full((3, 2, 3), -7.0, device=model.device)

    def ik(path=_p(t["path"]), rows=3, T=2, D=3, frames=_p(t["frames"]), axes=_p(t["axes"]), seed=_p(t["seed"]),
           orient=_p(t["orient"]), orient_rows=3, n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5, out=_p(traj)):
        return L.avae_motion_ik(h, path, rows, T, D, frames, axes, seed, orient, orient_rows, _p(t["limits"]), n_iters, tol, rot_tol,
                                damping, max_step, out, None, None, None, None, s)

    def pose(q=_p(t["seed"]), rows=1, T=3, D=3, frames=_p(t["frames"]), axes=_p(t["axes"]), out=_p(pos)):
        return L.avae_motion_pose(h, q, rows, T, D, frames, axes, out, None, None, s)
    assert ik(rows=0, orient_rows=0) == 0 and ik(rows=0, orient_rows=1) == 0 and pose(rows=0) == 0      # a no-op
    torch.cuda.synchronize()
    assert (traj == -7.0).all() and (pos == -7.0).all()
    inf, nan = float("inf"), float("nan")
    for kw, needle in ((dict(rows=-1), "rows"), (dict(D=0), "D"), (dict(D=17), "D"), (dict(T=0), "T"), (dict(T=1025), "T"),
                       (dict(n_iters=-1), "n_iters"), (dict(n_iters=1001), "n_iters"), (dict(damping=0.0), "damping"),
                       (dict(damping=nan), "damping"), (dict(max_step=0.0), "max_step"), (dict(max_step=-1.0), "max_step"),
                       (dict(tol=-1e-6), "tol"), (dict(tol=inf), "tol"), (dict(rot_tol=-1.0), "rot_tol"), (dict(rot_tol=nan), "rot_tol"),
                       (dict(orient_rows=2), "orient_rows"), (dict(orient_rows=0), "orient_rows"), (dict(path=None), "path_dev"),
                       (dict(frames=None), "frames_dev"), (dict(axes=None), "axes_dev"), (dict(seed=None), "seed_dev"),
                       (dict(out=None), "traj_dev")):
        assert ik(**kw) != 0 and needle in _err(model), (kw, _err(model))
    for kw, needle in ((dict(rows=-1), "rows"), (dict(D=0), "D"), (dict(D=17), "D"), (dict(T=0), "T"), (dict(T=1025), "T"),
                       (dict(q=None), "traj_dev"), (dict(frames=None), "frames_dev"), (dict(axes=None), "axes_dev"),
                       (dict(out=None), "output")):
        assert pose(**kw) != 0 and needle in _err(model), (kw, _err(model))
    torch.cuda.synchronize()
    assert (traj == -7.0).all() and (pos == -7.0).all()                                   # nothing was launched
    assert ik(orient=None, orient_rows=0) == 0 and ik(orient_rows=3) == 0 and pose() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(traj).all() and (traj != -7.0).all()
    assert (pos.flatten()[:9] != -7.0).all() and (pos.flatten()[9:] == -7.0).all()        # one row of three points was asked for
    with pytest.raises(ValueError):
        model.motion_ik(c["path"], c["chain"], c["seed"], damping=0.0)
    with pytest.raises(ValueError):
        model.motion_pose(c["path"][..., :2], c["chain"])                                 # two angles for three joints


# ------------------------------------------------------------------------------------------------ 6. the composed calls
def _writer():
    from vae_assoc_amd.kinematics import StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    fx, chain = R.fixture(), IC.fixture_chain()
    mean = np.zeros((7, 21))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(147, 0.012))
    return fx, basis, chain, StrokeCanvas()


def test_strokes_to_motion_is_the_separate_calls(V):
    model = _model(V)
    fx, basis, chain, canvas = _writer()
    strokes = IC.letters(3, 100)
    out = model.strokes_to_motion(strokes, basis, chain, canvas, fx["block_center"], fx["seed_pos"], orientation="seed")
    path = canvas.lift(strokes, fx["block_center"]).astype(np.float32)
    ik = model.motion_ik(path, chain, np.asarray(fx["seed_pos"]), orientation="seed")
    params = model.motion_fit(ik["trajectory"], basis)
    ev = model.motion_eval(params, basis, reference=ik["trajectory"])
    tip = np.linalg.norm(model.motion_fk(ev["trajectory"], chain).astype(np.float64) - path, axis=-1).max(1)
    assert _same(out["path"], path) and _same(out["trajectory"], ik["trajectory"]) and _same(out["params"], params)
    assert _same(out["image"], model.render_strokes(path, canvas)["image"]) and _same(out["fit_rmse"], ev["rmse"])
    assert out["converged"].shape == (3,) and out["converged"].all() and ik["converged"].all()
    assert out["params"].shape == (3, 147) and out["image"].shape == (3, 784) and out["tip_error"].shape == (3,)
    assert np.abs(out["tip_error"] - tip).max() < 1e-6
    print("strokes_to_motion N = 3, T = 100: fit_rmse max %.3e rad, tip_error max %.3e m" % (out["fit_rmse"].max(), out["tip_error"].max()))
    assert np.isfinite(out["fit_rmse"]).all() and np.isfinite(out["tip_error"]).all()
    dev = model.strokes_to_motion(torch.from_numpy(strokes).to(model.device), basis, chain, canvas, fx["block_center"],
                                  fx["seed_pos"], orientation="seed")
    assert all(torch.is_tensor(dev[k]) and _same(dev[k], out[k]) for k in out)
    with pytest.raises(ValueError):
        model.strokes_to_motion(strokes, basis, chain, canvas, fx["block_center"], fx["seed_pos"], stiffness=1.0)


def test_refine_pen_path_is_search_ik_and_fit(V):
    model = _model(V)
    fx, basis, chain, canvas = _writer()
    P, Rn = 2, 5
    z = np.random.default_rng(5).standard_normal((P, NZ)).astype(np.float32)
    img = model.draw_motion(model.generate(z)[1], basis, chain, canvas)["image"]
    kw = dict(n_rollouts=Rn, n_iters=2, seed=9, tol_search=0.0)
    seen, search = [], model.search

    def strict(*a, **k):                                                                 # a host round trip inside the search raises
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = search(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        seen.append(out)
        return out
    model.search = strict
    try:
        res = model.refine_pen_path(img, basis, chain, canvas, **kw)
    finally:
        del model.search
    again = model.refine_pen_path(img, basis, chain, canvas, **kw)
    assert len(seen) == 1 and seen[0]["avg_cost"].shape == (2, P)
    keys = ("mean", "var", "best_x", "best_cost", "avg_cost", "min_cost", "path", "trajectory", "params", "image", "converged")
    assert all(_same(res[k], again[k]) for k in keys) and _same(res["final"]["img_l2"], again["final"]["img_l2"])
    assert res["mean"].shape == (P, 42) and res["path"].shape == (P, 100, 3) and res["params"].shape == (P, 147)
    assert (res["n_applied"] == 2).all() and np.isfinite(res["avg_cost"]).all()
    assert _same(res["final"]["img_l2"], model.render_strokes(res["path"], canvas, target=img)["img_l2"])
    assert _same(res["image"], model.render_strokes(res["path"], canvas)["image"])
    start = model.motion_eval(model.generate(model.transform(img, 0))[1], basis)["trajectory"]
    ik = model.motion_ik(res["path"], chain, start[:, 0, :])
    assert _same(res["trajectory"], ik["trajectory"]) and _same(res["params"], model.motion_fit(ik["trajectory"], basis))
    assert _same(res["converged"], ik["converged"].all(1))
    assert _same(res["initial"]["img_l2"], model.render_strokes(model.motion_fk(start, chain), canvas, target=img)["img_l2"])
    # anchored: every candidate, and so the refined path, starts where the initial path's fit starts
    free = model.refine_pen_path(img, basis, chain, canvas, anchor_start=False, **kw)
    assert not _same(free["mean"], res["mean"])
    with pytest.raises(ValueError):
        model.refine_motion(img, basis, chain, canvas, space="cartesian")
    with pytest.raises(ValueError):
        model.refine_pen_path(img, basis, chain, canvas, stiffness=1.0)


# ------------------------------------------------------------------------------------------------ 7. every class and branch
def _steps_against_the_definition(model, c, label, variant, ns=(1, 4), **more):
    """``n_iters`` steps at ``tol = 0`` at every point: status 1, ``n_iters`` iterations, angles and residuals within 4x the
    restatement's own distance from the definition -> the kernel's outputs of the last ``n_iters``"""
    for n in ns:
        opt = dict(n_iters=n, tol=0.0, damping=IC.STEP_DAMPING[variant[0]], **more)
        r64, r32 = IC.solve(c, np.float64, **opt), IC.solve(c, np.float32, **opt)
        got = _ik(model, c, **opt)
        assert (got["status"] == 1).all() and (got["iterations"] == n).all() and (r64["status"] == 1).all()
        for k in ("trajectory", "residual", "rot_residual"):
            if r64[k] is None:
                assert got[k] is None
                continue
            own, err = IC.rel_err(r32[k], r64[k]), IC.rel_err(got[k], r64[k])
            print("ik %s %s n_iters=%d %s: kernel %.3e, restatement %.3e (bound 4x)" % (label, variant, n, k, err, own))
            assert got[k].shape == r64[k].shape and np.isfinite(got[k]).all() and err <= 4.0 * own, (k, n)
    return got


@pytest.mark.parametrize("variant", IC.VARIANTS, ids=["-".join(v) for v in IC.VARIANTS])
@pytest.mark.parametrize("shape", IC.IK_CLASS_SHAPES)
def test_ik_steps_inside_the_joint_classes(V, shape, variant):
    """The joints ``c >= D`` a class skips: D = 2 in the class D <= 4, D = 5 in D <= 8, D = 9, 12 and 15 in D <= 16 (the
    instantiations at the register limit, which the other shapes enter only with all sixteen joints), and T = 1024, the longest
    row.  A joint that is skipped where it should not be, or not skipped, moves the angles by far more than 4x a rounding error."""
    model = _model(V)
    c = IC.case(shape, *variant)
    got = _steps_against_the_definition(model, c, shape, variant)
    if variant[1] == "binding":
        lo, hi = c["limits"][0]
        assert (got["trajectory"][..., 0] >= lo).all() and (got["trajectory"][..., 0] <= hi).all()
    if shape == (3, 4, 12):                                                                # purity where DC = 16 and D < 16
        opt = dict(n_iters=4, tol=0.0, damping=IC.STEP_DAMPING[variant[0]])
        for r in range(3):
            alone = _ik(model, c, rows=slice(r, r + 1), **opt)
            assert all(_same(alone[k], got[k][r:r + 1]) for k in OUTPUTS if got[k] is not None), r
        for want in (("trajectory",), ("trajectory", "status"), ("trajectory", "residual", "iterations")):
            part = _ik(model, c, want=want, **opt)
            assert all(_same(part[k], got[k]) for k in want), want
        assert _same(_ik(model, c, **opt)["trajectory"], got["trajectory"])


@pytest.mark.parametrize("shape", IC.POSE_CLASS_SHAPES)
def test_pose_inside_the_joint_classes(V, shape):
    """D = 2, 5, 9, 15 and 12 over two tiles: inside a class the LDS rows of the angles are ``DC | 1`` floats apart while the
    copy-in divides by D, and the Jacobian's columns ``c >= D`` must not be stored.  All three outputs, and each alone."""
    model = _model(V)
    c, r64, r32 = IC.pose_refs(shape)
    got = _pose(model, c["traj"], c["frames"], c["axes"])
    for k in ("position", "rotation", "jacobian"):
        own, err = IC.rel_err(r32[k], r64[k]), IC.rel_err(got[k], r64[k])
        print("pose %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, k, err, own))
        assert got[k].shape == r64[k].shape and np.isfinite(got[k]).all() and err <= 4.0 * own, k
    for want in (("position",), ("rotation",), ("jacobian",)):
        part = _pose(model, c["traj"], c["frames"], c["axes"], want)
        assert set(part) == set(want) and _same(part[want[0]], got[want[0]]), want
    last = _pose(model, c["traj"][-1:, -1:], c["frames"], c["axes"])
    assert all(_same(last[k], got[k][-1:, -1:]) for k in got)


@pytest.mark.parametrize("limits", ["chain", "off"])
@pytest.mark.parametrize("max_step", [0.5, 0.05])
def test_ik_shrink_step_for_step(V, max_step, limits):
    """Targets 0.6 m further away (ik_cases.far_case): four steps in five are longer than 0.5 rad in some joint, nine in ten
    longer than 0.05, in both directions.  Four steps a point at ``tol = 0`` against the definition, and the definition's own steps
    show that the shrink decided them."""
    model = _model(V)
    c = IC.far_case(limits)
    r64, r32, steps = IC.far_refs(limits, max_step)
    assert IC.shrink_is_active(steps, max_step), "the shrink is not active"
    got = _ik(model, c, n_iters=4, tol=0.0, max_step=max_step)
    assert (got["status"] == 1).all() and (got["iterations"] == 4).all() and (r64["status"] == 1).all()
    for k in ("trajectory", "residual"):
        own, err = IC.rel_err(r32[k], r64[k]), IC.rel_err(got[k], r64[k])
        print("ik far max_step=%g limits=%s %s: kernel %.3e, restatement %.3e (bound 4x)" % (max_step, limits, k, err, own))
        assert np.isfinite(got[k]).all() and err <= 4.0 * own, k
    if limits == "chain":
        assert (got["trajectory"] >= c["limits"][:, 0]).all() and (got["trajectory"] <= c["limits"][:, 1]).all()


def _seed_residual_pair(c, got, r32):
    """the reported residuals of a run that took no step, kernel and restatement, against the float64 residual of the seed"""
    true = _residual64(c, np.broadcast_to(c["seed"][:, None, :], got["trajectory"].shape).astype(np.float64))
    return IC.rel_err(got["residual"], true), IC.rel_err(r32["residual"], true)


@pytest.mark.parametrize("D", [2, 3])
def test_ik_status_2_by_a_pivot_that_is_zero(V, D):
    """The planar arm, position only, ``damping = 1e-30``: damping^2 is 0 in float32 and the third pivot exactly 0, on any
    hardware.  Rows 0 and 2 end every point with status 2 after 0 steps with the seed's bits and the seed's residual; row 1 starts
    on its target and is done (status 0) before the solve is tried, in the same wave.  Statuses, iterations and angles are the
    restatement's to the bit; float64 has no underflow here and is not the oracle."""
    model = _model(V)
    c = IC.on_target(IC.planar_case(D), rows=[1])
    r32 = IC.solve(c, np.float32, damping=1e-30)
    got = _ik(model, c, damping=1e-30)
    assert (got["status"][[0, 2]] == 2).all() and (got["status"][1] == 0).all() and (got["iterations"] == 0).all()
    assert all(_same(got["trajectory"][:, t], c["seed"]) for t in range(got["trajectory"].shape[1]))
    assert all(_same(got[k], r32[k]) for k in ("trajectory", "iterations", "status"))
    err, own = _seed_residual_pair(c, got, r32)
    print("ik planar D=%d damping=1e-30: status 2 after 0 steps, seed residual kernel %.3e, restatement %.3e (bound 4x)" % (D, err, own))
    assert np.isfinite(got["residual"]).all() and err <= 4.0 * own and (got["residual"][1] < 1e-5).all()
    assert (got["residual"][[0, 2]] > 1e-3).all() and (IC.solve(c, np.float64, damping=1e-30)["status"] != 2).all()
    # the Python call is the C call, and says so
    py = model.motion_ik(c["path"], c["chain"], c["seed"], damping=1e-30)
    assert all(_same(py[k], got[k]) for k in OUTPUTS if got[k] is not None)
    assert not py["converged"][[0, 2]].any() and py["converged"][1].all()


@pytest.mark.parametrize("limits", ["chain", "off"])
@pytest.mark.parametrize("D", [2, 3])
def test_ik_status_2_by_a_step_that_is_not_finite(V, D, limits):
    """The planar arm with targets 0.1 m above its plane and ``damping = 1e-20``: damping^2 is a subnormal number, the pivot
    passes, e_z / damping^2 overflows and inf * 0 makes every dq NaN.  fmaxf drops the NaN and the clamp would turn it into lo =
    -3: the step must not be taken.  Status 2 after 0 steps, finite angles that are the carried q (the seed) to the bit and never
    lo, the seed's residual; everything equal to the restatement."""
    model = _model(V)
    c = IC.planar_case(D, lifted=True, limits=limits)
    r32 = IC.solve(c, np.float32, damping=1e-20)
    got = _ik(model, c, damping=1e-20)
    assert np.isfinite(got["trajectory"]).all() and np.isfinite(got["residual"]).all()
    assert (got["status"] == 2).all() and (got["iterations"] == 0).all() and (r32["status"] == 2).all()
    assert all(_same(got["trajectory"][:, t], c["seed"]) for t in range(got["trajectory"].shape[1]))
    assert (got["trajectory"] != np.float32(-3.0)).all() and (got["trajectory"] != np.float32(3.0)).all()
    assert all(_same(got[k], r32[k]) for k in ("trajectory", "iterations", "status"))
    err, own = _seed_residual_pair(c, got, r32)
    print("ik planar lifted D=%d limits=%s damping=1e-20: status 2 after 0 steps, seed residual kernel %.3e, restatement %.3e "
          "(bound 4x)" % (D, limits, err, own))
    assert err <= 4.0 * own and (got["residual"] >= 0.1).all()
    py = model.motion_ik(c["path"], c["chain"], c["seed"], damping=1e-20, limits=True if limits == "chain" else None)
    assert all(_same(py[k], got[k]) for k in OUTPUTS if got[k] is not None) and not py["converged"].any()
    # a damping that float32 can square takes its steps on the same case: nothing finite is refused
    assert (_ik(model, c, damping=1e-3)["iterations"] == 20).all()


HUGE = (3, 40, 1)           # (row, point, coordinate) of case((5, 100, 7)) that is made huge


def _with_target(base, value):
    c = dict(base, path=base["path"].copy())
    c["path"][HUGE] = value
    return c


def _rest_of_the_row_carries_on(model, c, got, clean):
    """the points before the huge one are the clean run's, the points after it the run that starts from the angles the huge point
    ended with, and the other rows keep their bits"""
    r, t, _ = HUGE
    tail = _ik(model, dict(c, path=c["path"][r:r + 1, t + 1:], seed=got["trajectory"][r:r + 1, t]))
    keep = [i for i in range(c["path"].shape[0]) if i != r]
    for k in OUTPUTS:
        if clean[k] is not None:
            assert _same(got[k][r:r + 1, t + 1:], tail[k]) and _same(got[k][r, :t], clean[k][r, :t]), k
            assert _same(got[k][keep], clean[k][keep]), k


def test_ik_status_2_by_a_huge_target_stays_at_its_point(V):
    """One coordinate of one target is 1e36: M^-1 e overflows.  The steps before that are finite and are taken (each cut to
    max_step: the restatement takes 2 here), the first one that is not ends the point: status 2, finite angles, an infinite
    residual.  The carried angles are the last good q, so the rest of the row is, to the bit, the run that starts from the angles
    this point returned -- and converges; it is not the run on the path without the point, which would start from the angles of
    the point before.  The other rows keep their bits."""
    model = _model(V)
    base = IC.case((5, 100, 7))
    clean = _ik(model, base)
    c = _with_target(base, 1e36)
    r32 = IC.solve(dict(c, shape=("huge", 1e36)), np.float32)
    got = _ik(model, c)
    r, t, _ = HUGE
    print("ik target 1e36: status %d after %d steps (restatement: %d after %d)"
          % (got["status"][r, t], got["iterations"][r, t], r32["status"][r, t], r32["iterations"][r, t]))
    assert got["status"][r, t] == 2 and r32["status"][r, t] == 2 and 0 <= got["iterations"][r, t] < 20
    assert np.isfinite(got["trajectory"]).all() and np.isinf(got["residual"][r, t])
    assert (np.delete(got["status"], t, axis=1) == 0).all() and np.isfinite(np.delete(got["residual"], t, axis=1)).all()
    _rest_of_the_row_carries_on(model, c, got, clean)
    # a point that fails before its first step is a deleted point: the largest float32 overflows e / L[0][0] or the next division
    c = _with_target(base, float(np.finfo(np.float32).max))
    got = _ik(model, c)
    assert got["status"][r, t] == 2 and got["iterations"][r, t] == 0 and np.isfinite(got["trajectory"]).all()
    assert _same(got["trajectory"][r, t], got["trajectory"][r, t - 1])
    _rest_of_the_row_carries_on(model, c, got, clean)
    cut = _ik(model, dict(base, path=np.delete(base["path"][r:r + 1], t, axis=1), seed=base["seed"][r:r + 1]))
    assert all(_same(np.delete(got[k][r:r + 1], t, axis=1), cut[k]) for k in OUTPUTS if cut[k] is not None)


def test_ik_huge_but_finite_targets_end_at_the_cap(V):
    """1e30 overflows nothing but the residual (e^2): twenty steps of max_step, status 1, finite angles, the residual inf; the
    following points converge from wherever that left the arm, and the other rows keep their bits."""
    model = _model(V)
    base = IC.case((5, 100, 7))
    clean = _ik(model, base)
    c = _with_target(base, 1e30)
    got = _ik(model, c)
    r, t, _ = HUGE
    assert got["status"][r, t] == 1 and got["iterations"][r, t] == 20 and np.isinf(got["residual"][r, t])
    assert np.isfinite(got["trajectory"]).all() and (got["trajectory"] >= c["limits"][:, 0]).all()
    assert (got["trajectory"] <= c["limits"][:, 1]).all()
    assert (np.delete(got["status"], t, axis=1) == 0).all(), "the following points do not converge"
    _rest_of_the_row_carries_on(model, c, got, clean)


def test_ik_zero_steps_and_a_seed_on_the_target(V):
    """``n_iters = 0``: status 1 after 0 steps with the seed's bits and the seed's residual at every point.  A seed on the target:
    status 0 after 0 steps, whatever ``n_iters`` is -- done is tested before the cap."""
    model = _model(V)
    base = IC.case((5, 100, 7))
    got, r32 = _ik(model, base, n_iters=0), IC.solve(base, np.float32, n_iters=0)
    assert (got["status"] == 1).all() and (got["iterations"] == 0).all()
    assert all(_same(got["trajectory"][:, t], base["seed"]) for t in range(100))
    err, own = _seed_residual_pair(base, got, r32)
    print("ik n_iters=0: seed residual kernel %.3e, restatement %.3e (bound 4x)" % (err, own))
    assert err <= 4.0 * own
    there = IC.on_target(base)
    for n in (0, 20):
        got = _ik(model, there, n_iters=n)
        assert (got["status"] == 0).all() and (got["iterations"] == 0).all() and (got["residual"] < 1e-5).all()
        assert all(_same(got["trajectory"][:, t], there["seed"]) for t in range(100))


def test_ik_limits_pinned_joint_and_seed_outside_the_box(V):
    """``lo == hi`` pins a joint: from the first step on its angle is lo to the bit, and the other six still reach every target at
    the defaults.  A seed outside the box is returned as it is after zero steps (the clamp belongs to the step) and is inside the
    box after one."""
    model = _model(V)
    c = IC.pinned_case()
    j, pin = IC.PIN_JOINT, c["limits"][IC.PIN_JOINT, 0]
    assert (IC.solve(c, np.float32)["status"] == 0).all(), "the pinned case is not reachable at the defaults"
    got = _ik(model, c)
    assert (got["status"] == 0).all() and (got["iterations"] >= 1).all() and _same(got["trajectory"][..., j], np.full((5, 100), pin))
    got = _steps_against_the_definition(model, c, "pinned", ("none", "pinned"))
    assert _same(got["trajectory"][..., j], np.full((5, 100), pin))
    base = IC.case((5, 100, 7))
    lo, hi = base["limits"][:, 0], base["limits"][:, 1]
    out_of = dict(base, seed=base["seed"].copy(), shape=("outside",) + base["shape"])
    out_of["seed"][:, 0], out_of["seed"][:, 3] = hi[0] + np.float32(0.3), lo[3] - np.float32(0.2)
    got = _ik(model, out_of, n_iters=0)
    assert (got["status"] == 1).all() and all(_same(got["trajectory"][:, t], out_of["seed"]) for t in range(100))
    got = _steps_against_the_definition(model, out_of, "seed outside the box", ("none", "chain"), ns=(1,))
    assert (got["trajectory"] >= lo).all() and (got["trajectory"] <= hi).all()
    assert (got["trajectory"][:, 0, 0] == hi[0]).any() or (got["trajectory"][:, 0, 3] == lo[3]).any()
