"""iLQR joint-trajectory synthesis (avae_motion_track, motion_track / strokes_to_motion(solver='ilqr')) on a real MI355X
(include/avae.h) against tests/track_reference.py.

1. the kernel try for try (``tol = 0``: 1 and 4 forced tries) against the float64 definition, within 4x the restatement's own worst
error over the same inputs (|err| / (|ref| + 1) per quantity, the controls against max |u| + 1), on cases where definition and
restatement take the same decisions (asserted first) -- ``iterations``, ``accepted`` and ``status`` must be the definition's;
2. every branch of the loop: an effort matrix, R = 0, a rejecting family, both lam_max exits, n_iters = 0, tol, binding limits,
non-finite inputs; 3. bit reproducibility and independence; 4. the C ABI's errors; 5. the composed call.  The shapes and cases are
tests/track_cases.py's; the measured pairs are in README.md and DESIGN.md section 29."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_cases as IC
import render_reference as R
import track_cases as TC
from conftest import make_arch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
OUTPUTS = ("trajectory", "controls", "cost0", "cost", "track_rmse", "iterations", "accepted", "status")
DTYPES = dict(trajectory=torch.float32, controls=torch.float32, cost0=torch.float64, cost=torch.float64, track_rmse=torch.float32,
              iterations=torch.int32, accepted=torch.int32, status=torch.int32)
DEFAULTS = dict(dt=0.01, track_weights=(10.0, 10.0, 50.0), effort_weight=0.01, limit_weight=0.0, n_iters=25, lam0=1.0, factor=10.0,
                lam_min=1e-6, lam_max=1e6, tol=1e-6)


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


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(model, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)


def _err(model):
    return model._L.avae_last_error(model._h).decode()


def _plan(model, rows, T, D):
    n = C.c_size_t(0)
    assert model._L.avae_motion_track_plan(rows, T, D, C.byref(n)) == 0
    return n.value


def _track(model, c, want=OUTPUTS, rows=None, extra_workspace=0, stream=None, expect=0, **options):
    """avae_motion_track on the rows ``rows`` (a slice) of a case -> dict of the NumPy outputs asked for, each prefilled with 7s;
    ``expect`` != 0: the return code the call must give (-> the error message)"""
    o = dict(DEFAULTS, **options)
    sl = slice(None) if rows is None else rows
    path, init = c["path"][sl], c["init"][sl]
    n, T, D = init.shape
    shapes = dict(trajectory=(n, T, D), controls=(n, max(T - 1, 0), D))
    out = {k: torch.full(shapes.get(k, (n,)), 7, dtype=DTYPES[k], device=model.device) for k in want}
    ws_bytes = o.pop("workspace_bytes", _plan(model, n, T, D) + extra_workspace)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=model.device)
    p, q0, fr, ax = (_dev(model, a) for a in (path, init, c["frames"], c["axes"]))
    E, lim = _dev(model, c.get("effort")), _dev(model, c.get("limits"))
    w = (C.c_float * 3)(*o["track_weights"])
    ptr = dict((k, out[k].data_ptr()) if k in out else (k, None) for k in OUTPUTS)
    ptr.update(o.pop("pointers", {}))
    s = C.c_void_p((stream or torch.cuda.current_stream(model.device)).cuda_stream)
    rc = model._L.avae_motion_track(
        model._h, ptr.get("path", p.data_ptr()), ptr.get("init", q0.data_ptr()), o.get("pass_rows", n), o.get("pass_T", T), o.get("pass_D", D),
        fr.data_ptr(), ax.data_ptr(), o["dt"], w, o["effort_weight"], None if E is None else E.data_ptr(),
        None if lim is None else lim.data_ptr(), o["limit_weight"], o["n_iters"], o["lam0"], o["factor"], o["lam_min"], o["lam_max"],
        o["tol"], ptr.get("workspace", ws.data_ptr()), ws_bytes, ptr["trajectory"], ptr["controls"], ptr["cost0"], ptr["cost"],
        ptr["track_rmse"], ptr["iterations"], ptr["accepted"], ptr["status"], s)
    if expect:
        assert rc == expect, (rc, _err(model))
        return _err(model)
    assert rc == 0, _err(model)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _against(got, r64, r32, label):
    """iterations, accepted and status are the definition's; trajectory, controls and cost within 4x the restatement's error"""
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(got[k], r64[k]), (label, k, got[k], r64[k])
    err, own = TC.errors(got, r64), TC.errors(r32, r64)
    print("%s kernel / restatement: %s" % (label, ", ".join("%s %.2e / %.2e" % (k, err[k], own[k]) for k in err)))
    for k in err:
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all() and err[k] <= 4.0 * own[k], (label, k, err[k], own[k])
    assert TC.rel_err(got["cost0"], r64["cost0"]) <= 4.0 * TC.rel_err(r32["cost0"], r64["cost0"]), label
    assert TC.rel_err(got["track_rmse"], r64["track_rmse"]) <= max(4.0 * TC.rel_err(r32["track_rmse"], r64["track_rmse"]),
                                                                   float(np.finfo(np.float32).eps)), label   # (a float output)


# ------------------------------------------------------------------------------------------------ 1. try for try
@pytest.mark.parametrize("tries", (1, 4))
@pytest.mark.parametrize("name", TC.STEP_CASES)
def test_tries_against_the_definition(V, name, tries):
    """(1, 1, 1): no controls; (3, 2, 3): one control that cannot move the pen; (3, 3, 3); (5, 100, 7) on the fixture arm ('figure');
    (2, 257, 16): five strides of the wave over T in the widest class; (65, 8, 7), (300, 3, 3): many workgroups; T = 63, 64, 65:
    the edges of a stride; D = 5, 9, 12, 15: the classes from the inside; an effort matrix; R = 0 with lam carrying the solve;
    binding limits.  D = 4, 8, 16 (also at T = 2): the tops of the classes, where the walk's uniform c < D branch is never taken;
    D = 6, 10, 13, 14; T = 127, 128, 129: the second stride's edges; 192, 193: a whole third stride; 1024 = kTrackMaxT; (1, 513,
    16): nine strides in the widest class (the third of its four tries is rejected)."""
    model = _model(V)
    c, opt = TC.named(name)
    opt = dict(opt, n_iters=tries, tol=0.0)
    r64, r32 = TC.refs(c, **opt)
    got = _track(model, c, **opt)
    _against(got, r64, r32, "%s after %d" % (name, tries))
    if name == "binding":
        hi = c["limits"][1, 1]
        assert (c["init"][:, :, 1] > hi).any() and (got["trajectory"][:, :, 1] > hi).any(), "the box does not bind"
    # the Python call is the C call
    py = model.motion_track(c["path"], c["chain"], init=c["init"], effort=c.get("effort"), limits=c.get("limits"), **opt)
    assert all(_same(py[k], got[k]) for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------ 2. the branches
def test_rejecting_family(V):
    """a = 0.12 from the seed repeated, lam0 = 1e-6, 8 tries: accept x3, reject x4, accept"""
    model = _model(V)
    c, opt = TC.named("rejecting")
    opt = dict(opt, n_iters=8, tol=0.0)
    r64, r32 = TC.refs(c, **opt)
    assert r64["decisions"] == ["aaarrrra"]
    _against(_track(model, c, **opt), r64, r32, "rejecting after 8")


@pytest.mark.parametrize("moving", (True, False), ids=("status0", "status2"))
def test_lam_max_exits(V, moving):
    """track_cases.dyadic_case: one accepted try onto J = 0 and then rejections until lam > lam_max (status 0); a first guess that
    stands still, J = 0 throughout, no try accepted (status 2)"""
    model = _model(V)
    c = TC.dyadic_case(moving)
    r64, r32 = TC.refs(c, **TC.DYADIC)
    assert (r64["status"] == (0 if moving else 2)).all() and (r64["accepted"] == int(moving)).all() and (r64["iterations"] < 20).all()
    got = _track(model, c, **TC.DYADIC)
    _against(got, r64, r32, "lam_max exit, status %d" % (0 if moving else 2))
    assert (got["cost"] == 0.0).all() and (got["controls"] == 0.0).all()


def test_no_tries(V):
    """n_iters = 0: status 1, the first controls and their rollout, cost = cost0"""
    model = _model(V)
    c, opt = TC.named("smooth-65-8-7")
    r64, r32 = TC.refs(c, n_iters=0)
    got = _track(model, c, n_iters=0)
    assert (got["status"] == 1).all() and (got["iterations"] == 0).all() and _same(got["cost"], got["cost0"])
    _against(got, r64, r32, "no tries")


def test_tol_ends_rows(V):
    """up to 25 tries on the figures: every row converges in the definition's try.  Three amplitudes at tol = 1e-5 (the sixth try
    gains 1.6e-6 to 7e-6 of the cost, the fifth 5e-4: no rounding moves a row across), the recorded a = 0.03 at the default 1e-6
    (its sixth try gains 1.6e-6, its seventh 1.9e-7)."""
    model = _model(V)
    c = TC.figure_case(TC.TOL_FIGURES, "ik")
    r64, r32 = TC.refs(c, tol=1e-5)
    assert (r64["status"] == 0).all() and (r64["iterations"] == 6).all()
    _against(_track(model, c, tol=1e-5), r64, r32, "figures at tol 1e-5")
    c = TC.figure_case((0.03,), "ik")
    r64, r32 = TC.refs(c)
    assert r64["status"][0] == 0 and r64["iterations"][0] == 7 and r64["accepted"][0] == 7
    _against(_track(model, c), r64, r32, "a = 0.03 at the defaults")


def test_non_finite_rows(V):
    """a NaN path point, a NaN and an infinite first guess: status 3 and NaN outputs for that row, the neighbours untouched"""
    model = _model(V)
    c, _ = TC.named("smooth-65-8-7")
    clean = _track(model, c, n_iters=2, tol=0.0)
    path, init = c["path"].copy(), c["init"].copy()
    path[3, 5, 1], init[40, 0, 6], init[64, 7, 0] = np.nan, np.nan, np.inf
    got = _track(model, dict(c, path=path, init=init), n_iters=2, tol=0.0)
    bad = np.zeros(65, dtype=bool)
    bad[[3, 40, 64]] = True
    assert (got["status"][bad] == 3).all() and (got["iterations"][bad] == 0).all() and (got["accepted"][bad] == 0).all()
    for k in ("trajectory", "controls", "cost0", "cost", "track_rmse"):
        assert np.isnan(got[k][bad]).all(), k
    assert all(_same(got[k][~bad], clean[k][~bad]) for k in OUTPUTS)
    # an infinite limit that is used: every row; one that is not (limit_weight = 0): none
    lim = c["chain"].limits.astype(np.float32)
    lim[2, 1] = np.inf
    assert (_track(model, dict(c, limits=lim), n_iters=1, limit_weight=1.0)["status"] == 3).all()
    assert all(_same(v, clean[k]) for k, v in _track(model, dict(c, limits=lim), n_iters=2, tol=0.0).items())


# ------------------------------------------------------------------------------------------------ 3. invariants
def test_rows_alone_among_many_streams_chunks(V):
    model = _model(V)
    c, _ = TC.named("smooth-300-3-3")
    opt = dict(n_iters=3, tol=0.0)
    whole = _track(model, c, **opt)
    for r in (0, 63, 64, 299):
        alone = _track(model, c, rows=slice(r, r + 1), **opt)
        assert all(_same(alone[k], whole[k][r:r + 1]) for k in OUTPUTS), r
    assert all(_same(v, whole[k]) for k, v in _track(model, c, **opt).items())                     # repetition
    assert all(_same(v, whole[k]) for k, v in _track(model, c, extra_workspace=4096 + 8, **opt).items())
    s1, s2 = torch.cuda.Stream(model.device), torch.cuda.Stream(model.device)
    a = _track(model, c, stream=s1, **opt)
    b = _track(model, c, stream=s2, **opt)
    assert all(_same(a[k], whole[k]) and _same(b[k], whole[k]) for k in OUTPUTS)
    try:
        model._track_chunk = 77
        py = model.motion_track(c["path"], c["chain"], init=c["init"], **opt)
    finally:
        model._track_chunk = None
    assert all(_same(py[k], whole[k]) for k in OUTPUTS)


def test_every_subset_of_outputs(V):
    model = _model(V)
    c, _ = TC.named("smooth-3-4-9")
    opt = dict(n_iters=2, tol=0.0)
    whole = _track(model, c, **opt)
    optional = OUTPUTS[1:]
    for mask in range(1 << len(optional)):
        want = ("trajectory",) + tuple(k for i, k in enumerate(optional) if mask >> i & 1)
        part = _track(model, c, want=want, **opt)
        assert all(_same(part[k], whole[k]) for k in want), want


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_plan_and_errors(V):
    model = _model(V)
    c, _ = TC.named("smooth-3-4-5")
    assert _plan(model, 5, 100, 7) == 5 * 89600 and _plan(model, 0, 1, 1) == 0
    assert _plan(model, 1, 1, 1) == 256 and _plan(model, 2, 1024, 16) == 2 * 1024 * (10 * 256 + 58 * 16)
    n = C.c_size_t(0)
    for bad in ((-1, 4, 5), (1, 0, 5), (1, 1025, 5), (1, 4, 0), (1, 4, 17)):
        assert model._L.avae_motion_track_plan(*bad, C.byref(n)) == 2
    before = _track(model, c, n_iters=1)
    for options, text in ((dict(pass_rows=-1), "rows"), (dict(pass_D=17), "D = 17"), (dict(pass_D=0), "D = 0"), (dict(pass_T=1025), "T = 1025"),
                          (dict(pass_T=0), "T = 0"), (dict(dt=0.0), "dt"), (dict(factor=1.0), "factor - 1"), (dict(lam0=0.0), "lam0"),
                          (dict(lam_min=0.0), "lam_min"), (dict(lam_max=0.5), "lam_max"), (dict(effort_weight=-1.0), "R"),
                          (dict(track_weights=(1.0, -1.0, 1.0)), "track_w"), (dict(track_weights=(1.0, float("nan"), 1.0)), "track_w"),
                          (dict(limit_weight=float("inf")), "limit_weight"), (dict(tol=-1e-3), "tol"), (dict(n_iters=-1), "n_iters"),
                          (dict(n_iters=1001), "n_iters"), (dict(workspace_bytes=_plan(model, 3, 4, 5) - 1), "workspace_bytes"),
                          (dict(pointers=dict(trajectory=None)), "traj_dev"), (dict(pointers=dict(workspace=None)), "workspace_dev"),
                          (dict(pointers=dict(path=None)), "path_dev"), (dict(pointers=dict(init=None)), "init_dev")):
        msg = _track(model, c, expect=2, **options)
        assert "avae_motion_track" in msg and text in msg, (options, msg)
    assert all(_same(v, before[k]) for k, v in _track(model, c, n_iters=1).items())
    none = _track(model, c, pass_rows=0)                                                   # rows == 0: a no-op
    assert all((v == 7).all() for v in none.values())
    py = model.motion_track(c["path"][:0], c["chain"], init=c["init"][:0])
    assert py["trajectory"].shape == (0, 4, 5) and py["controls"].shape == (0, 3, 5) and py["status"].shape == (0,)


# ------------------------------------------------------------------------------------------------ 5. the composed call
def test_strokes_to_motion_solvers(V):
    """solver='ik' is the call without the keyword, bit for bit; solver='ilqr' returns a smoother motion: max |second difference| /
    dt^2 below the IK route's on every seeded letter"""
    from vae_assoc_amd.kinematics import StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    model = _model(V)
    fx, chain = R.fixture(), IC.fixture_chain()
    strokes = IC.letters(4, 100)
    basis = MotionBasis(n_basis=20, n_dof=7, n_points=100)
    args = (strokes, basis, chain, StrokeCanvas(), fx["block_center"], np.asarray(fx["seed_pos"]))
    plain = model.strokes_to_motion(*args, orientation="seed")
    ik = model.strokes_to_motion(*args, solver="ik", orientation="seed")
    assert set(ik) == set(plain) and all(_same(ik[k], plain[k]) for k in plain)
    sm = model.strokes_to_motion(*args, solver="ilqr", orientation="seed")
    assert set(sm) == set(plain) | {"track_status", "track_cost"} and (sm["track_status"] <= 1).all()

    def roughness(t):
        return np.abs(t[:, 2:] - 2.0 * t[:, 1:-1] + t[:, :-2]).max(axis=(1, 2)) / 0.01 ** 2
    print("max |second difference| / dt^2, ik / ilqr: %s / %s; tip_error ik / ilqr: %s / %s; fit_rmse ik / ilqr: %.2e / %.2e"
          % (roughness(plain["trajectory"]), roughness(sm["trajectory"]), plain["tip_error"], sm["tip_error"],
             plain["fit_rmse"].max(), sm["fit_rmse"].max()))
    assert (roughness(sm["trajectory"]) < roughness(plain["trajectory"])).all()
    # bitwise what the separate calls give
    tr = model.motion_track(plain["path"], chain, init=plain["trajectory"])
    assert _same(tr["trajectory"], sm["trajectory"]) and _same(tr["cost"], sm["track_cost"]) and _same(tr["status"], sm["track_status"])
    # the first guess made by motion_ik inside motion_track
    own = model.motion_track(plain["path"], chain, seed=np.asarray(fx["seed_pos"]), orientation="seed")
    assert _same(own["trajectory"], sm["trajectory"])
    with pytest.raises(ValueError, match="solver"):
        model.strokes_to_motion(*args, solver="lqr")
    with pytest.raises(ValueError, match="track_options"):
        model.strokes_to_motion(*args, track_options=dict(n_iters=3))


def test_refine_pen_path_solvers(V):
    """refine_pen_path: solver='ik' is the call without the keyword; under 'ilqr' the refined path is the same, and trajectory and
    params are motion_track's from the inverse-kinematics solution and their fit"""
    from vae_assoc_amd.kinematics import StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    model = _model(V)
    fx, chain, canvas = R.fixture(), IC.fixture_chain(), StrokeCanvas()
    mean = np.zeros((7, 21))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(147, 0.012))
    z = np.random.default_rng(5).standard_normal((2, NZ)).astype(np.float32)
    img = model.draw_motion(model.generate(z)[1], basis, chain, canvas)["image"]
    kw = dict(n_rollouts=5, n_iters=2, seed=9, tol_search=0.0)
    plain = model.refine_pen_path(img, basis, chain, canvas, **kw)
    ik = model.refine_pen_path(img, basis, chain, canvas, solver="ik", **kw)
    keys = ("mean", "path", "trajectory", "params", "image", "converged")
    assert set(ik) == set(plain) and all(_same(ik[k], plain[k]) for k in keys)
    sm = model.refine_pen_path(img, basis, chain, canvas, solver="ilqr", track_options=dict(n_iters=3), **kw)
    assert set(sm) == set(plain) | {"track_status", "track_cost"}
    assert _same(sm["path"], plain["path"]) and _same(sm["converged"], plain["converged"])
    tr = model.motion_track(plain["path"], chain, init=plain["trajectory"], n_iters=3)
    assert _same(sm["trajectory"], tr["trajectory"]) and _same(sm["track_cost"], tr["cost"]) and _same(sm["track_status"], tr["status"])
    assert _same(sm["params"], model.motion_fit(tr["trajectory"], basis))
    with pytest.raises(ValueError, match="solver"):
        model.refine_pen_path(img, basis, chain, canvas, solver="newton", **kw)
