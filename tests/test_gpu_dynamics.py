"""Joint-space inertia and inverse dynamics (avae_motion_dynamics, motion_dynamics / motion_effort) on a real MI355X
(include/avae.h) against tests/dynamics_reference.py.

1. the kernel against the float64 by-value definition, within 4x the float32 restatement's own worst error over the same inputs
(the rule of test_gpu_ik.py; |err| / (|ref| + 1) per output): the shapes of the issue, every joint count class from the inside and
at its top, the edges of the 64-point tile, with and without speeds and accelerations, gravity 0 and tilted, a body of mass 0;
2. the outputs among themselves; 3. bit reproducibility and independence; 4. non-finite points, guard rows, the errors of the
C ABI; 5. the Python calls and motion_track with the arm's inertia as its effort matrix.  The measured pairs are in README.md and
DESIGN.md section 32."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import dynamics_reference as Dy
import ik_cases as IC
from conftest import make_arch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
OUTPUTS = ("inertia", "gravity", "coriolis", "torque")
TILE = 64                                                                    # kDynThreads: points a workgroup takes at a time

SHAPES = [(1, 1, 1), (3, 2, 3), (5, 100, 7), (2, 257, 16), (1, 1024, 16), (65, 3, 7), (300, 2, 3)]
CLASS_SHAPES = [(2, 5, D) for D in (2, 4, 5, 8, 9, 12, 15)]                  # inside and at the top of the classes D <= 4, 8, 16
TILE_SHAPES = [(1, TILE - 1, 7), (TILE, 1, 7), (1, TILE + 1, 7)]


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V):
    """one small fp32 relu model (the nets of test_gpu_ik.py), shared by every test here"""
    if "m" not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS["m"] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3)
    return _MODELS["m"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(model, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(model.device)


def _p(t):
    return None if t is None else t.data_ptr()


def _err(model):
    return model._L.avae_last_error(model._h).decode()


def _dyn(model, c, want=OUTPUTS, vel=True, acc=True, gravity=Dy.GRAVITY, rows=None, stream=None):
    """avae_motion_dynamics on a case of dynamics_reference (``rows``: a slice of its rows) -> dict of the NumPy outputs asked for.
    Every output lies between two guard rows of -7 that must come back untouched."""
    sl = slice(None) if rows is None else rows
    traj = c["traj"][sl]
    N, T, D = traj.shape
    tails = dict(inertia=(D,), gravity=(), coriolis=(), torque=())
    out = {k: torch.full((N + 2, T, D) + tails[k], -7.0, device=model.device) for k in want}
    ts = [_dev(model, x) for x in (traj, c["vel"][sl] if vel else None, c["acc"][sl] if acc else None, c["frames"], c["axes"],
                                   c["bodies"])]
    s = torch.cuda.current_stream(model.device) if stream is None else stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(model.device))
    inner = {k: v[1:] for k, v in out.items()}
    rc = model._L.avae_motion_dynamics(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, T, D, _p(ts[3]), _p(ts[4]), _p(ts[5]),
                                       (C.c_float * 3)(*gravity), _p(inner.get("inertia")), _p(inner.get("gravity")),
                                       _p(inner.get("coriolis")), _p(inner.get("torque")), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    res = {}
    for k, v in out.items():
        v = v.cpu().numpy()
        assert (v[0] == -7.0).all() and (v[-1] == -7.0).all(), "%s: a guard row was written" % k
        res[k] = v[1:-1]
    return res


def _check(label, got, r64, r32):
    """every output within 4x the restatement's own error; -> the (kernel, restatement) pairs"""
    pairs = {}
    for k in got:
        own, err = Dy.rel_err(r32[k], r64[k]), Dy.rel_err(got[k], r64[k])
        pairs[k] = (err, own)
        print("dynamics %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (label, k, err, own))
    for k in got:
        assert got[k].shape == r64[k].shape and pairs[k][0] <= 4.0 * pairs[k][1], (label, k, pairs[k])
    return pairs


def _combined(o, acc):
    """inertia @ a + coriolis + gravity in float64 from an output dict"""
    a = np.zeros(o["gravity"].shape) if acc is None else acc.astype(np.float64)
    return np.einsum("rtij,rtj->rti", o["inertia"].astype(np.float64), a) + o["coriolis"] + o["gravity"]


# ------------------------------------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("shape", SHAPES + CLASS_SHAPES + TILE_SHAPES)
def test_dynamics_against_the_definition(V, shape):
    """(rows, T, D) of the issue -- the fixture arm inside its limits up to D = 7, a random chain with random positive-definite
    inertias beyond --, D = 2, 4, 5, 8, 9, 12, 15, and 63, 64 and 65 points: the edges of the 64-point tile"""
    model = _model(V)
    c = Dy.case(shape)
    r64, r32 = Dy.refs(c)
    got = _dyn(model, c)
    _check(shape, got, r64, r32)
    assert _same(got["inertia"], np.swapaxes(got["inertia"], -1, -2)), "inertia is not symmetric bit for bit"
    # torque = inertia @ a + coriolis + gravity, from the kernel's own outputs, as well as the restatement's own add up
    own, err = Dy.rel_err(_combined(r32, c["acc"]), r64["torque"]), Dy.rel_err(_combined(got, c["acc"]), r64["torque"])
    print("dynamics %s M a + c + g: kernel %.3e, restatement %.3e" % (shape, err, own))
    assert err <= 4.0 * own


@pytest.mark.parametrize("vel,acc,gravity", [(False, False, Dy.GRAVITY), (True, False, (0.0, 0.0, 0.0)), (False, True, (0.0, 0.0, 0.0)),
                                             (True, True, (3.0, -4.0, -8.0)), (False, True, (3.0, -4.0, -8.0))])
@pytest.mark.parametrize("shape", [(3, 40, 7), (2, 33, 12)])
def test_derivative_and_gravity_variants(V, shape, vel, acc, gravity):
    """with and without vel, with and without acc, gravity 0 and tilted; with vel = NULL and gravity 0 the torque is M(q) a"""
    model = _model(V)
    c = Dy.case(shape)
    r64, r32 = Dy.refs(c, vel, acc, gravity)
    got = _dyn(model, c, vel=vel, acc=acc, gravity=gravity)
    _check((shape, vel, acc, gravity), got, r64, r32)
    if not vel and acc and not any(gravity):
        Ma = lambda o: np.einsum("rtij,rtj->rti", o["inertia"].astype(np.float64), c["acc"].astype(np.float64))
        own, err = Dy.rel_err(Ma(r32), r64["torque"]), Dy.rel_err(Ma(got), r64["torque"])
        print("dynamics %s M a against torque: kernel %.3e, restatement %.3e" % (shape, err, own))
        assert err <= 4.0 * own and not got["coriolis"].any() and not got["gravity"].any()
    if not vel:
        assert not got["coriolis"].any()


def test_a_body_of_mass_zero(V):
    model = _model(V)
    c = Dy.case((2, 5, 6), seed=1, massless=(2, 5))
    assert not c["bodies"][2].any() and not c["bodies"][5].any() and c["bodies"][3, 0] > 0.0
    r64, r32 = Dy.refs(c)
    _check("massless", _dyn(model, c), r64, r32)


# ------------------------------------------------------------------------------------------------ 3. purity, bit for bit
def test_rows_alone_among_many_streams_repetition_chunks(V):
    """a row's bits do not depend on the rows around it, the stream, the repetition or the chunk it travels in"""
    model = _model(V)
    c = Dy.case((300, 2, 3))
    whole = _dyn(model, c)
    again = _dyn(model, c)
    side = _dyn(model, c, stream=torch.cuda.Stream(model.device))
    for k in OUTPUTS:
        assert _same(whole[k], again[k]) and _same(whole[k], side[k]), k
    for r in (0, 17, 299):
        alone = _dyn(model, c, rows=slice(r, r + 1))
        assert all(_same(alone[k], whole[k][r:r + 1]) for k in OUTPUTS), r
    parts = [_dyn(model, c, rows=slice(r0, r1)) for r0, r1 in ((0, 37), (37, 64), (64, 300))]
    for k in OUTPUTS:
        assert _same(np.concatenate([p[k] for p in parts]), whole[k]), k
    c16 = Dy.case((2, 257, 16))
    whole = _dyn(model, c16)
    parts = [_dyn(model, c16, rows=slice(r, r + 1)) for r in range(2)]
    assert all(_same(np.concatenate([p[k] for p in parts]), whole[k]) for k in OUTPUTS)


def test_every_subset_of_outputs(V):
    """the 15 subsets of the four outputs: each output's bits are those of the call that asks for all four"""
    model = _model(V)
    for shape in ((3, 40, 7), (2, 33, 12)):
        c = Dy.case(shape)
        full = _dyn(model, c)
        for n in range(1, 4):
            for want in itertools.combinations(OUTPUTS, n):
                part = _dyn(model, c, want)
                assert set(part) == set(want) and all(_same(part[k], full[k]) for k in want), want


# ------------------------------------------------------------------------------------------------ 4. non-finite points, errors
def test_a_non_finite_point_stays_in_its_point(V):
    model = _model(V)
    base = Dy.case((3, 70, 7))
    clean = _dyn(model, base)
    for which, at, value in (("traj", (0, 0, 0), np.nan), ("traj", (1, 63, 6), np.inf), ("vel", (1, 64, 3), np.nan),
                             ("vel", (2, 69, 0), -np.inf), ("acc", (0, 65, 6), np.nan), ("acc", (2, 1, 1), np.inf)):
        c = dict(base)
        c[which] = base[which].copy()
        c[which][at] = value
        got = _dyn(model, c)
        for k in OUTPUTS:
            assert np.isnan(got[k][at[:2]]).all(), (which, at, k)
            keep = np.ones(got[k].shape[:2], dtype=bool)
            keep[at[:2]] = False
            assert _same(got[k][keep], clean[k][keep]), (which, at, k)
        # a speed that is not asked for is not read
        if which == "vel":
            assert all(_same(_dyn(model, c, vel=False)[k], _dyn(model, base, vel=False)[k]) for k in OUTPUTS)


def test_errors_and_the_empty_call(V):
    model = _model(V)
    L, h = model._L, model._h
    c = Dy.case((3, 2, 3))
    ts = [_dev(model, c[k]) for k in ("traj", "vel", "acc", "frames", "axes", "bodies")]
    out = torch.full((3, 2, 3), -7.0, device=model.device)
    g = (C.c_float * 3)(0.0, 0.0, -9.81)

    def call(rows=3, T=2, D=3, traj=ts[0], frames=ts[3], axes=ts[4], bodies=ts[5], gravity=g, outs=(None, None, None, out)):
        return L.avae_motion_dynamics(h, _p(traj), _p(ts[1]), _p(ts[2]), rows, T, D, _p(frames), _p(axes), _p(bodies), gravity,
                                      *[_p(o) for o in outs], None)
    for kw, needle in ((dict(rows=-1), "rows"), (dict(D=0), "D"), (dict(D=17), "D"), (dict(T=0), "T"), (dict(T=1025), "T"),
                       (dict(gravity=(C.c_float * 3)(0.0, float("nan"), 0.0)), "gravity"),
                       (dict(gravity=(C.c_float * 3)(float("inf"), 0.0, 0.0)), "gravity"), (dict(gravity=None), "gravity"),
                       (dict(traj=None), "traj_dev"), (dict(frames=None), "frames_dev"), (dict(axes=None), "axes_dev"),
                       (dict(bodies=None), "bodies_dev"), (dict(outs=(None, None, None, None)), "output")):
        assert call(**kw) != 0 and needle in _err(model), (kw, _err(model))
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                               # nothing was launched
    assert call(rows=0) == 0 and call(rows=0, traj=None, outs=(None, None, None, out)) != 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), _dyn(model, c, ("torque",))["torque"])


# ------------------------------------------------------------------------------------------------ 5. the Python calls
def test_motion_dynamics_call(V):
    """the dict of the Python call is the C call's bits; dt gives motion_track's finite differences; peak_torque and torque_ratio"""
    model = _model(V)
    c = Dy.case((5, 100, 7))
    ref = _dyn(model, c)
    py = V.motion_dynamics(model, c["traj"], c["chain"], velocities=c["vel"], accelerations=c["acc"], inertia=True)
    assert set(py) == {"torque", "gravity", "coriolis", "inertia", "peak_torque", "torque_ratio"}
    assert all(isinstance(py[k], np.ndarray) and _same(py[k], ref[k]) for k in OUTPUTS)
    peak = np.abs(ref["torque"]).max(axis=1)
    assert _same(py["peak_torque"], peak) and _same(py["torque_ratio"], peak / c["chain"].effort_limits.astype(np.float32))
    t = torch.from_numpy(c["traj"]).to(model.device)
    dev = V.motion_dynamics(model, t, c["chain"])
    assert set(dev) == {"torque", "gravity", "coriolis", "peak_torque", "torque_ratio"} and all(v.is_cuda for v in dev.values())
    assert _same(dev["gravity"].cpu().numpy(), ref["gravity"]) and _same(dev["torque"].cpu().numpy(), ref["gravity"])
    # dt: v_0 = 0, v_t = (q_t - q_(t-1)) / dt, a_t = (v_(t+1) - v_t) / dt, a_(T-1) = 0, formed in float32
    dt = np.float32(0.01)
    v = np.zeros_like(c["traj"])
    v[:, 1:] = (c["traj"][:, 1:] - c["traj"][:, :-1]) / dt
    a = np.zeros_like(c["traj"])
    a[:, :-1] = (v[:, 1:] - v[:, :-1]) / dt
    fd = V.motion_dynamics(model, c["traj"], c["chain"], dt=0.01)
    given = V.motion_dynamics(model, c["traj"], c["chain"], velocities=v, accelerations=a)
    assert all(_same(fd[k], given[k]) for k in fd)
    bare = V.motion_dynamics(model, c["traj"], type(c["chain"])([dict(j, effort=None) for j in Dy.fixture()["joints"]]))
    assert set(bare) == {"torque", "gravity", "coriolis"} and _same(bare["torque"], ref["gravity"])
    empty = V.motion_dynamics(model, np.zeros((0, 4, 7), np.float32), c["chain"], inertia=True)
    assert empty["torque"].shape == (0, 4, 7) and empty["inertia"].shape == (0, 4, 7, 7) and empty["peak_torque"].shape == (0, 7)
    with pytest.raises(ValueError, match="inertial"):
        V.motion_dynamics(model, c["traj"], IC.fixture_chain())


def test_motion_effort_against_the_definition(V):
    """effort = sum_(t < T - 1) |M(q_t) u_t|^2 against the float64 definition: within 4x the restatement's own error plus
    n 2^-24, the worst a float32 sum of the n = (T - 1) D non-negative squares can lose in any order"""
    model = _model(V)
    c = Dy.case((5, 100, 7))
    smooth = np.cumsum(np.cumsum(c["acc"] * np.float32(1e-4), axis=1), axis=1).astype(np.float32) * np.float32(0.02) + c["traj"][:, :1]
    want, u = Dy.effort64(smooth, c["frames"], c["axes"], c["bodies"], 0.01)
    full = np.concatenate([u, np.zeros_like(u[:, :1])], axis=1)
    tau32 = Dy.dynamics32(smooth, None, full, c["frames"], c["axes"], c["bodies"], (0.0, 0.0, 0.0))["torque"].astype(np.float64)
    own = Dy.rel_err((tau32[:, :-1] ** 2).sum((1, 2)), want)
    got = V.motion_effort(model, smooth, c["chain"], dt=0.01)
    err = Dy.rel_err(got["effort"], want)
    print("motion_effort: %s, kernel %.3e, restatement %.3e" % (np.round(want, 3), err, own))
    assert got["effort"].shape == (5,) and _same(got["controls"], u) and np.isfinite(got["effort"]).all()
    assert err <= 4.0 * own + u[0].size * 2.0 ** -24
    t = torch.from_numpy(smooth).to(model.device)
    dev = V.motion_effort(model, t, c["chain"])
    assert dev["effort"].is_cuda and _same(dev["effort"].cpu().numpy(), got["effort"])


def test_motion_track_with_the_arms_inertia_as_effort(V):
    """motion_track(effort=chain.mass_matrix(seed)) on the four seeded letters of test_gpu_track.py: it runs, no row ends with
    status 2 or 3 and its motion_effort is finite.  The efforts of the three routes are figures, not assertions."""
    from vae_assoc_amd.kinematics import StrokeCanvas
    model = _model(V)
    fx, chain = Dy.fixture(), Dy.fixture_chain()
    seed = np.asarray(fx["seed_pos"])
    path = StrokeCanvas().lift(IC.letters(4, 100), fx["block_center"], 0.0).astype(np.float32)
    ik = model.motion_ik(path, chain, seed, orientation="seed")
    plain = model.motion_track(path, chain, init=ik["trajectory"])
    heavy = model.motion_track(path, chain, init=ik["trajectory"], effort=chain.mass_matrix(seed))
    assert not np.isin(heavy["status"], (2, 3)).any() and np.isfinite(heavy["trajectory"]).all()
    e = [V.motion_effort(model, t, chain, dt=0.01)["effort"] for t in (ik["trajectory"], plain["trajectory"], heavy["trajectory"])]
    print("sum |M(q_t) u_t|^2 on the four letters: IK %s, motion_track(effort=None) %s, motion_track(effort=M(seed)) %s; status %s, "
          "track_rmse %s / %s" % (e[0], e[1], e[2], heavy["status"], plain["track_rmse"], heavy["track_rmse"]))
    assert np.isfinite(e[2]).all()
    ratio = V.motion_dynamics(model, heavy["trajectory"], chain, dt=0.01)["torque_ratio"]
    print("torque_ratio of the tracked letters (max over joints): %s" % ratio.max(axis=1))
