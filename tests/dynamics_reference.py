"""The definition of joint-space inertia and inverse dynamics (avae_motion_dynamics, include/avae.h) in NumPy
float64 *by value* -- Jacobian sums for M, the potential's gradient for g, the Christoffel terms of M for c -- and next to it a float32
restatement of the kernel: recursive Newton-Euler with the operations in the order csrc/avae_dynamics.h writes down.  The two share no
algebra, so they agree only if the recursion is right; the restatement's distance from the definition on a set of inputs is what the GPU
tests build their bounds from (4x, the rule of test_gpu_ik.py).

Both take the packed constants the device call takes (``KinematicChain.packed()`` and ``.bodies()``: the float32 values, widened for
the definition), so that the three of them start from the same bits."""
import json
import os

import numpy as np

from ik_reference import _cross, _frame32

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GRAVITY = (0.0, 0.0, -9.81)


def fixture():
    with open(os.path.join(HERE, "golden", "baxter_right_dynamics.json")) as f:
        return json.load(f)


def _tensor(b):
    """bodies[k][4:] -> the symmetric 3 x 3 matrix"""
    return np.array([[b[0], b[1], b[2]], [b[1], b[3], b[4]], [b[2], b[4], b[5]]], dtype=b.dtype)


# ------------------------------------------------------------------------------------------------ the definition, float64
def world64(q, frames, axes, bodies):
    """q [n, D] -> (o, z [n, D, 3] as ik_reference.walk64 gives them, the centres of mass pc = o + R^+ c [n, D, 3] and the inertias
    R^+ I R^+T [n, D, 3, 3] in the base frame, R^+ the rotation right behind each joint's own)"""
    q = np.asarray(q, dtype=np.float64)
    F, A, B = (np.asarray(x, dtype=np.float64) for x in (frames, axes, bodies))
    n, D = q.shape
    R = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    p = np.zeros((n, 3))
    o, z, pc = (np.empty((n, D, 3)) for _ in range(3))
    tens = np.empty((n, D, 3, 3))
    for j in range(D):
        p = p + R @ F[j, :, 3]
        R = R @ F[j, :, :3]
        o[:, j], z[:, j] = p, R @ A[j]
        a = A[j]
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
        R = R @ (c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a))
        pc[:, j] = p + R @ B[j, 1:4]
        tens[:, j] = R @ _tensor(B[j, 4:]) @ np.swapaxes(R, -1, -2)
    return o, z, pc, tens


def _body_jacobians(o, z, pc):
    """-> Jv [n, k, 3, j] = z_j x (pc_k - o_j) and Jw [n, k, 3, j] = z_j for j <= k, 0 otherwise"""
    D = o.shape[1]
    keep = (np.arange(D)[None, :] <= np.arange(D)[:, None]).astype(np.float64)             # [k, j]
    Jv = np.cross(z[:, None, :, :], pc[:, :, None, :] - o[:, None, :, :]) * keep[None, :, :, None]
    Jw = np.broadcast_to(z[:, None, :, :], Jv.shape) * keep[None, :, :, None]
    return np.swapaxes(Jv, -1, -2), np.swapaxes(Jw, -1, -2)


def mass_matrix64(q, frames, axes, bodies):
    """M = sum_k [ m_k Jv_k^T Jv_k + Jw_k^T I_k^w Jw_k ]  -> [n, D, D]"""
    o, z, pc, tens = world64(q, frames, axes, bodies)
    Jv, Jw = _body_jacobians(o, z, pc)
    m = np.asarray(bodies, dtype=np.float64)[:, 0]
    n, D = o.shape[:2]
    flat = lambda x: x.reshape(n, 3 * D, D)                                  # the sums over k and the three components as one
    return np.swapaxes(flat(Jv * m[None, :, None, None]), 1, 2) @ flat(Jv) + np.swapaxes(flat(Jw), 1, 2) @ flat(tens @ Jw)


def potential64(q, frames, axes, bodies, gravity=GRAVITY):
    """V = -sum_k m_k grav . pc_k  -> [n]"""
    pc = world64(q, frames, axes, bodies)[2]
    return -np.einsum("k,nka,a->n", np.asarray(bodies, dtype=np.float64)[:, 0], pc, np.asarray(gravity, dtype=np.float64))


def gravity64(q, frames, axes, bodies, gravity=GRAVITY):
    """g = dV/dq, with d pc_k / d q_j = Jv_k[:, j]  -> [n, D]"""
    o, z, pc, _ = world64(q, frames, axes, bodies)
    Jv = _body_jacobians(o, z, pc)[0]
    return -np.einsum("k,nkaj,a->nj", np.asarray(bodies, dtype=np.float64)[:, 0], Jv, np.asarray(gravity, dtype=np.float64))


def mass_matrix_gradient64(q, frames, axes, bodies, h=1e-5):
    """dM[n, i, j, k] = dM_ij / dq_k by central differences of ``mass_matrix64`` (about 1e-10 of M at h = 1e-5)"""
    q = np.asarray(q, dtype=np.float64)
    n, D = q.shape
    dM = np.empty((n, D, D, D))
    for k in range(D):
        e = np.zeros(D)
        e[k] = h
        dM[..., k] = (mass_matrix64(q + e, frames, axes, bodies) - mass_matrix64(q - e, frames, axes, bodies)) / (2.0 * h)
    return dM


def coriolis64(q, v, frames, axes, bodies):
    """the Christoffel terms of M:  c_i = sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) v_j v_k  -> [n, D]"""
    dM = mass_matrix_gradient64(q, frames, axes, bodies)
    v = np.asarray(v, dtype=np.float64)
    return np.einsum("nijk,nj,nk->ni", dM, v, v) - 0.5 * np.einsum("njki,nj,nk->ni", dM, v, v)


def dynamics64(traj, vel, acc, frames, axes, bodies, gravity=GRAVITY):
    """The definition of avae_motion_dynamics on [rows, T, D] inputs (``vel`` / ``acc`` None: zeros) -> dict of inertia
    [rows, T, D, D], gravity, coriolis, torque [rows, T, D]; a point with a non-finite input is NaN"""
    traj = np.asarray(traj, dtype=np.float64)
    rows, T, D = traj.shape
    q = traj.reshape(-1, D)
    v = np.zeros_like(q) if vel is None else np.asarray(vel, dtype=np.float64).reshape(-1, D)
    a = np.zeros_like(q) if acc is None else np.asarray(acc, dtype=np.float64).reshape(-1, D)
    bad = ~(np.isfinite(q).all(1) & np.isfinite(v).all(1) & np.isfinite(a).all(1))
    q, v, a = (np.where(bad[:, None], 0.0, x) for x in (q, v, a))
    M = mass_matrix64(q, frames, axes, bodies)
    g = gravity64(q, frames, axes, bodies, gravity)
    c = coriolis64(q, v, frames, axes, bodies) if vel is not None else np.zeros_like(q)
    tau = np.einsum("nij,nj->ni", M, a) + c + g
    M[bad], g[bad], c[bad], tau[bad] = np.nan, np.nan, np.nan, np.nan
    return dict(inertia=M.reshape(rows, T, D, D), gravity=g.reshape(rows, T, D), coriolis=c.reshape(rows, T, D),
                torque=tau.reshape(rows, T, D))


def effort64(traj, frames, axes, bodies, dt):
    """``motion_effort``: sum_(t < T - 1) |M(q_t) u_t|^2 with the finite differences of the float32 trajectory formed in float32 as
    torch forms them -> (effort [rows], controls [rows, T - 1, D])"""
    t = np.asarray(traj, dtype=F32)
    v = np.zeros_like(t)
    v[:, 1:] = (t[:, 1:] - t[:, :-1]) / F32(dt)
    u = (v[:, 1:] - v[:, :-1]) / F32(dt)
    rows, T, D = t.shape
    M = mass_matrix64(t[:, :-1].reshape(-1, D), frames, axes, bodies)
    tau = np.einsum("nij,nj->ni", M, u.reshape(-1, D).astype(np.float64)).reshape(rows, T - 1, D)
    return (tau * tau).sum((1, 2)), u


# ------------------------------------------------------------------------------------------------ the restatement, float32
def world32(q, frames, axes, bodies):
    """THE WALK WITH BODIES of csrc/avae_dynamics.h: plain float32 products and sums in its order; sine and cosine are the
    double-precision ones of the float angle, rounded once -> (o, z, r [n, D, 3], I [n, D, 6]: xx, xy, xz, yy, yz, zz)"""
    q = np.asarray(q, dtype=F32)
    F, A, B = (np.asarray(x, dtype=F32) for x in (frames, axes, bodies))
    n, D = q.shape
    R = np.broadcast_to(np.eye(3, dtype=F32), (n, 3, 3)).copy()
    p = np.zeros((n, 3), dtype=F32)
    o, z, r = (np.empty((n, D, 3), dtype=F32) for _ in range(3))
    tens = np.empty((n, D, 6), dtype=F32)
    for j in range(D):
        p, R = _frame32(F[j], p, R)
        ax, ay, az = A[j]
        s = np.sin(q[:, j].astype(np.float64)).astype(F32)[:, None]
        c = np.cos(q[:, j].astype(np.float64)).astype(F32)[:, None]
        r0, r1, r2 = R[:, :, 0], R[:, :, 1], R[:, :, 2]
        dot = (r0 * ax + r1 * ay) + r2 * az
        o[:, j], z[:, j] = p, dot
        x0, x1, x2 = r1 * az - r2 * ay, r2 * ax - r0 * az, r0 * ay - r1 * ax
        k = dot * (F32(1.0) - c)
        R = np.stack([(r0 * c + x0 * s) + ax * k, (r1 * c + x1 * s) + ay * k, (r2 * c + x2 * s) + az * k], axis=-1)
        b = B[j]
        L = _tensor(b[4:])
        r[:, j] = (R[:, :, 0] * b[1] + R[:, :, 1] * b[2]) + R[:, :, 2] * b[3]
        Am = (R[:, :, 0, None] * L[0] + R[:, :, 1, None] * L[1]) + R[:, :, 2, None] * L[2]                 # [n, i, k]
        slot = 0
        for i in range(3):
            for kk in range(i, 3):
                tens[:, j, slot] = (Am[:, i, 0] * R[:, kk, 0] + Am[:, i, 1] * R[:, kk, 1]) + Am[:, i, 2] * R[:, kk, 2]
                slot += 1
    assert o.dtype == F32 and r.dtype == F32 and tens.dtype == F32
    return o, z, r, tens


def _times32(t, x):
    """(I x)[i] = (I[i][0] x0 + I[i][1] x1) + I[i][2] x2 with I given as its six numbers [n, 6]"""
    xx, xy, xz, yy, yz, zz = (t[:, i] for i in range(6))
    return np.stack([(xx * x[:, 0] + xy * x[:, 1]) + xz * x[:, 2], (xy * x[:, 0] + yy * x[:, 1]) + yz * x[:, 2],
                     (xz * x[:, 0] + yz * x[:, 1]) + zz * x[:, 2]], axis=-1)


def pass32(world, mass, v, a, g, has_v):
    """THE PASS of csrc/avae_dynamics.h -> tau [n, D] float32"""
    o, z, r, tens = world
    n, D = a.shape
    w, dw = np.zeros((n, 3), dtype=F32), np.zeros((n, 3), dtype=F32)
    ao = np.broadcast_to(np.asarray(g, dtype=F32), (n, 3)).copy()
    Fs, Ns = [], []
    for j in range(D):
        if j > 0:
            d = o[:, j] - o[:, j - 1]
            ao = ao + _cross(dw, d)
            if has_v:
                ao = ao + _cross(w, _cross(w, d))
        t1 = dw + z[:, j] * a[:, j, None]
        if has_v:
            t1 = t1 + _cross(w, z[:, j]) * v[:, j, None]
            w = w + z[:, j] * v[:, j, None]
        dw = t1
        ac = ao + _cross(dw, r[:, j])
        if has_v:
            ac = ac + _cross(w, _cross(w, r[:, j]))
        Fs.append(mass[j] * ac)
        t1 = _times32(tens[:, j], dw)
        if has_v:
            t1 = t1 + _cross(w, _times32(tens[:, j], w))
        Ns.append(t1)
    tau = np.empty((n, D), dtype=F32)
    nn = f = None
    for j in range(D - 1, -1, -1):
        t1 = _cross(r[:, j], Fs[j])
        if j == D - 1:
            nn, f = Ns[j] + t1, Fs[j]
        else:
            t2 = _cross(o[:, j + 1] - o[:, j], f)
            nn = ((Ns[j] + t1) + nn) + t2
            f = f + Fs[j]
        tau[:, j] = (z[:, j, 0] * nn[:, 0] + z[:, j, 1] * nn[:, 1]) + z[:, j, 2] * nn[:, 2]
    assert tau.dtype == F32 and nn.dtype == F32 and f.dtype == F32
    return tau


def dynamics32(traj, vel, acc, frames, axes, bodies, gravity=GRAVITY):
    """THE OUTPUTS of csrc/avae_dynamics.h restated -> the dict of ``dynamics64`` in float32"""
    traj = np.asarray(traj, dtype=F32)
    rows, T, D = traj.shape
    q = traj.reshape(-1, D)
    zero = np.zeros_like(q)
    v = zero if vel is None else np.asarray(vel, dtype=F32).reshape(-1, D)
    a = zero if acc is None else np.asarray(acc, dtype=F32).reshape(-1, D)
    bad = ~(np.isfinite(q).all(1) & np.isfinite(v).all(1) & np.isfinite(a).all(1))
    with np.errstate(all="ignore"):
        world = world32(q, frames, axes, bodies)
        mass = np.asarray(bodies, dtype=F32)[:, 0]
        g = -np.asarray(gravity, dtype=F32)
        none = np.zeros(3, dtype=F32)
        out = dict(gravity=pass32(world, mass, zero, zero, g, False), coriolis=pass32(world, mass, v, zero, none, vel is not None),
                   torque=pass32(world, mass, v, a, g, vel is not None))
        M = np.empty((q.shape[0], D, D), dtype=F32)
        for j in range(D):
            unit = zero.copy()
            unit[:, j] = 1.0
            t = pass32(world, mass, zero, unit, none, False)
            M[:, :j + 1, j] = t[:, :j + 1]
            M[:, j, :j] = t[:, :j]
    out["inertia"] = M
    for k in out:
        out[k][bad] = np.nan
    return dict(inertia=M.reshape(rows, T, D, D), **{k: out[k].reshape(rows, T, D) for k in ("gravity", "coriolis", "torque")})


# ------------------------------------------------------------------------------------------------ cases
def fixture_chain():
    from vae_assoc_amd.kinematics import KinematicChain
    return KinematicChain(fixture()["joints"])


def random_joints(D, seed, massless=()):
    """D revolute joints with arbitrary unit axes and origins and random positive-definite inertias about rotated inertial origins, a
    fixed joint in front, between some and behind (each carrying a part of a body); the bodies ``massless`` have mass 0"""
    rng = np.random.default_rng([seed, D, 32])

    def inertial(k):
        if k in massless:
            return dict(mass=0.0)
        m = rng.uniform(0.2, 3.0)
        a = rng.standard_normal((3, 3))
        t = m * 0.01 * (a @ a.T + 0.5 * np.eye(3))
        return dict(mass=m, com=rng.uniform(-0.1, 0.1, 3), com_rpy=rng.uniform(-3, 3, 3),
                    inertia=[t[0, 0], t[0, 1], t[0, 2], t[1, 1], t[1, 2], t[2, 2]])
    out = [dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3))]
    for d in range(D):
        a = rng.standard_normal(3)
        out.append(dict(type="revolute", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3), axis=a / np.linalg.norm(a),
                        lower=-3.0, upper=3.0, effort=50.0, velocity=4.0, **inertial(d)))
        if d % 3 == 1:
            out.append(dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3), **inertial(d)))
    out.append(dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3), **inertial(D - 1)))
    return out


def fixture_joints(D):
    """the fixture's joints with the first D revolute ones moving and the others held at angle 0 (fixed)"""
    out, d = [], 0
    for j in fixture()["joints"]:
        j = dict(j)
        if j["type"] == "revolute":
            d += 1
            if d > D:
                j["type"] = "fixed"
        out.append(j)
    return out


_CACHE = {}


def case(shape, seed=0, massless=()):
    """(rows, T, D) -> dict(chain, frames, axes, bodies (float32), traj, vel, acc [rows, T, D] float32): the fixture arm (its first D
    joints) for D <= 7, a random chain beyond; angles inside the limits, speeds within +-2 rad / s, accelerations within +-10"""
    key = (tuple(shape), seed, tuple(massless))
    if key not in _CACHE:
        from vae_assoc_amd.kinematics import KinematicChain
        rows, T, D = shape
        chain = KinematicChain(fixture_joints(D) if D <= 7 and not massless else random_joints(D, seed, massless))
        rng = np.random.default_rng([seed, rows, T, D, 32])
        lim = chain.limits
        frames, axes = chain.packed()
        _CACHE[key] = dict(chain=chain, frames=frames, axes=axes, bodies=chain.bodies(),
                           traj=rng.uniform(lim[:, 0], lim[:, 1], size=(rows, T, D)).astype(F32),
                           vel=rng.uniform(-2.0, 2.0, size=(rows, T, D)).astype(F32),
                           acc=rng.uniform(-10.0, 10.0, size=(rows, T, D)).astype(F32))
    return _CACHE[key]


def refs(c, vel=True, acc=True, gravity=GRAVITY):
    """-> (definition, restatement) of a case with or without its speeds and accelerations, computed once"""
    key = ("refs", id(c), vel, acc, tuple(gravity))
    if key not in _CACHE:
        args = (c["traj"], c["vel"] if vel else None, c["acc"] if acc else None, c["frames"], c["axes"], c["bodies"], gravity)
        _CACHE[key] = (dynamics64(*args), dynamics32(*args), c)
    return _CACHE[key][:2]


def rel_err(got, ref):
    """worst |err| / (|ref| + 1); NaN must sit where NaN sits"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    return float((np.abs(got - ref)[ok] / (np.abs(ref)[ok] + 1.0)).max()) if ok.any() else 0.0
