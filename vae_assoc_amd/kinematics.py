"""The host side of pen-path kinematics and stroke rendering (avae_motion_fk / avae_stroke_render in include/avae.h, DESIGN.md
section 24): a serial chain of URDF-style joints packed into the matrices the device call takes, and the canvas a pen path is
drawn on.

The reference turns a joint trajectory into a pen path with one PyKDL call per time point (``derive_cartesian_trajectory``,
baxter_vae_assoc_writer.py:448-449) and draws it with matplotlib, crops it to the ink and shrinks it to 28 x 28 with OpenCV
(utils.py:240-257).  ``KinematicChain`` is the first half, ``StrokeCanvas`` the framing of the second.  Everything here is NumPy
float64 and needs no GPU."""
import numpy as np

from ._capi import MOTION_MAX_DOF as MAX_DOF, MOTION_MAX_POINTS as MAX_POINTS, RENDER_MAX_SIZE as MAX_SIZE
from ._capi import RENDER_SUPERSAMPLES as SUPERSAMPLES


def _vec3(a, name, unit=False):
    try:
        v = np.array(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be three numbers, got %r" % (name, a))
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("%s must be three finite numbers, got %r" % (name, a))
    if unit:
        n = np.linalg.norm(v)
        if abs(n - 1.0) > 1e-6:
            raise ValueError("%s must be a unit vector, got %r (norm %.9g)" % (name, a, n))
        v = v / n
    return v


def origin_matrix(xyz, rpy):
    """``Trans(xyz) Rz(yaw) Ry(pitch) Rx(roll)`` as a 4 x 4 matrix (the URDF ``origin`` of a joint)"""
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = xyz
    return m


def axis_rotation(axis, q):
    """Rodrigues' formula: the rotation by ``q`` about the unit vector ``axis``, 3 x 3"""
    a = np.asarray(axis, dtype=np.float64)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.cos(q) * np.eye(3) + np.sin(q) * k + (1.0 - np.cos(q)) * np.outer(a, a)


def _number(x, name, low=None):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) \
            or (low is not None and x < low):
        raise ValueError("%s must be a finite number%s, got %r" % (name, "" if low is None else " >= %g" % low, x))
    return float(x)


def _inertial(j, where):
    """The optional dynamics keys of a joint dict, checked -> dict(mass, com, com_rpy, inertia, effort, velocity): ``mass`` None
    when the child link carries no inertial data (the other three are then None too)"""
    out = dict(mass=None, com=None, com_rpy=None, inertia=None, effort=None, velocity=None)
    for k in ("effort", "velocity"):
        if j.get(k) is not None:
            out[k] = _number(j[k], "%s: %s" % (where, k), 0.0)
    if j.get("mass") is None:
        for k in ("com", "com_rpy", "inertia"):
            if j.get(k) is not None:
                raise ValueError("%s: %s is given without mass" % (where, k))
        return out
    out["mass"] = _number(j["mass"], "%s: mass" % where, 0.0)
    out["com"] = _vec3(j.get("com") if j.get("com") is not None else (0.0, 0.0, 0.0), "%s: com" % where)
    out["com_rpy"] = _vec3(j.get("com_rpy") if j.get("com_rpy") is not None else (0.0, 0.0, 0.0), "%s: com_rpy" % where)
    try:
        t = np.array(j.get("inertia") if j.get("inertia") is not None else [0.0] * 6, dtype=np.float64)
    except (TypeError, ValueError):
        t = np.zeros(0)
    if t.shape != (6,) or not np.isfinite(t).all():
        raise ValueError("%s: inertia must be six finite numbers [ixx, ixy, ixz, iyy, iyz, izz], got %r" % (where, j.get("inertia")))
    out["inertia"] = t
    return out


def _tensor(t):
    """[ixx, ixy, ixz, iyy, iyz, izz] -> the symmetric 3 x 3 matrix"""
    return np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]], dtype=np.float64)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


GRAVITY = (0.0, 0.0, -9.81)


class KinematicChain(object):
    """A serial chain from base to tip.  ``joints`` is a list of dicts: ``type`` 'fixed' or 'revolute', ``xyz`` and ``rpy`` of the
    joint's origin (default zeros), ``axis`` (a unit vector; revolute joints only, default (1, 0, 0) as in URDF), and optionally
    ``name``, ``lower`` and ``upper``.  The pose is ``T(q) = prod_j O_j Rot(axis_j, q_j)`` in chain order, with no rotation for a
    fixed joint and ``O_j = Trans(xyz) Rz(yaw) Ry(pitch) Rx(roll)``; the pen tip is ``T[:3, 3]``.

    Rigid-body dynamics need more, all optional and all about the joint's *child link*: ``mass`` (>= 0),
    ``com`` and ``com_rpy`` (xyz and rpy of the inertial origin in the link frame, default zeros), ``inertia`` (``[ixx, ixy, ixz,
    iyy, iyz, izz]`` about the centre of mass, in the inertial frame, default zeros) and the joint's ``effort`` and ``velocity``
    limits.  A chain without them is a kinematic chain only (``has_inertia`` is False)."""

    def __init__(self, joints):
        self.joints = []
        for i, j in enumerate(joints):
            if not isinstance(j, dict):
                raise ValueError("joints[%d] must be a dict, got %r" % (i, type(j).__name__))
            kind = j.get("type")
            if kind not in ("fixed", "revolute"):
                raise ValueError("joints[%d]: type must be 'fixed' or 'revolute', got %r" % (i, kind))
            xyz = _vec3(j.get("xyz") if j.get("xyz") is not None else (0.0, 0.0, 0.0), "joints[%d]: xyz" % i)
            rpy = _vec3(j.get("rpy") if j.get("rpy") is not None else (0.0, 0.0, 0.0), "joints[%d]: rpy" % i)
            axis = None
            if kind == "revolute":
                axis = _vec3(j.get("axis") if j.get("axis") is not None else (1.0, 0.0, 0.0), "joints[%d]: axis" % i, unit=True)
            self.joints.append(dict(name=j.get("name"), type=kind, xyz=xyz, rpy=rpy, axis=axis, lower=j.get("lower"),
                                    upper=j.get("upper"), **_inertial(j, "joints[%d]" % i)))
        self.n_dof = sum(1 for j in self.joints if j["type"] == "revolute")
        if not 1 <= self.n_dof <= MAX_DOF:
            raise ValueError("the chain must hold 1 to %d revolute joints (n_dof), got %d" % (MAX_DOF, self.n_dof))
        self._cache = {}

    @classmethod
    def from_urdf(cls, path, base, tip):
        """The chain from link ``base`` to link ``tip`` of a URDF file (or of a string that holds one): walks the parent links
        from the tip.  ``continuous`` joints count as revolute; any other moving joint is refused.  Each joint also takes the
        ``<inertial>`` of its child link (mass, origin, inertia) and ``effort`` / ``velocity`` of its ``<limit>``.  Only the
        links on the way from base to tip count, as in a KDL chain: side branches (cameras, gripper fingers, the other arm) are
        ignored, and so is their mass."""
        import os
        import xml.etree.ElementTree as ET
        text = str(path)
        root = ET.fromstring(text) if text.lstrip().startswith("<") else ET.parse(os.fspath(path)).getroot()
        by_child, links = {}, {l.get("name"): l for l in root.iter("link")}
        for j in root.iter("joint"):
            child, parent = j.find("child"), j.find("parent")
            if child is not None and parent is not None:
                by_child[child.get("link")] = j

        def numbers(el, attr, default):
            s = None if el is None else el.get(attr)
            return default if s is None else [float(x) for x in s.split()]
        joints, link = [], tip
        while link != base:
            j = by_child.get(link)
            if j is None:
                raise ValueError("no joint chain leads from link %r to link %r" % (base, tip))
            kind = {"continuous": "revolute"}.get(j.get("type"), j.get("type"))
            if kind not in ("fixed", "revolute"):
                raise ValueError("joint %r is %r: only fixed and revolute joints are supported" % (j.get("name"), j.get("type")))
            lim = j.find("limit")
            dyn = {k: None if lim is None or lim.get(k) is None else float(lim.get(k)) for k in ("effort", "velocity")}
            inert = None if links.get(link) is None else links[link].find("inertial")
            if inert is not None and inert.find("mass") is not None:
                t = inert.find("inertia")
                dyn.update(mass=float(inert.find("mass").get("value")), com=numbers(inert.find("origin"), "xyz", [0.0, 0.0, 0.0]),
                           com_rpy=numbers(inert.find("origin"), "rpy", [0.0, 0.0, 0.0]),
                           inertia=[0.0 if t is None or t.get(k) is None else float(t.get(k))
                                    for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")])
            joints.append(dict(name=j.get("name"), type=kind, xyz=numbers(j.find("origin"), "xyz", [0.0, 0.0, 0.0]),
                               rpy=numbers(j.find("origin"), "rpy", [0.0, 0.0, 0.0]),
                               axis=numbers(j.find("axis"), "xyz", [1.0, 0.0, 0.0]) if kind == "revolute" else None,
                               lower=None if lim is None or lim.get("lower") is None else float(lim.get("lower")),
                               upper=None if lim is None or lim.get("upper") is None else float(lim.get("upper")), **dyn))
            link = j.find("parent").get("link")
        return cls(joints[::-1])

    @property
    def limits(self):
        """[n_dof, 2] (lower, upper) of the revolute joints, or None when one of them has no limits"""
        rev = [j for j in self.joints if j["type"] == "revolute"]
        if any(j["lower"] is None or j["upper"] is None for j in rev):
            return None
        return np.array([[j["lower"], j["upper"]] for j in rev], dtype=np.float64)

    def packed(self, dtype=np.float32):
        """-> (``frames [n_dof + 1, 3, 4]``, ``axes [n_dof, 3]``): frame j < n_dof is the product of the fixed origins since the
        previous revolute joint and the origin of revolute joint j, frame n_dof the fixed origins behind the last revolute joint
        (the identity if there are none), so that ``T(q) = F_0 Rot_0 F_1 ... Rot_{D-1} F_D``.  The products are formed in float64
        and rounded once to ``dtype`` (float32: what the device call takes)."""
        if "packed" not in self._cache:
            frames, axes, run = [], [], np.eye(4)
            for j in self.joints:
                run = run @ origin_matrix(j["xyz"], j["rpy"])
                if j["type"] == "revolute":
                    frames.append(run[:3])
                    axes.append(j["axis"])
                    run = np.eye(4)
            frames.append(run[:3])
            self._cache["packed"] = (np.array(frames, dtype=np.float64), np.array(axes, dtype=np.float64))
        f, a = self._cache["packed"]
        return np.ascontiguousarray(f, dtype=dtype).copy(), np.ascontiguousarray(a, dtype=dtype).copy()

    def forward(self, q):
        """Joint angles ``[..., n_dof]`` -> pen tips ``[..., 3]``, float64, joint by joint as the definition is written"""
        q = np.asarray(q, dtype=np.float64)
        if q.shape[-1:] != (self.n_dof,):
            raise ValueError("q must be [..., %d], got %s" % (self.n_dof, q.shape))
        flat = q.reshape(-1, self.n_dof)
        out = np.empty((flat.shape[0], 3))
        origins = [origin_matrix(j["xyz"], j["rpy"]) for j in self.joints]
        for i, row in enumerate(flat):
            m, d = np.eye(4), 0
            for j, o in zip(self.joints, origins):
                m = m @ o
                if j["type"] == "revolute":
                    r = np.eye(4)
                    r[:3, :3] = axis_rotation(j["axis"], row[d])
                    m = m @ r
                    d += 1
            out[i] = m[:3, 3]
        return out.reshape(q.shape[:-1] + (3,))

    def _walk(self, q):
        """The packed chain walked from base to tip at ``q [n, n_dof]`` (float64) -> (tip position ``[n, 3]``, tip rotation
        ``[n, 3, 3]``, joint origins ``o [n, n_dof, 3]``, joint axes in the base frame ``z [n, n_dof, 3]``): ``o_j`` and
        ``z_j = R_j axis_j`` are taken after frame j, ahead of joint j's own rotation."""
        frames, axes = self.packed(np.float64)
        n = q.shape[0]
        R = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
        p = np.zeros((n, 3))
        o, z = np.empty((n, self.n_dof, 3)), np.empty((n, self.n_dof, 3))
        for j in range(self.n_dof):
            p = p + R @ frames[j, :, 3]
            R = R @ frames[j, :, :3]
            o[:, j], z[:, j] = p, R @ axes[j]
            a = axes[j]
            K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
            c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
            R = R @ (c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a))
        p = p + R @ frames[self.n_dof, :, 3]
        R = R @ frames[self.n_dof, :, :3]
        return p, R, o, z

    def _angles(self, q):
        q = np.asarray(q, dtype=np.float64)
        if q.shape[-1:] != (self.n_dof,):
            raise ValueError("q must be [..., %d], got %s" % (self.n_dof, q.shape))
        return q, q.reshape(-1, self.n_dof)

    def pose(self, q):
        """Joint angles ``[..., n_dof]`` -> (pen tip ``[..., 3]``, its rotation ``[..., 3, 3]``), float64: ``T(q)[:3, 3]`` and
        ``T(q)[:3, :3]``.  The tip is ``forward(q)`` up to rounding (the packed frames are products formed ahead)."""
        q, flat = self._angles(q)
        p, R, _, _ = self._walk(flat)
        return p.reshape(q.shape[:-1] + (3,)), R.reshape(q.shape[:-1] + (3, 3))

    def jacobian(self, q):
        """Joint angles ``[..., n_dof]`` -> the geometric Jacobian ``[..., 6, n_dof]``, float64: column j holds
        ``z_j x (tip - o_j)`` over ``z_j``, the tip's linear and angular velocity per unit speed of joint j, in the base frame."""
        q, flat = self._angles(q)
        p, _, o, z = self._walk(flat)
        J = np.concatenate([np.cross(z, p[:, None, :] - o), z], axis=-1)          # [n, D, 6]
        return np.swapaxes(J, -1, -2).reshape(q.shape[:-1] + (6, self.n_dof))

    # ------------------------------------------------------------------ rigid-body dynamics
    def _revolute_limits(self, key):
        rev = [j for j in self.joints if j["type"] == "revolute"]
        return None if any(j[key] is None for j in rev) else np.array([j[key] for j in rev], dtype=np.float64)

    @property
    def effort_limits(self):
        """[n_dof] torque limits of the revolute joints (N m), or None when one of them has none"""
        return self._revolute_limits("effort")

    @property
    def velocity_limits(self):
        """[n_dof] speed limits of the revolute joints (rad / s), or None when one of them has none"""
        return self._revolute_limits("velocity")

    def _moving(self):
        first = next(i for i, j in enumerate(self.joints) if j["type"] == "revolute")
        return self.joints[first:]

    @property
    def has_inertia(self):
        """True when every link from the first revolute joint to the tip carries inertial data (``bodies`` then works)"""
        return all(j["mass"] is not None for j in self._moving())

    def bodies(self, dtype=np.float32):
        """-> ``[n_dof, 10]``: per moving body k ``(m, c_x, c_y, c_z, Ixx, Ixy, Ixz, Iyy, Iyz, Izz)`` -- mass, centre of mass and
        inertia about it -- in the frame ``packed()``'s walk has right after revolute joint k's own rotation.  Body k is the
        child link of revolute joint k and every link fixed to it, up to the next revolute joint or the tip: each part is carried
        through the fixed origins and its inertial origin, masses add, the centre of mass is their mass-weighted mean and the
        inertias are rotated and moved to it by the parallel-axis theorem.  Links ahead of the first revolute joint do not move
        and are dropped; a body of total mass 0 has ``c = 0`` and ``I = 0``.  Formed in float64 and rounded once to ``dtype``."""
        if "bodies" not in self._cache:
            parts, run = [], np.eye(4)
            for i, j in enumerate(self.joints):
                if j["type"] == "revolute":
                    parts.append([])
                    run = np.eye(4)
                elif parts:
                    run = run @ origin_matrix(j["xyz"], j["rpy"])
                if not parts:
                    continue
                if j["mass"] is None:
                    raise ValueError("the child link of joint %r (joints[%d]) has no inertial data: give it mass, com, com_rpy and "
                                     "inertia" % (j["name"], i))
                t = run @ origin_matrix(j["com"], j["com_rpy"])
                parts[-1].append((j["mass"], t[:3, 3], t[:3, :3] @ _tensor(j["inertia"]) @ t[:3, :3].T))
            out = np.zeros((self.n_dof, 10))
            for k, body in enumerate(parts):
                m = sum(p[0] for p in body)
                if not m > 0.0:
                    continue
                c = sum(p[0] * p[1] for p in body) / m
                tens = np.zeros((3, 3))
                for pm, pc, pi in body:
                    d = pc - c
                    tens += pi + pm * (np.dot(d, d) * np.eye(3) - np.outer(d, d))
                out[k] = [m, c[0], c[1], c[2], tens[0, 0], tens[0, 1], tens[0, 2], tens[1, 1], tens[1, 2], tens[2, 2]]
            self._cache["bodies"] = out
        return np.ascontiguousarray(self._cache["bodies"], dtype=dtype).copy()

    def _world_bodies(self, q):
        """``_walk`` with the bodies carried along, at ``q [n, n_dof]`` (float64) -> (``o``, ``z [n, n_dof, 3]`` as ``_walk``
        gives them, ``r [n, n_dof, 3]``: the centres of mass relative to ``o`` in the base frame, ``r_k = R_k^+ c_k`` with
        ``R_k^+`` the rotation right after joint k's own, ``I [n, n_dof, 3, 3]``: ``R_k^+ I_k R_k^+T``, and the masses)"""
        frames, axes = self.packed(np.float64)
        b = self.bodies(np.float64)
        n = q.shape[0]
        R = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
        p = np.zeros((n, 3))
        o, z, r = (np.empty((n, self.n_dof, 3)) for _ in range(3))
        tens = np.empty((n, self.n_dof, 3, 3))
        for j in range(self.n_dof):
            p = p + R @ frames[j, :, 3]
            R = R @ frames[j, :, :3]
            o[:, j], z[:, j] = p, R @ axes[j]
            a = axes[j]
            K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
            c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
            R = R @ (c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a))
            r[:, j] = R @ b[j, 1:4]
            tens[:, j] = R @ _tensor(b[j, 4:]) @ np.swapaxes(R, -1, -2)
        return o, z, r, tens, b[:, 0]

    @staticmethod
    def _newton_euler(o, z, r, tens, m, v, a, ao):
        """Recursive Newton-Euler in base-frame coordinates (avae_dynamics.h) -> joint torques ``[n, D]``: outwards the angular
        velocity ``w``, its rate ``dw`` and the joint origins' accelerations ``ao`` (``-gravity`` ahead of the first joint), the
        force and moment each body needs; inwards their sums about each joint's origin, projected on its axis"""
        n, D = v.shape
        w, dw = np.zeros((n, 3)), np.zeros((n, 3))
        F, N = np.empty((n, D, 3)), np.empty((n, D, 3))
        for j in range(D):
            if j:
                d = o[:, j] - o[:, j - 1]
                ao = ao + _cross(dw, d) + _cross(w, _cross(w, d))
            dw = dw + z[:, j] * a[:, j, None] + _cross(w, z[:, j]) * v[:, j, None]
            w = w + z[:, j] * v[:, j, None]
            ac = ao + _cross(dw, r[:, j]) + _cross(w, _cross(w, r[:, j]))
            F[:, j] = m[j] * ac
            Iw = np.einsum("nij,nj->ni", tens[:, j], w)
            N[:, j] = np.einsum("nij,nj->ni", tens[:, j], dw) + _cross(w, Iw)
        tau = np.empty((n, D))
        nn, f = np.zeros((n, 3)), np.zeros((n, 3))
        for j in range(D - 1, -1, -1):
            nn = N[:, j] + _cross(r[:, j], F[:, j]) + nn
            if j + 1 < D:
                nn = nn + _cross(o[:, j + 1] - o[:, j], f)
            f = f + F[:, j]
            tau[:, j] = np.einsum("ni,ni->n", z[:, j], nn)
        return tau

    def mass_matrix(self, q):
        """Joint angles ``[..., n_dof]`` -> the joint-space inertia ``M(q) [..., n_dof, n_dof]``, float64: column j is the torque
        a unit acceleration of joint j asks for at rest and without gravity; the upper triangle is computed and mirrored.
        ``motion_track(effort=chain.mass_matrix(seed))`` prices the controls by ``|M(seed) u|^2``, the reference's effort term
        at one pose."""
        q, flat = self._angles(q)
        D, n = self.n_dof, flat.shape[0]
        world = self._world_bodies(flat)
        M, zero = np.empty((n, D, D)), np.zeros((n, D))
        for j in range(D):
            unit = zero.copy()
            unit[:, j] = 1.0
            tau = self._newton_euler(*world, zero, unit, np.zeros((n, 3)))
            M[:, :j + 1, j] = tau[:, :j + 1]
            M[:, j, :j] = tau[:, :j]
        return M.reshape(q.shape[:-1] + (D, D))

    def gravity_torque(self, q, gravity=GRAVITY):
        """Joint angles ``[..., n_dof]`` -> the torques ``[..., n_dof]`` that hold the arm still against ``gravity`` (the
        acceleration of free fall in the base frame, m / s^2): ``dV/dq`` of the potential energy, float64"""
        return self.inverse_dynamics(q, gravity=gravity)

    def inverse_dynamics(self, q, v=None, a=None, gravity=GRAVITY):
        """Joint angles, speeds and accelerations ``[..., n_dof]`` (None: zeros) -> the joint torques ``M(q) a + c(q, v) + g(q)``
        ``[..., n_dof]``, float64.  ``gravity=(0, 0, 0)`` and ``v=None`` leave ``M(q) a``."""
        q, flat = self._angles(q)
        g = _vec3(gravity, "gravity")
        rest = []
        for x, name in ((v, "v"), (a, "a")):
            x = np.zeros_like(q) if x is None else np.asarray(x, dtype=np.float64)
            if x.shape != q.shape:
                raise ValueError("%s must have q's shape %s, got %s" % (name, q.shape, x.shape))
            rest.append(x.reshape(-1, self.n_dof))
        tau = self._newton_euler(*self._world_bodies(flat), rest[0], rest[1], np.broadcast_to(-g, (flat.shape[0], 3)))
        return tau.reshape(q.shape)


class StrokeCanvas(object):
    """How a pen path becomes a picture.  ``plane [3, 3]`` holds the rows u (image x, to the right), v (image y, upwards) and n (the
    height above the paper); by default u = -y / scale, v = x / scale, n = z, the reference's writing plane with its 0.03 m per
    unit (baxter_writer.py:30).  ``half_width`` is half the line's width in plane units (0.0625: a 12 pt line at 100 dpi on a
    400 px canvas of 3 units), ``size`` the picture's side in pixels, ``supersample`` the samples per pixel side (1, 2, 4 or 8)
    and ``margin`` the border around the ink as a share of its longer side (0.6, utils.py:240-257)."""

    def __init__(self, scale=0.03, half_width=0.0625, size=28, supersample=4, margin=0.6, plane=None):
        def number(x, name):
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
                raise ValueError("%s must be a finite number, got %r" % (name, x))
            return float(x)
        self.scale = number(scale, "scale")
        if not self.scale > 0.0:
            raise ValueError("scale must be > 0, got %r" % (scale,))
        self.half_width = float(np.float32(number(half_width, "half_width")))
        if not self.half_width > 0.0:
            raise ValueError("half_width must be > 0, got %r" % (half_width,))
        self.margin = float(np.float32(number(margin, "margin")))
        if not self.margin >= 0.0:
            raise ValueError("margin must be >= 0, got %r" % (margin,))
        if isinstance(size, (bool, np.bool_)) or not isinstance(size, (int, np.integer)) or not 1 <= size <= MAX_SIZE:
            raise ValueError("size must be an integer in [1, %d], got %r" % (MAX_SIZE, size))
        self.size = int(size)
        if isinstance(supersample, (bool, np.bool_)) or supersample not in SUPERSAMPLES:
            raise ValueError("supersample must be one of %s, got %r" % (SUPERSAMPLES, supersample))
        self.supersample = int(supersample)
        if plane is None:
            plane = np.array([[0.0, -1.0 / self.scale, 0.0], [1.0 / self.scale, 0.0, 0.0], [0.0, 0.0, 1.0]])
        plane = np.array(plane, dtype=np.float64)
        if plane.shape != (3, 3) or not np.isfinite(plane).all():
            raise ValueError("plane must be a finite [3, 3] array (rows u, v, n), got shape %s" % (plane.shape,))
        self.plane = plane
        self._cache = {}

    @property
    def n_pixels(self):
        return self.size * self.size

    def lift(self, strokes, center, height=0.0):
        """Strokes in plane units ``[..., 2]`` (u to the right, v upwards) -> the pen path ``[..., 3]`` that draws them around
        ``center`` at ``height`` above the paper: ``center + P^-1 (u, v, height)`` with ``P = plane``, the inverse of the
        projection ``render_strokes`` applies.  With the default plane and the reference's image-style stroke coordinates,
        ``(u, v) = (char_x, -char_y)`` gives ``generate_spatial_trajectory`` after the flip of baxter_writer.py:156.  NumPy
        float64."""
        s = np.asarray(strokes, dtype=np.float64)
        if s.shape[-1:] != (2,):
            raise ValueError("strokes must be [..., 2], got %s" % (s.shape,))
        c = _vec3(center, "center")
        if isinstance(height, (bool, np.bool_)) or not isinstance(height, (int, float, np.integer, np.floating)) or not np.isfinite(height):
            raise ValueError("height must be a finite number, got %r" % (height,))
        try:
            inv = np.linalg.inv(self.plane)
        except np.linalg.LinAlgError:
            raise ValueError("plane is singular: its rows u, v, n do not span the space")
        return c + s @ inv[:, :2].T + float(height) * inv[:, 2]
