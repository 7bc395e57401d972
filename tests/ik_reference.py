"""The definition of pose, Jacobian and inverse kinematics (avae_motion_pose / avae_motion_ik, include/avae.h)
in NumPy float64, and next to it a float32 restatement of the kernels: the same operations in the order csrc/avae_ik.h writes down
(sin and cos are NumPy's float32 ones).  The restatement's distance from the definition on a set of inputs is what the GPU tests
build their bounds from (4x, the rule of test_gpu_motion.py).

Both take the packed constants the device call takes (``KinematicChain.packed()``: the float32 values, widened for the
definition), so that the three of them start from the same bits."""
import numpy as np

F32 = np.float32
STATUS_OK, STATUS_CAP, STATUS_PIVOT, STATUS_NONFINITE = 0, 1, 2, 3     # 2: the solve failed (pivot not > 0 or a non-finite step)


# ------------------------------------------------------------------------------------------------ the walk
def walk64(q, frames, axes):
    """q [n, D] -> (p [n, 3], R [n, 3, 3], o [n, D, 3], z [n, D, 3]) in float64: T(q) = F_0 Rot_0 F_1 ... Rot_{D-1} F_D from base to
    tip as matrix products, o_j and z_j = R_j axis_j taken after F_j"""
    q = np.asarray(q, dtype=np.float64)
    F, A = np.asarray(frames, dtype=np.float64), np.asarray(axes, dtype=np.float64)
    n, D = q.shape
    R = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    p = np.zeros((n, 3))
    o, z = np.empty((n, D, 3)), np.empty((n, D, 3))
    for j in range(D):
        p = p + R @ F[j, :, 3]
        R = R @ F[j, :, :3]
        o[:, j], z[:, j] = p, R @ A[j]
        a = A[j]
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
        R = R @ (c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a))
    p = p + R @ F[D, :, 3]
    R = R @ F[D, :, :3]
    return p, R, o, z


def _frame32(f, p, R):
    """apply_frame of avae_ik.hip on p [n, 3] and R [n, 3, 3] (the three rows r of R at once) -> (p, R)"""
    r0, r1, r2 = R[:, :, 0], R[:, :, 1], R[:, :, 2]
    p = ((r0 * f[0, 3] + r1 * f[1, 3]) + r2 * f[2, 3]) + p
    R = (r0[:, :, None] * f[0, :3] + r1[:, :, None] * f[1, :3]) + r2[:, :, None] * f[2, :3]
    return p, R


def walk32(q, frames, axes):
    """THE WALK of csrc/avae_ik.h: plain float32 products and sums in its order"""
    q = np.asarray(q, dtype=F32)
    F, A = np.asarray(frames, dtype=F32), np.asarray(axes, dtype=F32)
    n, D = q.shape
    R = np.broadcast_to(np.eye(3, dtype=F32), (n, 3, 3)).copy()
    p = np.zeros((n, 3), dtype=F32)
    o, z = np.empty((n, D, 3), dtype=F32), np.empty((n, D, 3), dtype=F32)
    for j in range(D):
        p, R = _frame32(F[j], p, R)
        ax, ay, az = A[j]
        s, c = np.sin(q[:, j])[:, None], np.cos(q[:, j])[:, None]
        r0, r1, r2 = R[:, :, 0], R[:, :, 1], R[:, :, 2]
        dot = (r0 * ax + r1 * ay) + r2 * az
        o[:, j], z[:, j] = p, dot
        x0, x1, x2 = r1 * az - r2 * ay, r2 * ax - r0 * az, r0 * ay - r1 * ax
        k = dot * (F32(1.0) - c)
        R = np.stack([(r0 * c + x0 * s) + ax * k, (r1 * c + x1 * s) + ay * k, (r2 * c + x2 * s) + az * k], axis=-1)
    p, R = _frame32(F[D], p, R)
    assert p.dtype == F32 and R.dtype == F32
    return p, R, o, z


def _cross(a, b):
    """a x b on [..., 3] arrays, two products and a difference per component (no wider intermediate)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _jacobian(p, o, z):
    """[n, 6, D]: J_v[:, j] = z_j x (p - o_j) over J_w[:, j] = z_j"""
    return np.swapaxes(np.concatenate([_cross(z, p[:, None, :] - o), z], axis=-1), 1, 2)


def pose(traj, frames, axes, dt=np.float64):
    """[..., D] angles -> dict(position [..., 3], rotation [..., 3, 3], jacobian [..., 6, D]) in ``dt`` (float64: the definition,
    float32: the restatement)"""
    q = np.asarray(traj, dtype=dt)
    D = q.shape[-1]
    p, R, o, z = (walk64 if dt == np.float64 else walk32)(q.reshape(-1, D), frames, axes)
    J = _jacobian(p, o, z)
    assert J.dtype == dt
    lead = q.shape[:-1]
    return dict(position=p.reshape(lead + (3,)), rotation=R.reshape(lead + (3, 3)), jacobian=J.reshape(lead + (6, D)))


# ------------------------------------------------------------------------------------------------ the solver
def _norm3(e):
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def fmaxf(a, b):
    """C's fmaxf, elementwise: a NaN operand is dropped where the other is a number (``np.maximum`` returns the NaN)"""
    return np.fmax(a, b)


def fminf(a, b):
    """C's fminf, elementwise: a NaN operand is dropped where the other is a number (``np.minimum`` returns the NaN)"""
    return np.fmin(a, b)


def _step(J, e, damp2, max_step):
    """One damped least-squares step on [n] problems, every operation in the order of csrc/avae_ik.h and in the dtype of J ->
    (dq [n, D] after the shrink, pivot_ok [n], shrunk [n]).  ``dq`` may hold non-finite values: ``ik`` refuses such a step."""
    n, m, D = J.shape
    M = J[:, :, None, 0] * J[:, None, :, 0]
    for c in range(1, D):
        M = M + J[:, :, None, c] * J[:, None, :, c]
    L = M.copy()
    for i in range(m):
        L[:, i, i] = L[:, i, i] + damp2
    ok = np.ones(n, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for j in range(m):
            s = L[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= s > 0
            d = np.sqrt(s)
            L[:, j, j] = d
            for i in range(j + 1, m):
                v = L[:, i, j].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / d
        y = np.empty_like(e)
        for i in range(m):
            v = e[:, i].copy()
            for k in range(i):
                v = v - L[:, i, k] * y[:, k]
            y[:, i] = v / L[:, i, i]
        for i in range(m - 1, -1, -1):
            v = y[:, i].copy()
            for k in range(m - 1, i, -1):
                v = v - L[:, k, i] * y[:, k]
            y[:, i] = v / L[:, i, i]
        dq = J[:, 0, :] * y[:, 0, None]
        for i in range(1, m):
            dq = dq + J[:, i, :] * y[:, i, None]
        big = np.zeros(n, dtype=J.dtype)
        for c in range(D):                                       # the kernel's fold from 0: fmaxf drops a NaN
            big = fmaxf(big, np.abs(dq[:, c]))
        shrink = big > max_step
        f = max_step / big
        dq = np.where(shrink[:, None], dq * f[:, None], dq)
    assert dq.dtype == J.dtype
    return dq, ok, shrink


@np.errstate(over="ignore", under="ignore", invalid="ignore")    # targets of 1e30 and a damping of 1e-20 are cases, not mistakes
def ik(path, frames, axes, seed, orient=None, limits=None, n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5,
       dt=np.float64, steps=None):
    """avae_motion_ik in ``dt``: path [N, T, 3], seed [N, D], orient None, [3, 3] or [N, 3, 3], limits None or [D, 2] -> dict of
    trajectory [N, T, D], residual, rot_residual [N, T], iterations, status [N, T] (int32).  float64 is the definition; float32
    restates the kernel (the options rounded to float32 first, as the C call takes them, in both).  Status 2 (STATUS_PIVOT) is
    "the solve failed": a pivot that is not > 0, or a step after which an angle would not be finite (after the shrink, before the
    clamp); such a step is not taken, the point keeps its last good q, the residuals at it and the steps taken so far.
    ``steps``: a list that receives, per solver step, dict(t, k, rows, dq [n, D] (after the shrink), shrunk [n], taken [n])."""
    walk = walk64 if dt == np.float64 else walk32
    path, q = np.asarray(path, dtype=dt), np.array(seed, dtype=dt)
    N, T = path.shape[:2]
    D = q.shape[1]
    tol, rot_tol, max_step = dt(F32(tol)), dt(F32(rot_tol)), dt(F32(max_step))
    damp2 = dt(F32(damping)) * dt(F32(damping))
    G = None if orient is None else np.broadcast_to(np.asarray(orient, dtype=dt).reshape(-1, 3, 3), (N, 3, 3))
    lim = None if limits is None else np.asarray(limits, dtype=dt)
    bad_seed = ~np.isfinite(q).all(axis=1)
    traj = np.full((N, T, D), np.nan, dtype=dt)
    res, rres = np.full((N, T), np.nan, dtype=dt), np.full((N, T), np.nan, dtype=dt)
    iters, status = np.zeros((N, T), dtype=np.int32), np.full((N, T), STATUS_NONFINITE, dtype=np.int32)
    half = dt(0.5)
    for t in range(T):
        g = path[:, t]
        bad = bad_seed | ~np.isfinite(g).all(axis=1)
        active = ~bad
        k = 0
        while active.any():
            idx = np.nonzero(active)[0]
            p, R, o, z = walk(q[idx], frames, axes)
            e = g[idx] - p
            res[idx, t] = _norm3(e)
            done = res[idx, t] < tol
            if G is not None:
                ew = _cross(R[:, :, 0], G[idx][:, :, 0])
                for i in (1, 2):
                    ew = ew + _cross(R[:, :, i], G[idx][:, :, i])
                ew = half * ew
                rres[idx, t] = _norm3(ew)
                done &= rres[idx, t] < rot_tol
                e = np.concatenate([e, ew], axis=1)
            iters[idx, t] = k
            cap = ~done & (k == n_iters)
            status[idx[done], t], status[idx[cap], t] = STATUS_OK, STATUS_CAP
            go = ~(done | cap)
            active[idx] = False
            if go.any():
                sub = idx[go]
                J = _jacobian(p[go], o[go], z[go])
                dq, ok, shrunk = _step(J[:, :e.shape[1]], e[go], damp2, max_step)
                x = q[sub] + dq
                ok &= np.isfinite(x).all(axis=1)                 # a step is committed only when every new angle is finite
                status[sub[~ok], t] = STATUS_PIVOT
                if steps is not None:
                    steps.append(dict(t=t, k=k, rows=sub, dq=dq, shrunk=shrunk, taken=ok.copy()))
                x = x[ok]
                if lim is not None:
                    x = fminf(fmaxf(x, lim[:, 0]), lim[:, 1])
                q[sub[ok]] = x
                active[sub[ok]] = True
            k += 1
        traj[~bad, t] = q[~bad]
    assert traj.dtype == dt and res.dtype == dt
    return dict(trajectory=traj, residual=res, rot_residual=rres if G is not None else None, iterations=iters, status=status)
