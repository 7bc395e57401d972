"""The definition of the iLQR joint-trajectory synthesis (avae_motion_track, include/avae.h) in NumPy float64,
and next to it a restatement of the kernel's precision split (csrc/avae_track.h): the point sees the angles rounded to float32, the
walk, the Jacobian, l_q and l_qq are float32 in the kernel's order (``walk32`` below), the stored gains are rounded to
float32; the cost, the value recursion, the Cholesky and the rollout stay float64.  The restatement's distance from the definition
on a set of inputs is what the GPU tests build their bounds from (4x, the rule of test_gpu_motion.py).

The definition is written from the formulas of the issue with dense A and B (``Q_xx = l_xx + A^T V_xx A`` and so on), not from the
kernel's block algebra: the two agree only if that algebra is right.

Both take the packed constants the device call takes (``KinematicChain.packed()``), and the options rounded to float32 where the C
call takes floats (dt, the track weights, R, limit_weight)."""
import numpy as np

import ik_reference as K

F32 = np.float32
STATUS_OK, STATUS_CAP, STATUS_STUCK, STATUS_NONFINITE = 0, 1, 2, 3


def walk32(q, frames, axes):
    """THE WALK of csrc/avae_ik.h as ``ik_reference.walk32`` writes it, with the sines and cosines avae_track.h asks for: the
    double-precision functions of the float angle, rounded once.  Everything else is plain float32 in THE WALK's order."""
    q = np.asarray(q, dtype=F32)
    F, A = np.asarray(frames, dtype=F32), np.asarray(axes, dtype=F32)
    n, D = q.shape
    R = np.broadcast_to(np.eye(3, dtype=F32), (n, 3, 3)).copy()
    p = np.zeros((n, 3), dtype=F32)
    o, z = np.empty((n, D, 3), dtype=F32), np.empty((n, D, 3), dtype=F32)
    for j in range(D):
        p, R = K._frame32(F[j], p, R)
        ax, ay, az = A[j]
        s = np.sin(q[:, j].astype(np.float64)).astype(F32)[:, None]
        c = np.cos(q[:, j].astype(np.float64)).astype(F32)[:, None]
        r0, r1, r2 = R[:, :, 0], R[:, :, 1], R[:, :, 2]
        dot = (r0 * ax + r1 * ay) + r2 * az
        o[:, j], z[:, j] = p, dot
        x0, x1, x2 = r1 * az - r2 * ay, r2 * ax - r0 * az, r0 * ay - r1 * ax
        k = dot * (F32(1.0) - c)
        R = np.stack([(r0 * c + x0 * s) + ax * k, (r1 * c + x1 * s) + ay * k, (r2 * c + x2 * s) + az * k], axis=-1)
    p, R = K._frame32(F[D], p, R)
    assert p.dtype == F32 and R.dtype == F32
    return p, R, o, z


def first_controls(init, dt):
    """THE FIRST CONTROLS: init [N, T, D] -> u [N, T - 1, D] (float64)"""
    init = np.asarray(init, dtype=np.float64)
    v0 = np.zeros_like(init)
    v0[:, 1:] = (init[:, 1:] - init[:, :-1]) / dt
    return (v0[:, 1:] - v0[:, :-1]) / dt


def rollout(x0, u, dt):
    """x0 [N, 2 D], u [N, T - 1, D] -> x [N, T, 2 D]"""
    N, Tm, D = u.shape
    x = np.empty((N, Tm + 1, 2 * D))
    x[:, 0] = x0
    for t in range(Tm):
        x[:, t + 1, :D] = x[:, t, :D] + dt * x[:, t, D:]
        x[:, t + 1, D:] = x[:, t, D:] + dt * u[:, t]
    return x


def effort_matrix(D, R, effort):
    """S = R E^T E, or R I"""
    if effort is None:
        return R * np.eye(D)
    E = np.asarray(np.asarray(effort, dtype=F32), dtype=np.float64)
    return R * (E.T @ E)


def points(q, u, path, frames, axes, w, Se, lim, wl, prec, linearise=True):
    """THE POINT at every (row, t): q [n, T, D], u [n, T - 1, D], path [n, T, 3] -> (J [n], sum of |p - g|^2 [n], l_q [n, T, D],
    l_qq [n, T, D, D]) -- the last two float64 arrays holding float32 values under ``prec`` float32, None without ``linearise``"""
    n, T, D = q.shape
    g = np.asarray(path, dtype=np.float64)
    if prec == np.float64:
        qp = q.reshape(-1, D)
        p, _, o, z = K.walk64(qp, frames, axes)
    else:
        qp = q.reshape(-1, D).astype(F32)
        p, _, o, z = walk32(qp, frames, axes)
    e = p.astype(np.float64).reshape(n, T, 3) - g
    c = ((w * e) ** 2).sum(axis=2)
    sq = (e * e).sum(axis=(1, 2))
    viol = None
    if lim is not None:
        lo, hi = lim[:, 0].astype(prec), lim[:, 1].astype(prec)
        viol = np.where(qp > hi, qp - hi, np.where(qp < lo, qp - lo, prec(0.0)))             # in prec: the linearisation's
        lo64, hi64, q64 = lo.astype(np.float64), hi.astype(np.float64), qp.astype(np.float64)
        v64 = np.where(qp > hi, q64 - hi64, np.where(qp < lo, q64 - lo64, 0.0))
        c = c + wl * (v64 * v64).sum(axis=1).reshape(n, T)
    if T > 1:
        c[:, :-1] += np.einsum("nti,ij,ntj->nt", u, Se, u)
    J = c.sum(axis=1)
    if not linearise:
        return J, sq, None, None
    Jv = K._cross(z, p[:, None, :] - o)                                                       # [m, D, 3], J_v[r][i] = Jv[:, i, r]
    wp = w.astype(prec)
    ww = wp * wp
    ew = ww * (p - np.asarray(path, dtype=prec).reshape(-1, 3))
    two = prec(2.0)
    lq = two * ((Jv[:, :, 0] * ew[:, None, 0] + Jv[:, :, 1] * ew[:, None, 1]) + Jv[:, :, 2] * ew[:, None, 2])
    wJ = ww * Jv
    lqq = two * ((Jv[:, :, None, 0] * wJ[:, None, :, 0] + Jv[:, :, None, 1] * wJ[:, None, :, 1]) + Jv[:, :, None, 2] * wJ[:, None, :, 2])
    lqq = np.tril(lqq) + np.swapaxes(np.tril(lqq, -1), 1, 2)                                 # i >= j is what is formed; [j][i] is a copy
    assert lq.dtype == prec and lqq.dtype == prec
    if viol is not None:
        twl = prec(2.0) * prec(wl)
        on = viol != 0
        lq = np.where(on, lq + twl * viol, lq)
        idx = np.arange(D)
        lqq[:, idx, idx] = np.where(on, lqq[:, idx, idx] + twl, lqq[:, idx, idx])
    return J, sq, lq.astype(np.float64).reshape(n, T, D), lqq.astype(np.float64).reshape(n, T, D, D)


def _cholesky(M):
    """M [n, D, D] -> (L, ok [n]) column by column; ok: every pivot > 0"""
    n, D, _ = M.shape
    L = np.zeros_like(M)
    ok = np.ones(n, dtype=bool)
    for j in range(D):
        s = M[:, j:, j] - np.einsum("nik,nk->ni", L[:, j:, :j], L[:, j, :j])
        ok &= s[:, 0] > 0
        d = np.sqrt(s[:, 0])
        L[:, j, j] = d
        L[:, j + 1:, j] = s[:, 1:] / d[:, None]
    return L, ok


def _solve(L, Y):
    """L L^T X = Y: L [n, D, D], Y [n, D, m] -> X"""
    D = L.shape[1]
    X = np.array(Y, dtype=np.float64)
    for i in range(D):
        X[:, i] = (X[:, i] - np.einsum("nk,nkm->nm", L[:, i, :i], X[:, :i])) / L[:, i, i, None]
    for i in range(D - 1, -1, -1):
        X[:, i] = (X[:, i] - np.einsum("nk,nkm->nm", L[:, i + 1:, i], X[:, i + 1:])) / L[:, i, i, None]
    return X


def backward(u, lq, lqq, Se, dt, lam, prec, exits=None):
    """THE BACKWARD PASS for n rows at their own lam [n] -> (k [n, T - 1, D], K [n, T - 1, D, 2 D] as the forward pass uses them,
    ok [n]).  ``exits``: a list that gets, per step from T - 2 down, (t, the rows whose pivots were > 0, the rows whose gains were
    finite): which of the kernel's exits a rejected row takes and where."""
    n, Tm, D = u.shape
    A = np.eye(2 * D)
    A[:D, D:] = dt * np.eye(D)
    B = np.zeros((2 * D, D))
    B[D:] = dt * np.eye(D)
    vx = np.zeros((n, 2 * D))
    vx[:, :D] = lq[:, Tm]
    V = np.zeros((n, 2 * D, 2 * D))
    V[:, :D, :D] = lqq[:, Tm]
    ks, Ks = np.zeros((n, Tm, D)), np.zeros((n, Tm, D, 2 * D))
    ok = np.ones(n, dtype=bool)
    for t in range(Tm - 1, -1, -1):
        Qx = A.T @ vx[:, :, None]
        Qx = Qx[:, :, 0]
        Qx[:, :D] += lq[:, t]
        Qu = 2.0 * (u[:, t] @ Se.T) + vx @ B
        Qxx = A.T @ V @ A
        Qxx[:, :D, :D] += lqq[:, t]
        Qux = B.T @ V @ A
        Quu = 2.0 * Se + B.T @ V @ B + lam[:, None, None] * np.eye(D)
        L, good = _cholesky(Quu)
        pivots = good.copy()
        sol = -_solve(L, np.concatenate([Qu[:, :, None], Qux], axis=2))
        k, Kt = sol[:, :, 0], sol[:, :, 1:]
        kf, Kf = k.astype(F32), Kt.astype(F32)
        stored_k, stored_K = (k, Kt) if prec == np.float64 else (kf.astype(np.float64), Kf.astype(np.float64))
        # not finite as double or as float rejects the try (avae_track.h): the definition's rule too, though it uses the doubles
        good &= np.isfinite(k).all(axis=1) & np.isfinite(Kt).all(axis=(1, 2)) & np.isfinite(kf).all(axis=1) & np.isfinite(Kf).all(axis=(1, 2))
        ok &= good
        if exits is not None:
            exits.append((t, pivots, good | ~pivots))
        ks[:, t], Ks[:, t] = stored_k, stored_K
        KT = np.swapaxes(Kt, 1, 2)
        vx = Qx + (KT @ (Quu @ k[:, :, None] + Qu[:, :, None]))[:, :, 0] + (np.swapaxes(Qux, 1, 2) @ k[:, :, None])[:, :, 0]
        V = Qxx + KT @ (Quu @ Kt + Qux) + np.swapaxes(Qux, 1, 2) @ Kt
        V = 0.5 * (V + np.swapaxes(V, 1, 2))
    return ks, Ks, ok


def forward(x, u, ks, Ks, dt):
    """THE FORWARD PASS -> (x', u')"""
    n, Tm, D = u.shape
    xn, un = np.empty_like(x), np.empty_like(u)
    xn[:, 0] = x[:, 0]
    for t in range(Tm):
        un[:, t] = (u[:, t] + ks[:, t]) + np.einsum("nic,nc->ni", Ks[:, t], xn[:, t] - x[:, t])
        xn[:, t + 1, :D] = xn[:, t, :D] + dt * xn[:, t, D:]
        xn[:, t + 1, D:] = xn[:, t, D:] + dt * un[:, t]
    return xn, un


@np.errstate(over="ignore", invalid="ignore", divide="ignore")
def track(path, init, frames, axes, dt=0.01, track_weights=(10.0, 10.0, 50.0), effort_weight=0.01, effort=None, limits=None, limit_weight=0.0,
          n_iters=25, lam0=1.0, factor=10.0, lam_min=1e-6, lam_max=1e6, tol=1e-6, prec=np.float64):
    """avae_motion_track: path [N, T, 3], init [N, T, D] (float32 values) -> dict(trajectory [N, T, D], controls [N, T - 1, D],
    cost0, cost, track_rmse [N], iterations, accepted, status [N] int32, decisions: per row the string of its tries, 'a' accepted,
    'r' rejected by the cost, 'p' rejected by the backward pass).  ``prec`` float64: the definition; float32: the restatement, whose
    trajectory and controls are rounded to float32 as the kernel returns them."""
    path, init = np.asarray(path, dtype=F32), np.asarray(init, dtype=F32)
    N, T, D = init.shape
    dt, R, wl = float(F32(dt)), float(F32(effort_weight)), float(F32(limit_weight))
    w = np.asarray(track_weights, dtype=F32).astype(np.float64)
    lim = None if limits is None or not wl > 0 else np.asarray(limits, dtype=F32)
    Se = effort_matrix(D, R, effort)
    bad = ~np.isfinite(path).all(axis=(1, 2)) | ~np.isfinite(init).all(axis=(1, 2))
    if lim is not None and not np.isfinite(lim).all():
        bad[:] = True
    good = np.nonzero(~bad)[0]
    traj, ctrl = np.full((N, T, D), np.nan), np.full((N, max(T - 1, 0), D), np.nan)
    cost0, cost, rmse = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
    iters, acc = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    status = np.full(N, STATUS_NONFINITE, dtype=np.int32)
    decisions = [""] * N
    if good.size:
        g = path[good]
        u = first_controls(init[good], dt)
        x0 = np.concatenate([init[good, 0].astype(np.float64), np.zeros((good.size, D))], axis=1)
        x = rollout(x0, u, dt)
        J, sq, lq, lqq = points(x[:, :, :D], u, g, frames, axes, w, Se, lim, wl, prec)
        J0 = J.copy()
        lam = np.full(good.size, float(lam0))
        st = np.full(good.size, STATUS_OK if T == 1 else STATUS_CAP, dtype=np.int32)
        it, ac = np.zeros(good.size, dtype=np.int32), np.zeros(good.size, dtype=np.int32)
        active = np.full(good.size, T > 1 and n_iters > 0)
        dec = [""] * good.size
        for _ in range(n_iters if T > 1 else 0):
            idx = np.nonzero(active)[0]
            if not idx.size:
                break
            it[idx] += 1
            ks, Ks, ok = backward(u[idx], lq[idx], lqq[idx], Se, dt, lam[idx], prec)
            xn, un = forward(x[idx], u[idx], ks, Ks, dt)
            Jn, sqn, _, _ = points(xn[:, :, :D], un, g[idx], frames, axes, w, Se, lim, wl, prec, linearise=False)
            accept = ok & (Jn < J[idx])
            for r, o_, a_ in zip(idx, ok, accept):
                dec[r] += "a" if a_ else ("r" if o_ else "p")
            ia, ir = idx[accept], idx[~accept]
            conv = J[ia] - Jn[accept] < tol * J[ia]
            x[ia], u[ia], J[ia], sq[ia] = xn[accept], un[accept], Jn[accept], sqn[accept]
            lam[ia] = np.maximum(lam[ia] / factor, lam_min)
            ac[ia] += 1
            st[ia[conv]] = STATUS_OK
            active[ia[conv]] = False
            lam[ir] = lam[ir] * factor
            out = lam[ir] > lam_max
            st[ir[out]] = np.where(ac[ir[out]] > 0, STATUS_OK, STATUS_STUCK)
            active[ir[out]] = False
            if ia.size:
                _, _, lq[ia], lqq[ia] = points(x[ia][:, :, :D], u[ia], g[ia], frames, axes, w, Se, lim, wl, prec)
        q = x[:, :, :D]
        if prec != np.float64:
            q, u = q.astype(F32).astype(np.float64), u.astype(F32).astype(np.float64)
        traj[good], ctrl[good], cost0[good], cost[good], rmse[good] = q, u, J0, J, np.sqrt(sq / T)
        iters[good], acc[good], status[good] = it, ac, st
        for r, d in zip(good, dec):
            decisions[r] = d
    return dict(trajectory=traj, controls=ctrl, cost0=cost0, cost=cost, track_rmse=rmse, iterations=iters, accepted=acc,
                status=status, decisions=decisions)


def objective(u, x0, path, frames, axes, dt, w, Se, lim=None, wl=0.0):
    """J of the controls u [T - 1, D] from x0 [2 D] in float64 (the stationarity test's finite differences)"""
    x = rollout(x0[None], u[None], dt)
    return points(x[:, :, :D_(u)], u[None], path[None], frames, axes, w, Se, lim, wl, np.float64, linearise=False)[0][0]


def D_(u):
    return u.shape[-1]
