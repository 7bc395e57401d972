"""Reference of the sigma-lognormal stroke model (include/avae.h): the float64 definition of
avae_lognormal_eval, avae_lognormal_sample and avae_lognormal_fit, and a restatement that follows csrc/avae_lognormal.h operation
for operation (float32 where the kernels are, their order in every sum), plus the generator of the strokes the tests fit.

``erf`` is torch's in float64 (scipy may be absent); the restatement takes log, exp, erf, sin and cos as the kernels do, in double
and rounded once to float32.  The stream: Philox4x32-10,
key = (seed lo, seed hi ^ 'slgn'), counter (row_offset + n, s, c, 0); the normals are the block's Box-Muller pairs, formed as
tests/search_reference.py forms them."""
import numpy as np
import torch

import search_reference as S
from denoise_reference import philox4x32_10

SALT = 0x736c676e
F32, F64 = np.float32, np.float64
SQRT2PI32, INVSQRTPI32 = F32(2.5066282746), F32(0.5641895835)
DEFAULT_WEIGHTS = (1.0, 1e-3)


def _erf(z):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(z))).numpy()


def _fn(fun, x):
    """a transcendental function as the kernels take it: in double, rounded once to the dtype of ``x``"""
    return fun(np.asarray(x, dtype=F64)).astype(x.dtype)


# ------------------------------------------------------------------------------------------------------------ the component
def components(p, t, f, jac=False):
    """THE COMPONENT of avae_lognormal.h in dtype ``f``: p [C, 6], t [T] -> (vx, vy [C, T], (jx, jy [C, 6, T]) or None).  Every
    operation is the header's, in its order; in float64 that is the definition."""
    p, t = np.asarray(p, dtype=f), np.asarray(t, dtype=f)
    D, t0, mu, sigma, ths, the = (p[:, j:j + 1] for j in range(6))
    sq2pi, isqpi = (SQRT2PI32, INVSQRTPI32) if f is F32 else (np.sqrt(2.0 * np.pi), 1.0 / np.sqrt(np.pi))
    tau = t[None, :] - t0
    sg = np.maximum(sigma, f(1e-6))
    on = tau >= f(1e-6)
    tc = np.maximum(tau, f(1e-6))
    z = (_fn(np.log, tc) - mu) / sg
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        u = np.where(on, _fn(np.exp, -(z * z) * f(0.5)) / ((sg * sq2pi) * (tc + f(1e-5))), f(0))
        amp = D * u
        a = np.abs(amp)
        E = _fn(_erf, z)
        q = the - ths
        phi = ths + (q * f(0.5)) * (f(1) + E)
        sn, cs = _fn(np.sin, phi), _fn(np.cos, phi)
        vx, vy = a * cs, a * sn
        if not jac:
            return vx.astype(f), vy.astype(f), None
        s = np.sign(amp)
        sa = s * amp
        K = -(q * isqpi) * _fn(np.exp, -(z * z))
        H = f(0.5) * (f(1) + E)
        zero = np.zeros_like(z)
        da = [s * u, sa * (f(1) / (tc + f(1e-5)) + z / (sg * tc)), (sa * z) / sg, (sa * (z * z - f(1))) / sg, zero, zero]
        dphi = [zero, K * np.where(on, f(1) / (sg * tc), f(0)), K * (f(1) / sg) + zero, K * (z / sg), f(1) - H, H]
        jx = np.stack([da[j] * cs - (a * sn) * dphi[j] for j in range(6)], axis=1)
        jy = np.stack([da[j] * sn + (a * cs) * dphi[j] for j in range(6)], axis=1)
    return vx.astype(f), vy.astype(f), (jx.astype(f), jy.astype(f))


def _times(T, dt, f):
    return np.arange(T).astype(f) * f(dt)


def _counts(params, count):
    N, C = params.shape[0], params.shape[1]
    return np.full(N, C, dtype=np.int64) if count is None else np.asarray(count, dtype=np.int64)


def _row_bad(p, cnt, start):
    return not (np.isfinite(p[:cnt]).all() and np.isfinite(start).all())


# ------------------------------------------------------------------------------------------------------------ eval
def stroke(p, start, T, dt):
    """The float64 definition of one stroke: p [count, 6] -> (path [T, 2], velocity [T, 2])"""
    p = np.asarray(p, dtype=F64).reshape(-1, 6)
    start = np.asarray(start, dtype=F64)
    vx, vy, _ = components(p, _times(T, dt, F64), F64)
    v = np.stack([vx.sum(0), vy.sum(0)], axis=1) if len(p) else np.zeros((T, 2))
    return start[None, :] + dt * np.cumsum(v, axis=0), v


def evaluate(params, count, start, T, dt):
    """avae_lognormal_eval in float64: params [N, C, 6], count [N] or None, start [N, 2] -> (path, velocity [N, T, 2]); a row with
    a non-finite start or parameter is NaN"""
    params, start = np.asarray(params, dtype=F64), np.asarray(start, dtype=F64)
    cnt = _counts(params, count)
    path, vel = np.full((len(params), T, 2), np.nan), np.full((len(params), T, 2), np.nan)
    for n in range(len(params)):
        if not _row_bad(params[n], cnt[n], start[n]):
            path[n], vel[n] = stroke(params[n, :cnt[n]], start[n], T, dt)
    return path, vel


def _scan64(x):
    """THE SCAN of avae_lognormal.h over one chunk of 64 float32 values"""
    x = x.copy()
    off = 1
    while off < 64:
        y = x.copy()
        y[off:] = x[off:] + x[:-off]
        x, off = y, off * 2
    return x


def stroke_restated(p, start, T, dt):
    """k_lognormal_eval's wave_stroke in float32: p [count, 6] float32 -> (path [T, 2], velocity [T, 2]) float32"""
    p = np.asarray(p, dtype=F32).reshape(-1, 6)
    start, dt = np.asarray(start, dtype=F32), F32(dt)
    vx, vy, _ = components(p, _times(T, dt, F32), F32)
    v = np.zeros((T, 2), dtype=F32)
    for c in range(len(p)):
        v[:, 0] = v[:, 0] + vx[c]
        v[:, 1] = v[:, 1] + vy[c]
    path = np.zeros((T, 2), dtype=F32)
    carry = np.zeros(2, dtype=F32)
    for k0 in range(0, T, 64):
        n = min(64, T - k0)
        for xy in range(2):
            chunk = np.zeros(64, dtype=F32)
            chunk[:n] = v[k0:k0 + n, xy]
            s = carry[xy] + _scan64(chunk)
            carry[xy] = s[63]
            path[k0:k0 + n, xy] = start[xy] + dt * s[:n]
    return path, v


def evaluate_restated(params, count, start, T, dt):
    params, start = np.asarray(params, dtype=F32), np.asarray(start, dtype=F32)
    cnt = _counts(params, count)
    path, vel = np.full((len(params), T, 2), np.nan, dtype=F32), np.full((len(params), T, 2), np.nan, dtype=F32)
    for n in range(len(params)):
        if not _row_bad(params[n], cnt[n], start[n]):
            path[n], vel[n] = stroke_restated(params[n, :cnt[n]], start[n], T, dt)
    return path, vel


# ------------------------------------------------------------------------------------------------------------ sample
def words(seed, N, S_, C, row_offset=0):
    """uint32 [N, S, C, 4]: the Philox blocks of a call"""
    n = (row_offset + np.arange(N, dtype=np.uint64))[:, None, None]
    s = np.arange(S_, dtype=np.uint64)[None, :, None]
    c = np.arange(C, dtype=np.uint64)[None, None, :]
    return np.stack(philox4x32_10(n, s, c, 0, seed & 0xFFFFFFFF, ((seed >> 32) ^ SALT) & 0xFFFFFFFF), axis=-1)


def normals(seed, N, S_, C, row_offset=0):
    """float64 [N, S, C, 3]: the first three Box-Muller normals of every block (the uniforms formed in float32 as on the device)"""
    u = S._uniforms(words(seed, N, S_, C, row_offset)).astype(F64)
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    return np.stack([ra * np.cos(2.0 * np.pi * u[..., 1]), ra * np.sin(2.0 * np.pi * u[..., 1]), rb * np.cos(2.0 * np.pi * u[..., 3])], -1)


def normals_f32(seed, N, S_, C, row_offset=0):
    """float32 [N, S, C, 3]: box_muller4 with every operation rounded to float32"""
    u = S._uniforms(words(seed, N, S_, C, row_offset))
    ra = np.sqrt(F32(-2.0) * np.log(u[..., 0]).astype(F32)).astype(F32)
    rb = np.sqrt(F32(-2.0) * np.log(u[..., 2]).astype(F32)).astype(F32)
    ang = lambda v: 2.0 * np.pi * v.astype(F64)
    return np.stack([ra * np.cos(ang(u[..., 1])).astype(F32), ra * np.sin(ang(u[..., 1])).astype(F32),
                     rb * np.cos(ang(u[..., 3])).astype(F32)], -1).astype(F32)


def perturb(params, count, nrm, amplitude, angle, straightness, f):
    """params [N, C, 6], normals [N, S, C, 3] -> perturbed [N, S, C, 6] in dtype ``f`` (zeros for c >= count)"""
    p = np.asarray(params, dtype=f)[:, None, :, :]
    n = (np.asarray(nrm, dtype=f) / f(3.0)).astype(f)
    out = np.broadcast_to(p, n.shape[:3] + (6,)).astype(f).copy()
    D, ths, the = p[..., 0], p[..., 4], p[..., 5]
    out[..., 0] = D + (n[..., 0] * f(amplitude)) * D
    out[..., 4] = ths + n[..., 1] * f(angle)
    out[..., 5] = (the + n[..., 1] * f(angle)) + (n[..., 2] * f(straightness)) * (the - ths)
    cnt = _counts(np.asarray(params), count)
    out[np.broadcast_to(np.arange(out.shape[2])[None, None, :] >= cnt[:, None, None], out.shape[:3])] = 0
    return out


def sample(params, count, start, T, dt, S_, seed, amplitude=0.2, angle=np.pi / 9, straightness=0.1, shift_mean=True, row_offset=0):
    """avae_lognormal_sample in float64 -> (strokes [N, S, T, 2], perturbed [N, S, C, 6])"""
    params = np.asarray(params, dtype=F64)
    N, C = params.shape[0], params.shape[1]
    pert = perturb(params, count, normals(seed, N, S_, C, row_offset), amplitude, angle, straightness, F64)
    out = np.stack([evaluate(pert[:, s], count, start, T, dt)[0] for s in range(S_)], axis=1)
    if shift_mean:
        out = out - out.mean(axis=2, keepdims=True)
    return out, pert


def mean_restated(path):
    """the sample kernel's mean point of path [T, 2] float32: per-lane sums, THE BUTTERFLY, a division by (float)T"""
    T = path.shape[0]
    lanes = np.zeros((64, 2), dtype=F32)
    for k0 in range(0, T, 64):
        n = min(64, T - k0)
        lanes[:n] = lanes[:n] + path[k0:k0 + n]
    off = 32
    while off:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off //= 2
    return lanes[0] / F32(T)


def sample_restated(params, count, start, T, dt, S_, seed, amplitude=0.2, angle=np.pi / 9, straightness=0.1, shift_mean=True,
                    row_offset=0):
    params = np.asarray(params, dtype=F32)
    N, C = params.shape[0], params.shape[1]
    pert = perturb(params, count, normals_f32(seed, N, S_, C, row_offset), amplitude, angle, straightness, F32)
    out = np.stack([evaluate_restated(pert[:, s], count, start, T, dt)[0] for s in range(S_)], axis=1)
    if shift_mean:
        for n in range(N):
            for s in range(S_):
                out[n, s] = out[n, s] - mean_restated(out[n, s])[None, :]
    return out, pert


# ------------------------------------------------------------------------------------------------------------ fit
def target_velocity(P, start, dt, f):
    P, start = np.asarray(P, dtype=f), np.asarray(start, dtype=f)
    prev = np.concatenate([start[None, :], P[:-1]], axis=0)
    return ((P - prev) / f(dt)).astype(f)


def jacobian(p, start, T, dt):
    """float64: p [count, 6] -> (path, v [T, 2], JP, JV [T, 2, 6 count]): the Jacobians of position and velocity"""
    p = np.asarray(p, dtype=F64).reshape(-1, 6)
    path, v = stroke(p, start, T, dt)
    _, _, (jx, jy) = components(p, _times(T, dt, F64), F64, jac=True)
    JV = np.stack([jx.reshape(-1, T).T, jy.reshape(-1, T).T], axis=1)            # [T, 2, P], column 6 c + j
    return path, v, dt * np.cumsum(JV, axis=0), JV


def _pass64(p, tgt, start, dt, wp, wv, jac):
    T = len(tgt)
    V = target_velocity(tgt, start, dt, F64)
    if not jac:
        path, v = stroke(p, start, T, dt)
        return wp * ((path - tgt) ** 2).sum() + wv * ((v - V) ** 2).sum(), None, None
    path, v, JP, JV = jacobian(p, start, T, dt)
    ep, ev = path - tgt, v - V
    A, B = JP.reshape(2 * T, -1), JV.reshape(2 * T, -1)
    return (wp * (ep ** 2).sum() + wv * (ev ** 2).sum(), wp * A.T @ A + wv * B.T @ B, wp * A.T @ ep.reshape(-1) + wv * B.T @ ev.reshape(-1))


def _pass32(p, tgt, start, dt, wp, wv, jac):
    """A PASS of avae_lognormal.h: float32 model values and Jacobian, running sums over k, double accumulation row by row"""
    p = np.asarray(p, dtype=F32).reshape(-1, 6)
    tgt, start, dt = np.asarray(tgt, dtype=F32), np.asarray(start, dtype=F32), F32(dt)
    T, Pn = len(tgt), 6 * len(p)
    vx, vy, J = components(p, _times(T, dt, F32), F32, jac=jac)
    v = np.zeros((T, 2), dtype=F32)
    for c in range(len(p)):
        v[:, 0] = v[:, 0] + vx[c]
        v[:, 1] = v[:, 1] + vy[c]
    run = np.cumsum(v, axis=0, dtype=F32)                  # (a running sum: numpy's cumsum adds in order)
    pos = (start[None, :] + dt * run).astype(F32)
    V = target_velocity(tgt, start, dt, F32)
    e = np.concatenate([pos.astype(F64) - tgt.astype(F64), v.astype(F64) - V.astype(F64)], axis=1)      # [T, 4]
    w = np.array([wp, wp, wv, wv], dtype=F64)
    L = 0.0
    for k in range(T):
        for r in range(4):
            L = L + (w[r] * e[k, r]) * e[k, r]
    if not jac:
        return L, None, None
    JV = np.stack([J[0].reshape(Pn, T).T, J[1].reshape(Pn, T).T], axis=1).astype(F32)                   # [T, 2, P]
    JP = (dt * np.cumsum(JV, axis=0, dtype=F32)).astype(F32)
    rows = np.concatenate([JP, JV], axis=1).astype(F64)                                                 # [T, 4, P]
    M, g = np.zeros((Pn, Pn)), np.zeros(Pn)
    for k in range(T):
        for r in range(4):
            wa = w[r] * rows[k, r]
            M = M + wa[:, None] * rows[k, r][None, :]
            g = g + wa * e[k, r]
    return L, M, g


def _solve(M, g, why=None):
    """the kernel's Cholesky and substitutions in double, its order -> x or None (a pivot not > 0, a non-finite x); ``why`` (a
    list) gets "ok", "pivot" or "x" appended: which of the two rejections a failed solve took"""
    why = [] if why is None else why
    n = len(g)
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            s = M[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not s > 0.0:
                why.append("pivot")
                return None
            L[j, j] = np.sqrt(s)
            v = M[j + 1:, j].copy()
            for k in range(j):
                v = v - L[j + 1:, k] * L[j, k]
            L[j + 1:, j] = v / L[j, j]
        y = g.copy()
        for j in range(n):
            y[j] = y[j] / L[j, j]
            y[j + 1:] = y[j + 1:] - L[j + 1:, j] * y[j]
        for j in range(n - 1, -1, -1):
            y[j] = y[j] / L[j, j]
            y[:j] = y[:j] - L[j, :j] * y[j]
    why.append("ok" if np.isfinite(y).all() else "x")
    return y if np.isfinite(y).all() else None


def fit_row(tgt, init, start, dt, n_iters=40, weights=DEFAULT_WEIGHTS, free=None, lo=None, hi=None, tol=1e-9, restated=False):
    """avae_lognormal_fit for one row: tgt [T, 2], init [count, 6], free None or bool [count, 6] -> dict(params [count, 6], loss0,
    loss, iterations, accepted, status, tries: [(L, L(new) or None)] per try, solves: "ok", "pivot" or "x" per try).  ``restated``:
    float32 parameters, model values and Jacobian in the kernel's orders; else everything in float64."""
    f = F32 if restated else F64
    run = _pass32 if restated else _pass64
    wp, wv = float(weights[0]), float(weights[1])
    tgt, start = np.asarray(tgt, dtype=f), np.asarray(start, dtype=f)
    p = np.asarray(init, dtype=f).reshape(-1, 6).copy()
    cnt = len(p)
    out = dict(params=np.full((cnt, 6), np.nan, dtype=f), loss0=np.nan, loss=np.nan, iterations=0, accepted=0, status=3, tries=[],
               solves=[])
    if not (np.isfinite(tgt).all() and np.isfinite(start).all() and np.isfinite(p).all()):
        return out
    fr = np.ones(6 * cnt, dtype=bool) if free is None else np.broadcast_to(np.asarray(free, dtype=bool), (cnt, 6)).reshape(-1)
    L = run(p, tgt, start, dt, wp, wv, False)[0]
    out.update(loss0=L, status=0 if cnt == 0 else 1)
    lam, rejects, it, acc = 1e-3, 0, 0, 0
    while cnt > 0 and it < n_iters:
        _, M, g = run(p, tgt, start, dt, wp, wv, True)
        it += 1
        M, g = M.copy(), g.copy()
        off = ~(fr[:, None] & fr[None, :])
        M[off] = 0.0
        M[np.arange(6 * cnt)[~fr], np.arange(6 * cnt)[~fr]] = 1.0
        g[~fr] = 0.0
        d = np.where(fr, np.diag(M), 0.0)
        md = max(0.0, d.max()) if len(d) else 0.0
        M[np.arange(6 * cnt)[fr], np.arange(6 * cnt)[fr]] += lam * d[fr] + 1e-12 * (md + 1.0)
        x = _solve(M, g, out["solves"])
        Ln = None
        if x is not None:
            new = (p.reshape(-1).astype(F64) - x).astype(f).reshape(cnt, 6)
            new[:, 3] = np.minimum(np.maximum(new[:, 3], f(1e-3)), f(3.0))
            if lo is not None:
                new = np.maximum(new, np.asarray(lo, dtype=f)[None, :])
            if hi is not None:
                new = np.minimum(new, np.asarray(hi, dtype=f)[None, :])
            new = np.where(fr.reshape(cnt, 6), new, p).astype(f)
            Ln = run(new, tgt, start, dt, wp, wv, False)[0]
        out["tries"].append((L, Ln))
        if Ln is not None and Ln < L:
            conv = L - Ln < tol * L
            p, L, lam, acc, rejects = new, Ln, max(lam / 3.0, 1e-9), acc + 1, 0
            if conv:
                out["status"] = 0
                break
        else:
            lam, rejects = min(4.0 * lam, 1e9), rejects + 1
            if rejects == 8:
                out["status"] = 0 if acc > 0 else 2
                break
    out.update(params=p, loss=L, iterations=it, accepted=acc)
    return out


def fit(target, init, count, start, dt, free=None, **opt):
    """Every row through ``fit_row`` -> dict of stacked outputs: params [N, C, 6] (zeros above count, NaN for status 3), loss0, loss,
    iterations, accepted, status, tries (a list per row).  ``free``: None, [6] or [N, C, 6]."""
    init = np.asarray(init)
    N, C = init.shape[0], init.shape[1]
    cnt = _counts(init, count)
    res = dict(params=np.zeros((N, C, 6)), loss0=np.zeros(N), loss=np.zeros(N), iterations=np.zeros(N, np.int32),
               accepted=np.zeros(N, np.int32), status=np.zeros(N, np.int32), tries=[], solves=[])
    for n in range(N):
        fr = None if free is None else (np.asarray(free)[n, :cnt[n]] if np.asarray(free).ndim == 3 else np.asarray(free))
        r = fit_row(target[n], init[n, :cnt[n]], start[n], dt, free=fr, **opt)
        if r["status"] == 3:
            res["params"][n] = np.nan
        else:
            res["params"][n, :cnt[n]] = r["params"]
        for k in ("loss0", "loss", "iterations", "accepted", "status"):
            res[k][n] = r[k]
        res["tries"].append(r["tries"])
        res["solves"].append(r["solves"])
    return res


# ------------------------------------------------------------------------------------------------------------ cases
T_CASE, DT_CASE, START_CASE = 100, 0.01, (0.1, -0.2)


def separated_params(C, rng, sigma_guess=None):
    """C components separated in time: centres ((c + 0.5) / C) 0.8 + 0.08, sigma ~ U(0.15, 0.4), width U(0.8, 1.3) 0.9 / C, mu and
    t0 from width and centre as the initial guess forms them, D ~ U(0.3, 1.5), theta_s ~ U(-3, 3), theta_e - theta_s ~
    U(-1.5, 1.5) -> [C, 6]"""
    centre = ((np.arange(C) + 0.5) / C) * 0.8 + 0.08
    sigma = rng.uniform(0.15, 0.4, C)
    width = rng.uniform(0.8, 1.3, C) * 0.9 / C
    mu = np.log(width / (np.exp(3.0 * sigma) - np.exp(-3.0 * sigma)))
    t0 = centre - np.exp(mu - sigma * sigma)
    D = rng.uniform(0.3, 1.5, C)
    ths = rng.uniform(-3.0, 3.0, C)
    the = ths + rng.uniform(-1.5, 1.5, C)
    return np.stack([D, t0, mu, sigma, ths, the], axis=1)


def separated_stroke(C, rng):
    """-> (stroke [T, 2] float64, params [C, 6]) at T = 100, dt = 0.01, start (0.1, -0.2)"""
    p = separated_params(C, rng)
    return stroke(p, START_CASE, T_CASE, DT_CASE)[0], p


def extent(path):
    path = np.asarray(path, dtype=F64)
    return float(np.max(path.max(axis=-2) - path.min(axis=-2)))


def rel_err(got, ref):
    """worst |err| / (|ref| + 1); NaN where both are NaN counts as equal"""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    both = np.isnan(got) & np.isnan(ref)
    e = np.where(both, 0.0, np.abs(got - ref) / (np.abs(ref) + 1.0))
    return float(np.max(e)) if e.size else 0.0


# the default-option contract: (C, seed) of separated_stroke(C, default_rng(100 C + seed)).  The initial guess reads a component's
# angles where its speed pulse begins and ends; where neighbours overlap (C = 4 and 6: widths up to 1.3 * 0.9 / C against centres
# 0.8 / C apart) those are the neighbour's angles, and from some such guesses the float64 definition itself ends in another
# minimum (C = 4: seeds 6, 8 of 0 .. 11; C = 6: seeds 0, 1, 4, 6).  The tests are about the fit, so they take the first four seeds
# from which the definition reproduces the stroke; tests/test_lognormal_cpu.py asserts that it does.
CONTRACT_SEEDS = {1: (0, 1, 2, 3), 2: (0, 1, 2, 3), 3: (0, 1, 2, 3), 4: (0, 1, 2, 3), 6: (2, 3, 5, 7)}


def contract_stroke(C, seed):
    return separated_stroke(C, np.random.default_rng(100 * C + seed))


def step_case(N, C, seed, counts=None, T=T_CASE, dt=DT_CASE):
    """A step-for-step case: N strokes of C separated components (row n: counts[n] of them) at T points dt apart, the float64
    stroke rounded to float32 as the target, and the true parameters perturbed by up to 10 % as the start -> dict(target
    [N, T, 2], init [N, C, 6], count [N], start [N, 2], true [N, C, 6]) in float32 / int32"""
    rng = np.random.default_rng(seed)
    counts = [C] * N if counts is None else list(counts)
    true, tgt = np.zeros((N, C, 6)), np.zeros((N, T, 2))
    for n, c in enumerate(counts):
        if c:
            true[n, :c] = separated_params(c, rng)
        tgt[n] = stroke(true[n, :c], START_CASE, T, dt)[0]
    init = true * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, true.shape))
    return dict(target=tgt.astype(F32), init=init.astype(F32), count=np.asarray(counts, dtype=np.int32),
                start=np.tile(np.asarray(START_CASE, dtype=F32), (N, 1)), true=true.astype(F32))


def margins(tries):
    """the smallest |L(new) - L| / L over the tries of a run (inf for a run without a priced try)"""
    m = [abs(ln - l) / l for l, ln in tries if ln is not None and l > 0]
    return min(m) if m else np.inf


# ---- the step-for-step cases: (name, N, C, counts or None, variant); the seeds are chosen so that every accept decision of the
# float64 definition over the four compared tries has a margin |L(new) - L| > 1e-3 L (the tests assert it): a decision that
# close could fall the other way in float32, and the runs would part ways
BOUNDS_THAT_BIND = ((-np.inf, -np.inf, -np.inf, 0.2, -np.inf, -np.inf), (1.0, np.inf, np.inf, 0.3, np.inf, np.inf))
STEP_CASES = [
    ("1x1", 1, 1, None, "full"), ("3x3", 3, 3, None, "full"), ("5x4", 5, 4, None, "full"), ("2x5", 2, 5, None, "full"),
    ("2x8", 2, 8, None, "full"), ("1x16", 1, 16, None, "full"), ("ragged", 5, 5, (5, 4, 3, 1, 0), "full"),
    ("3x3-angles", 3, 3, None, "angles"), ("3x3-timing", 3, 3, None, "timing"), ("2x8-angles", 2, 8, None, "angles"),
    ("ragged-per-row", 5, 5, (5, 4, 3, 1, 0), "per_row"), ("3x3-bounds", 3, 3, None, "bounds"), ("5x4-bounds", 5, 4, None, "bounds"),
    ("2x8-timing-bounds", 2, 8, None, "timing+bounds"),
]
STEP_SEEDS = {"3x3-angles": 1008, "ragged-per-row": 1004}          # every other case: 1000 (the first seed tried)


def step_seed(name):
    return STEP_SEEDS.get(name, 1000)


def step_options(case, variant):
    """-> (free: None, [6] or [N, C, 6] uint8; bounds: None or (lo, hi))"""
    N, C = case["init"].shape[0], case["init"].shape[1]
    free, bounds = None, None
    if "angles" in variant:
        free = np.array([0, 0, 0, 0, 1, 1], dtype=np.uint8)
    if "timing" in variant:
        free = np.array([1, 1, 1, 1, 0, 0], dtype=np.uint8)
    if "per_row" in variant:
        free = (np.random.default_rng(77).random((N, C, 6)) < 0.7).astype(np.uint8)
    if "bounds" in variant:
        bounds = BOUNDS_THAT_BIND
    return free, bounds


def run_step_case(case, variant, n_iters, restated):
    free, bounds = step_options(case, variant)
    lo, hi = (None, None) if bounds is None else bounds
    return fit(case["target"], case["init"], case["count"], case["start"], DT_CASE, free=free, n_iters=n_iters, tol=0.0, lo=lo, hi=hi,
               restated=restated)
