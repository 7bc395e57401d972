"""NumPy definition of the motion layer (vae_assoc_amd/motion.py, avae_motion_eval / _fit / _moments in include/avae.h, DESIGN.md
section 23): a fresh restatement of the reference's function approximator, pyrbf_funcapprox.py, cited by file:line.

``*64`` functions are the definition, in float64.  ``*32`` functions are the same definition in float32 arithmetic with the
kernels' operation order: float32 matrices and parameters, float32 products and sums over the basis index, the anchor terms
added behind them, the clamp by comparison, the moments by the sequential float32 update (tests/impute_reference.py:140-151), the
squared errors of a (row, joint) added per thread and then over the kernel's tree.  The distance of a ``*32`` result from the
``*64`` one on a test's own inputs is the yardstick of the GPU tests: the kernels may differ from float64 by rounding of that size.

``case`` builds the seeded inputs the tests share."""
import numpy as np

THREADS, J_MAX, PHI_FLOATS, MAX_SLAB, ROW_TILE = 256, 4, 4096, 512, 4      # the launch shapes of avae_motion.h


# ------------------------------------------------------------------------------------------------ the basis, float64
def features64(kind, K, z, normalize=True):
    """[len(z), K + 1].  pyrbf_funcapprox.py:26-39 (centres, widths), :72-78 (the two functions), :88-102 (a trailing 1)"""
    z = np.asarray(z, np.float64)
    out = np.ones((len(z), K + 1))
    for i in range(K):
        if kind == "sigmoid":
            t0 = np.linspace(1.0 / K, 1.0, K)[i]                 # :35
            out[:, i] = 1.0 / (1.0 + np.exp(-(K * 2) * (z - t0)))  # :34, :77
        else:
            mu = np.linspace(0.1, 0.9, K)[i]                     # :30
            out[:, i] = np.exp(-(z - mu) ** 2 / (1.0 / K))       # :31, :73
    if kind == "gaussian" and normalize and K:
        out[:, :K] /= out[:, :K].sum(1, keepdims=True)           # :92-93
    return out


def pinv64(F):
    """F [T, Kb] -> [Kb, T], singular values <= 1e-6 dropped (pyrbf_funcapprox.py:109-115; its ``features`` is F.T)"""
    U, s, V = np.linalg.svd(F)
    n = int((s > 1e-6).sum())
    return V.T[:, :n] @ np.diag(1.0 / s[:n]) @ U[:, :n].T


def constraint64(Fc):
    """Fc = features at the constrained phases [n_c, Kb] -> (A, B) with apply_lin_cons(theta) = A theta + B target
    (pyrbf_funcapprox.py:55-60: theta - C inv(C^T C) (C^T theta - target), C = Fc.T)"""
    Cm = Fc.T
    B = Cm @ np.linalg.pinv(Cm.T @ Cm)
    return np.eye(Cm.shape[0]) - B @ Cm.T, B


# ------------------------------------------------------------------------------------------------ the definition, float64
def _theta(params, scale, shift, D, dt):
    p = np.asarray(params, dt)
    sc = np.ones(p.shape[-1], dt) if scale is None else np.asarray(scale, dt)
    sh = np.zeros(p.shape[-1], dt) if shift is None else np.asarray(shift, dt)
    return (p * sc + sh).astype(dt).reshape(p.shape[:-1] + (D, -1))


def _clamp(q, limits):
    """pyrbf_funcapprox.py:136-141, per joint: by comparison, so NaN stays -> (q, clamped mask)"""
    hit = np.zeros(q.shape, bool)
    if limits is None:
        return q, hit
    q = q.copy()
    lim = np.asarray(limits, q.dtype)
    for d in range(q.shape[-1]):
        lo, hi = lim[d]
        if hi > lo:
            with np.errstate(invalid="ignore"):
                up = q[..., d] > hi
                q[..., d][up] = hi
                dn = q[..., d] < lo
                q[..., d][dn] = lo
            hit[..., d] = up | dn
    return q, hit


def unclamped(params, phi, D, scale=None, shift=None, gain=None, target=None, dt=np.float64):
    """params [..., P] -> q [..., T, D] before the clamp, in ``dt`` arithmetic"""
    th = _theta(params, scale, shift, D, dt)                                  # [..., D, Kb]
    q = np.matmul(np.asarray(phi, dt), np.swapaxes(th, -1, -2)).astype(dt)    # [T, Kb] x [..., Kb, D]
    if gain is not None:
        g, tg = np.asarray(gain, dt), np.asarray(target, dt)
        for c in range(g.shape[1]):
            q = (q + g[:, c][:, None] * tg[..., None, :, c]).astype(dt)
    return q


def eval64(params, phi, D, scale=None, shift=None, limits=None, gain=None, target=None, dt=np.float64):
    """-> (trajectory [R, T, D], saturated [R, D])"""
    q, hit = _clamp(unclamped(params, phi, D, scale, shift, gain, target, dt), limits)
    return q, hit.sum(-2).astype(np.int64)


def errors64(q, q_ref):
    """-> (rmse [R, D], max_abs [R, D]) over the time axis"""
    e = np.asarray(q, np.float64) - np.asarray(q_ref, np.float64)
    return np.sqrt((e ** 2).mean(-2)), np.abs(e).max(-2)


def fit64(traj, pinv, scale=None, shift=None, dt=np.float64):
    """traj [R, T, D] -> standardised parameters [R, D * Kb]"""
    th = np.matmul(np.asarray(pinv, dt), np.asarray(traj, dt)).astype(dt)     # [R, Kb, D]
    th = np.swapaxes(th, -1, -2).reshape(th.shape[0], -1)
    sc = np.ones(th.shape[1], dt) if scale is None else np.asarray(scale, dt)
    sh = np.zeros(th.shape[1], dt) if shift is None else np.asarray(shift, dt)
    return ((th - sh) / sc).astype(dt)


def moments64(samples, phi, D, scale=None, shift=None, limits=None, gain=None, target=None, delta=None):
    """samples [R, S, P] -> (mean, population variance [R, T, D], saturated_frac [R, D]): two passes over the S trajectories.
    With ``delta`` also ``sandwich``'s (fewest, most) clamped points per (row, joint) over samples and time."""
    samples = np.asarray(samples)
    R, S, _ = samples.shape
    out = []
    for r0 in range(0, R, 16):                                                    # (16 rows at a time bound the memory)
        tg = None if target is None else np.asarray(target)[r0:r0 + 16, None]
        raw = unclamped(samples[r0:r0 + 16], phi, D, scale, shift, gain, tg)      # [rows, S, T, D]
        q, hit = _clamp(raw, limits)
        mean = q.sum(1) / S
        res = (mean, ((q - mean[:, None]) ** 2).sum(1) / S, hit.sum((1, 2)) / float(S * q.shape[2]))
        out.append(res if delta is None else res + sandwich(raw, limits, delta, (1, 2)))
    return tuple(np.concatenate(x) for x in zip(*out))


# ------------------------------------------------------------------------------------------------ the float32 restatement
def slab_of(D, Kb, T):
    """time points of a slab and threads per joint (avae_motion.h motion_slab / motion_tq)"""
    tq = THREADS // D
    return min(J_MAX * tq, PHI_FLOATS // (Kb | 1), MAX_SLAB, T), tq


def eval32(params, phi, D, scale=None, shift=None, limits=None, gain=None, target=None):
    return eval64(params, np.asarray(phi, np.float32), D, scale, shift, None if limits is None else np.asarray(limits, np.float32),
                  None if gain is None else np.asarray(gain, np.float32), target, dt=np.float32)


def errors32(q, q_ref, Kb):
    """float32: a thread adds the squared errors of its own time points in order, then the tree over the joint's threads"""
    q, q_ref = np.asarray(q, np.float32), np.asarray(q_ref, np.float32)
    R, T, D = q.shape
    ts, tq = slab_of(D, Kb, T)
    e = q - q_ref
    part = np.zeros((R, tq, D), np.float32)
    for t in range(T):
        i = (t % ts) % tq
        part[:, i] = part[:, i] + e[:, t] * e[:, t]
    s = THREADS // 2
    while s:
        for i in range(min(s, tq)):
            if i + s < tq:
                part[:, i] = part[:, i] + part[:, i + s]
        s //= 2
    return np.sqrt(part[:, 0] / np.float32(T)), np.abs(e).max(1)


def fit32(traj, pinv, scale=None, shift=None):
    """k_motion_fit restated: theta[r][d][k] = sum_t pinv[k][t] traj[r][t][d] as one fma per t, t ascending, from 0 (a fused
    multiply-add is formed in float64 and rounded once), then (theta - shift) / scale in float32.  (A float32 matrix product is
    not that: a BLAS adds in several partial sums, which at T = 1024 is ten times closer to float64 than the kernel's one chain.)"""
    traj, pinv = np.asarray(traj, np.float32), np.asarray(pinv, np.float32)
    R, T, D = traj.shape
    th = np.zeros((R, pinv.shape[0], D), np.float32)
    for t in range(T):
        th = (pinv[None, :, t, None].astype(np.float64) * traj[:, None, t, :].astype(np.float64) + th.astype(np.float64)).astype(np.float32)
    th = np.swapaxes(th, -1, -2).reshape(R, -1)
    sc = np.ones(th.shape[1], np.float32) if scale is None else np.asarray(scale, np.float32)
    sh = np.zeros(th.shape[1], np.float32) if shift is None else np.asarray(shift, np.float32)
    out = (th - sh) / sc
    assert out.dtype == np.float32
    return out


def moments32(samples, phi, D, scale=None, shift=None, limits=None, gain=None, target=None):
    """the sequential float32 update, in sample order -> (mean, var, saturated_frac, the worst |q32 - q64| of a trajectory point)"""
    samples = np.asarray(samples, np.float32)
    R, S, _ = samples.shape
    mean = m2 = None
    sat, worst = 0, 0.0
    for k in range(S):
        q, hit = eval32(samples[:, k], phi, D, scale, shift, limits, gain, target)
        worst = max(worst, float(np.abs(q - eval64(samples[:, k], phi, D, scale, shift, limits, gain, target)[0]).max()))
        if mean is None:
            mean, m2 = np.zeros_like(q), np.zeros_like(q)
        d = q - mean
        mean = mean + d / np.float32(k + 1)
        m2 = m2 + d * (q - mean)
        sat = sat + hit
    return mean, m2 / np.float32(S), (sat / np.float64(S * mean.shape[1])).astype(np.float32), worst


NEAR = 1e-3


def moments_both(samples, phi, D, scale=None, shift=None, limits=None, gain=None, target=None):
    """``moments64`` and ``moments32`` in one pass over chunks of 16 rows, for the large cases -> dict: ``r64`` = (mean, var,
    saturated_frac), ``r32`` = (mean, var), ``worst`` = the largest |q32 - q64| of a trajectory point, and ``counts(delta)`` ->
    ``sandwich``'s (fewest, most) clamped points per (row, joint) for any delta <= NEAR (the points within NEAR of a limit are
    kept, the others counted at once)."""
    samples = np.asarray(samples, np.float32)
    R, S, _ = samples.shape
    lim32 = None if limits is None else np.asarray(limits, np.float32)
    r64, r32, worst, far, near = [], [], 0.0, [], []
    for r0 in range(0, R, 16):
        sm = samples[r0:r0 + 16]
        tg = None if target is None else np.asarray(target)[r0:r0 + 16, None]
        raw = unclamped(sm, phi, D, scale, shift, gain, tg)                       # [rows, S, T, D] float64
        q, hit = _clamp(raw, limits)
        mean = q.sum(1) / S
        r64.append((mean, ((q - mean[:, None]) ** 2).sum(1) / S, hit.sum((1, 2)) / float(S * q.shape[2])))
        q32 = _clamp(unclamped(sm, np.asarray(phi, np.float32), D, scale, shift,
                               None if gain is None else np.asarray(gain, np.float32), tg, np.float32), lim32)[0]
        worst = max(worst, float(np.abs(q32 - q).max()))
        m, m2 = np.zeros_like(q32[:, 0]), np.zeros_like(q32[:, 0])
        for k in range(S):
            d = q32[:, k] - m
            m = m + d / np.float32(k + 1)
            m2 = m2 + d * (q32[:, k] - m)
        r32.append((m, m2 / np.float32(S)))
        f, n = np.zeros((len(sm), D), np.int64), []
        for d in range(D if limits is not None else 0):
            lo, hi = np.asarray(limits, np.float32).astype(np.float64)[d]
            if hi > lo:
                s = np.maximum(raw[..., d] - hi, lo - raw[..., d])                # > 0: past a limit by that much
                f[:, d] = (s > NEAR).sum((1, 2))
                rows, _, _ = np.nonzero(np.abs(s) <= NEAR)
                n.append((rows + r0, np.full(len(rows), d), s[np.abs(s) <= NEAR]))
        far.append(f)
        near += n
    far = np.concatenate(far)

    def counts(delta):
        assert delta <= NEAR
        lo, hi = far.copy(), far.copy()
        for rows, ds, s in near:
            np.add.at(lo, (rows[s > delta], ds[s > delta]), 1)
            np.add.at(hi, (rows[s > -delta], ds[s > -delta]), 1)
        return lo, hi
    return dict(r64=tuple(np.concatenate(x) for x in zip(*r64)), r32=tuple(np.concatenate(x) for x in zip(*r32)), worst=worst,
                counts=counts)


# ------------------------------------------------------------------------------------------------ error measures
def rel_err(got, ref):
    """max |err| / (|ref| + 1); a NaN on one side only counts as infinite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    if (np.isnan(got) != np.isnan(ref)).any():
        return float("inf")
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(got - ref) / (np.abs(ref) + 1.0), initial=0.0))


def var_err(got, ref):
    """max |err| / max var64 (impute's measure)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(ref.max(), 1e-30))


def sandwich(q64_unclamped, limits, delta, axes):
    """-> (fewest, most) clamped points per (row, joint): a point counts for sure when it is past a limit by more than ``delta``
    and may count when it is within ``delta`` of it.  Joints without a valid limit pair: (0, 0)."""
    q = np.asarray(q64_unclamped, np.float64)
    sure, may = np.zeros(q.shape, bool), np.zeros(q.shape, bool)
    if limits is not None:
        for d in range(q.shape[-1]):
            lo, hi = np.asarray(limits, np.float32).astype(np.float64)[d]
            if hi > lo:
                sure[..., d] = (q[..., d] > hi + delta) | (q[..., d] < lo - delta)
                may[..., d] = (q[..., d] > hi - delta) | (q[..., d] < lo + delta)
    return sure.sum(axes), may.sum(axes)


# ------------------------------------------------------------------------------------------------ inputs
SHAPES = ((7, 21, 100), (1, 1, 1), (16, 64, 257), (3, 9, 2))           # (D, Kb, T)
ROWS = (1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 15, 16, 17, 300)       # the kernel's row tile is 4: 3, 4, 5 straddle it
VARIANTS = ("plain", "scaled", "limits", "anchor1", "anchor2", "all")
# The slab classes of avae_motion.h (slab_of: min(4 (256 / D), 4096 / (Kb | 1), 512, T) points):
#   (1, 5, 1024)   the 512 cap: two slabs, two points a thread
#   (7, 21, 1024)  limited by 4 TQ = 144: 8 slabs, the last of 16 points
#   (5, 13, 205)   204-point slabs and a last slab of one point
#   (2, 64, 64)    63-point slabs (the phi budget, Kb | 1 = 65) and a last slab of one point
#   (16, 20, 300)  64-point slabs, 44 in the last (three points a thread); P = 320: k_motion_fit's second parameter for 64 threads
CLASS_SHAPES = ((1, 5, 1024), (7, 21, 1024), (5, 13, 205), (2, 64, 64), (16, 20, 300))
CLASS_ROWS = (1, ROW_TILE + 1, 17)
CLASS_VARIANTS = VARIANTS + ("anchor3", "anchor4")                     # n_c = 3, 4: the phases ANCHOR_PHASES[:n_c]
ANCHOR_PHASES = (0.0, 0.25, 0.5, 1.0)
MOMENT_CLASS_SHAPES = ((16, 64, 257), (7, 21, 1024))                   # several slabs each
MOMENT_CLASS_S = (3, 5, 9)              # tiles of 4 samples: one short tile; a last tile of one sample; an odd count of 3 tiles


def matrices(D, Kb, T, kind="sigmoid"):
    """phi [T, Kb], pinv [Kb, T] of the basis with Kb - 1 functions at T phase points, float64"""
    F = features64(kind, Kb - 1, np.linspace(0.0, 1.0, T))
    return F, pinv64(F)


def case(shape, rows, variant, seed=0, kind="sigmoid", S=None):
    """One seeded case -> dict of float32 inputs (None where the variant has none): params [R, P] (or samples [R, S, P]), phi, pinv,
    scale, shift, limits, gain, target, nc and the raw float64 matrices.  theta ~ N(0, 1); the limits lie 1.5 standard deviations
    of the joint's unclamped values (with samples: those of the first 16 rows) either side of their mean, so some points clamp and
    some do not."""
    D, Kb, T = shape
    P = D * Kb
    rng = np.random.default_rng([seed, D, Kb, T, rows, CLASS_VARIANTS.index(variant), 0 if S is None else S])
    F, pinv = matrices(D, Kb, T, kind)
    c = dict(D=D, Kb=Kb, T=T, rows=rows, scale=None, shift=None, limits=None, gain=None, target=None, nc=0, F=F)
    theta = rng.standard_normal((rows, P) if S is None else (rows, S, P))
    if variant in ("scaled", "all"):
        sc, sh = rng.uniform(0.5, 1.5, P), rng.standard_normal(P)
        c["scale"], c["shift"] = sc.astype(np.float32), sh.astype(np.float32)
        theta = (theta - sh) / sc
    c["params"] = theta.astype(np.float32)
    phi = F
    nc = {"anchor1": 1, "anchor2": 2, "all": 2, "anchor3": 3, "anchor4": 4}.get(variant, 0)
    if nc:
        ph = np.array([0.0, 1.0][:nc] if nc <= 2 else ANCHOR_PHASES[:nc])
        A, Bm = constraint64(features64(kind, Kb - 1, ph))
        phi, c["gain"], c["nc"] = F @ A, (F @ Bm).astype(np.float32), nc
        c["target"] = rng.standard_normal((rows, D, nc)).astype(np.float32)
    c["phi"], c["pinv"] = phi.astype(np.float32), pinv.astype(np.float32)
    if variant in ("limits", "all"):
        tg = c["target"] if S is None or c["target"] is None else c["target"][:16, None]
        q = unclamped(c["params"] if S is None else c["params"][:16], c["phi"], D, c["scale"], c["shift"], c["gain"], tg)
        ax = tuple(range(q.ndim - 1))
        m, sd = q.mean(ax), q.std(ax)
        c["limits"] = np.stack([m - 1.5 * sd, m + 1.5 * sd], 1).astype(np.float32)
    return c


def eval_kw(c):
    return dict(scale=c["scale"], shift=c["shift"], limits=c["limits"], gain=c["gain"], target=c["target"])
