"""The definition of pen-path kinematics and stroke rendering (avae_motion_fk / avae_stroke_render, include/avae.h, DESIGN.md section
24) in NumPy float64, and next to it a float32 restatement of the kernels: the same operations in the order csrc/avae_render.h
writes down (a fused multiply-add is formed in float64 and rounded once; sin and cos are NumPy's float32 ones).  The restatement's
distance from the definition on a set of inputs is what the GPU tests build their bounds from (4x, the rule of test_gpu_motion.py).

Also the inputs of the tests: seeded paths of every family the renderer has to draw, and a brute-force hard-coverage raster."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
THREADS = 256

# (rows, T, D): the first three on the fixture chain (its first D joints move, the rest stay at 0), the last on a random chain
FK_SHAPES = ((1, 1, 1), (3, 2, 3), (5, 100, 7), (2, 257, 16))
# (T, H, ss)
RENDER_SHAPES = ((1, 28, 4), (2, 28, 1), (100, 28, 4), (100, 28, 8), (1024, 64, 2), (7, 5, 4))
HALF_WIDTH, MARGIN, SCALE = 0.0625, 0.6, 0.03

# The classes the kernels' own control flow distinguishes (csrc/avae_render.hip).  FK (rows, T, D): one tile of exactly 256 points
# with D = 2 (row length D | 1 = 3), 256 points with D = 4 (row length 5), exactly 512 points with D = 8 (row length 9), 513 points
# (a third tile of one point) with the odd D = 15.  FK_WILD: angles drawn uniformly in +-4 pi, past every joint limit.
FK_CLASS_SHAPES = ((1, 256, 2), (4, 64, 4), (2, 256, 8), (3, 171, 15))
FK_WILD = (5, 100, 7)
# The renderer (T, H, ss), by the 64-pixel chunks of step 4 (two per wave and trip: k0, k0 + 4, stride 8), the passes of step 5
# (256 / ss pixels each) and T against the 256 threads:
#   (3, 1, 8)     one pixel: a chunk of one lane, 8 items
#   (256, 8, 2)   exactly one full chunk (lane 63 owns a pixel), 255 segments
#   (257, 16, 1)  4 chunks (every wave's second chunk is out of range), thread 0 owns two points, the segment loop is one trip
#   (258, 20, 4)  7 chunks (the second element partly valid), 257 segments: a second trip of one
#   (513, 23, 2)  9 chunks (a second trip for wave 0 only), a third point for thread 0
#   (2, 64, 1)    64 chunks, ss = 1 on one segment, 256 pixels a pass
#   (100, 64, 8)  H ss = 512 (the size the header's culling argument is made at), 32 pixels a pass
RENDER_CLASS_SHAPES = ((3, 1, 8), (256, 8, 2), (257, 16, 1), (258, 20, 4), (513, 23, 2), (2, 64, 1), (100, 64, 8))
# (half_width, margin): the writer's; a hairline in a window without margin (r / delta small: the half diagonal dominates the
# culling threshold); a broad pen in a wide margin (r / delta large)
RENDER_CLASS_PARAMS = ((HALF_WIDTH, MARGIN), (0.002, 0.0), (0.5, 3.0))
RENDER_BIG = (100, 64, 8)                     # the definition and the restatement cost about 1.5 s a row here


def class_params(shape):
    """the (half_width, margin) pairs of a class shape: all three, the largest shape without the broad pen"""
    return RENDER_CLASS_PARAMS[:2] if tuple(shape) == RENDER_BIG else RENDER_CLASS_PARAMS


def rel_err(got, ref):
    """worst |err| / (|ref| + 1)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 1.0)).max()) if ref.size else 0.0


# ------------------------------------------------------------------------------------------------ chains
def fixture():
    with open(os.path.join(HERE, "golden", "baxter_right_chain.json")) as f:
        return json.load(f)


def fixture_joints(D=7):
    """the fixture's twelve joints with the first D revolute ones moving and the others held at angle 0 (fixed)"""
    out, d = [], 0
    for j in fixture()["joints"]:
        j = dict(j)
        if j["type"] == "revolute":
            d += 1
            if d > D:
                j["type"] = "fixed"
        out.append(j)
    return out


def random_joints(D, seed):
    """D revolute joints with arbitrary unit axes and origins, a fixed joint in front, between some and behind"""
    rng = np.random.default_rng([seed, D])
    out = [dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3))]
    for d in range(D):
        a = rng.standard_normal(3)
        out.append(dict(type="revolute", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3), axis=a / np.linalg.norm(a),
                        lower=-3.0, upper=3.0))
        if d % 3 == 1:
            out.append(dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3)))
    out.append(dict(type="fixed", xyz=rng.uniform(-0.3, 0.3, 3), rpy=rng.uniform(-3, 3, 3)))
    return out


def fk_case(shape, seed=0, wild=False):
    """-> dict(chain, frames, axes (float32), traj [rows, T, D] float32 inside the joint limits; ``wild``: uniform in +-4 pi,
    whatever the limits say)"""
    from vae_assoc_amd.kinematics import KinematicChain
    rows, T, D = shape
    chain = KinematicChain(fixture_joints(D) if D <= 7 else random_joints(D, seed))
    rng = np.random.default_rng([seed, rows, T, D] + ([1] if wild else []))
    if wild:
        frames, axes = chain.packed()
        return dict(chain=chain, frames=frames, axes=axes, traj=rng.uniform(-4.0 * np.pi, 4.0 * np.pi, size=(rows, T, D)).astype(F32))
    lim = chain.limits
    q = rng.uniform(lim[:, 0], lim[:, 1], size=(rows, T, D))
    # a smooth motion between two poses, as a trajectory is, plus the random pose
    tau = np.linspace(0.0, 1.0, T)[None, :, None]
    q = np.clip(0.5 * q + 0.5 * (q[:, :1] * (1.0 - tau) + q[:, -1:] * tau), lim[:, 0], lim[:, 1])
    frames, axes = chain.packed()
    return dict(chain=chain, frames=frames, axes=axes, traj=q.astype(F32))


def fk64(traj, frames, axes):
    """the definition on the packed constants: T = F_0 Rot_0 F_1 ... Rot_{D-1} F_D as 4 x 4 products, tip = T[:3, 3]"""
    q = np.asarray(traj, dtype=np.float64)
    F = np.asarray(frames, dtype=np.float64)
    A = np.asarray(axes, dtype=np.float64)
    D = A.shape[0]
    flat = q.reshape(-1, D)

    def hom(m34):
        return np.concatenate([m34, np.broadcast_to(np.array([[0.0, 0.0, 0.0, 1.0]]), m34.shape[:-2] + (1, 4))], axis=-2)
    Tm = np.broadcast_to(hom(F[0]), (flat.shape[0], 4, 4)).copy()
    for j in range(D):
        a = A[j]
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        c, s = np.cos(flat[:, j])[:, None, None], np.sin(flat[:, j])[:, None, None]
        R = np.zeros((flat.shape[0], 4, 4))
        R[:, :3, :3] = c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)
        R[:, 3, 3] = 1.0
        Tm = Tm @ R @ hom(F[j + 1])
    return Tm[:, :3, 3].reshape(q.shape[:-1] + (3,))


def fk32(traj, frames, axes):
    """k_motion_fk restated: the chain applied to a vector from the tip inwards, plain float32 products and sums"""
    q = np.asarray(traj, dtype=F32)
    F, A = np.asarray(frames, dtype=F32), np.asarray(axes, dtype=F32)
    D = A.shape[0]
    flat = q.reshape(-1, D)
    n = flat.shape[0]
    vx, vy, vz = (np.full(n, F[D, r, 3], dtype=F32) for r in range(3))
    for j in range(D - 1, -1, -1):
        s, c = np.sin(flat[:, j]), np.cos(flat[:, j])
        ax, ay, az = A[j]
        cx, cy, cz = ay * vz - az * vy, az * vx - ax * vz, ax * vy - ay * vx
        k = ((ax * vx + ay * vy) + az * vz) * (F32(1.0) - c)
        wx, wy, wz = (vx * c + cx * s) + ax * k, (vy * c + cy * s) + ay * k, (vz * c + cz * s) + az * k
        f = F[j]
        vx, vy, vz = (((f[r, 0] * wx + f[r, 1] * wy) + f[r, 2] * wz) + f[r, 3] for r in range(3))
    out = np.stack([vx, vy, vz], axis=-1)
    assert out.dtype == F32
    return out.reshape(q.shape[:-1] + (3,))


# ------------------------------------------------------------------------------------------------ rendering: the definition
def _dist2_64(u, v, c):
    """squared distance of the sample grid (u [n], v [m]) to the polyline c [T, 2] -> [m, n]"""
    m = np.full((v.size, u.size), np.inf)
    segs = [(c[0], c[0])] if len(c) == 1 else zip(c[:-1], c[1:])
    for a, b in segs:
        d = b - a
        len2 = d[0] * d[0] + d[1] * d[1]
        px, py = u[None, :] - a[0], v[:, None] - a[1]
        t = np.clip((px * d[0] + py * d[1]) / len2, 0.0, 1.0) if len2 > 0.0 else 0.0
        ex, ey = px - t * d[0], py - t * d[1]
        m = np.minimum(m, ex * ex + ey * ey)
    return m


def frame64(path, plane, r, margin):
    """one row -> (c [T, 2], ctr [2], W)"""
    p = np.asarray(path, dtype=np.float64)
    pl = np.asarray(plane, dtype=np.float64)
    c = (p - p.mean(0)) @ pl[:2].T
    lo, hi = c.min(0) - r, c.max(0) + r
    return c, (lo + hi) / 2.0, (1.0 + margin) * float((hi - lo).max())


def render64(path, plane, r, margin, H, ss, target=None, height=None):
    """the definition.  path [N, T, 3] -> dict(image [N, H * H], window [N, 3], img_l2 [N] or None, height_l2 [N] or None)"""
    path = np.asarray(path, dtype=np.float64)
    pl = np.asarray(plane, dtype=np.float64)
    r, margin = float(r), float(margin)
    N, n = path.shape[0], H * ss
    image, window = np.empty((N, H * H)), np.empty((N, 3))
    for i in range(N):
        if not np.isfinite(path[i]).all():
            image[i], window[i] = np.nan, np.nan
            continue
        c, ctr, W = frame64(path[i], pl, r, margin)
        delta = W / n
        u = ctr[0] - W / 2.0 + (np.arange(n) + 0.5) * delta
        v = ctr[1] + W / 2.0 - (np.arange(n) + 0.5) * delta
        cov = np.clip(0.5 + (r - np.sqrt(_dist2_64(u, v, c))) / delta, 0.0, 1.0)
        image[i] = cov.reshape(H, ss, H, ss).mean(axis=(1, 3)).reshape(-1)
        window[i] = ctr[0], ctr[1], W
    out = dict(image=image, window=window, img_l2=None, height_l2=None)
    if target is not None:
        out["img_l2"] = np.sqrt(((image - np.asarray(target, dtype=np.float64)) ** 2).sum(1))
    if height is not None:
        with np.errstate(invalid="ignore"):
            hn = path @ pl[2]
            out["height_l2"] = np.sqrt(((hn - np.asarray(height, dtype=np.float64)[:, None]) ** 2).sum(1))
        out["height_l2"][~np.isfinite(path).all(axis=(1, 2))] = np.nan
    return out


def hard_raster64(path, plane, r, margin, H, sub=32):
    """brute force: the share of ``sub x sub`` sample points of each pixel that lie within r of the polyline (one row's [T, 3] path).
    A pixel whose centre is further than r plus its half diagonal from the polyline holds none and is not sampled."""
    c, ctr, W = frame64(path, plane, r, margin)
    pitch = W / H
    pu = ctr[0] - W / 2.0 + (np.arange(H) + 0.5) * pitch
    pv = ctr[1] + W / 2.0 - (np.arange(H) + 0.5) * pitch
    near = np.sqrt(_dist2_64(pu, pv, c)) <= r + pitch * np.sqrt(0.5) * (1.0 + 1e-9)
    off = ((np.arange(sub) + 0.5) / sub - 0.5) * pitch
    img = np.zeros((H, H))
    for i, j in zip(*np.nonzero(near)):
        img[i, j] = (_dist2_64(pu[j] + off, pv[i] - off, c) <= r * r).mean()
    return img.reshape(-1)


# ------------------------------------------------------------------------------------------------ rendering: the restatement
def fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def tree32(x, op=np.add):
    """THE TREE of csrc/avae_render.h over 256 float32 values"""
    x = np.array(x, dtype=F32)
    s = THREADS // 2
    while s > 0:
        x[:s] = op(x[:s], x[s:2 * s])
        s //= 2
    return x[0]


def _strided(n):
    """thread i owns the items i, i + 256, ...: [(j, item indices, thread indices)] in the order a thread visits them"""
    return [(j, np.arange(j * THREADS, min(n, (j + 1) * THREADS)), np.arange(0, min(n, (j + 1) * THREADS) - j * THREADS))
            for j in range((n + THREADS - 1) // THREADS)]


def render32(path, plane, r, margin, H, ss, target=None, height=None):
    """k_stroke_render restated, without the culling (which changes no bit)"""
    path, pl = np.asarray(path, dtype=F32), np.asarray(plane, dtype=F32)
    r, margin = F32(r), F32(margin)
    N, T, n, npx = path.shape[0], path.shape[1], H * ss, H * H
    image, window = np.empty((N, npx), dtype=F32), np.empty((N, 3), dtype=F32)
    img_l2 = None if target is None else np.empty(N, dtype=F32)
    height_l2 = None if height is None else np.empty(N, dtype=F32)
    half, one, zero = F32(0.5), F32(1.0), F32(0.0)
    for i in range(N):
        p = path[i]
        if not np.isfinite(p).all():
            image[i], window[i] = np.nan, np.nan
            if img_l2 is not None:
                img_l2[i] = np.nan
            if height_l2 is not None:
                height_l2[i] = np.nan
            continue
        # 1. the mean
        part = np.zeros((THREADS, 3), dtype=F32)
        for _, items, th in _strided(T):
            part[th] = part[th] + p[items]
        mean = np.array([tree32(part[:, k]) for k in range(3)], dtype=F32) / F32(T)
        # 2. projection, box, height
        d = p - mean
        cu = fma32(pl[0, 2], d[:, 2], fma32(pl[0, 1], d[:, 1], pl[0, 0] * d[:, 0]))
        cv = fma32(pl[1, 2], d[:, 2], fma32(pl[1, 1], d[:, 1], pl[1, 0] * d[:, 0]))
        if height is not None:
            e = fma32(pl[2, 2], p[:, 2], fma32(pl[2, 1], p[:, 1], pl[2, 0] * p[:, 0])) - F32(height[i])
            acc = np.zeros(THREADS, dtype=F32)
            for _, items, th in _strided(T):
                acc[th] = fma32(e[items], e[items], acc[th])
            height_l2[i] = np.sqrt(tree32(acc))
        lo_u, hi_u, lo_v, hi_v = cu.min() - r, cu.max() + r, cv.min() - r, cv.max() + r
        ctr_u, ctr_v = (lo_u + hi_u) * half, (lo_v + hi_v) * half
        W = (one + margin) * max(hi_u - lo_u, hi_v - lo_v)
        delta = W / F32(n)
        u0, v0 = ctr_u - half * W, ctr_v + half * W
        window[i] = ctr_u, ctr_v, W
        # 3. segment records
        s1 = np.minimum(np.arange(max(T - 1, 1)) + 1, T - 1)
        ax, ay = cu[:max(T - 1, 1)], cv[:max(T - 1, 1)]
        dx, dy = cu[s1] - ax, cv[s1] - ay
        len2 = fma32(dy, dy, dx * dx)
        with np.errstate(divide="ignore"):
            inv = np.where(len2 >= F32(1e-30), one / len2, zero).astype(F32)
        # 5. every sample
        u = fma32(np.arange(n, dtype=F32) + half, delta, u0)[None, :]
        v = fma32(-(np.arange(n, dtype=F32) + half), delta, v0)[:, None]
        m = np.full((n, n), np.inf, dtype=F32)
        for s in range(len(ax)):
            px, py = u - ax[s], v - ay[s]
            t = np.minimum(np.maximum(fma32(px, dx[s], py * dy[s]) * inv[s], zero), one)
            ex, ey = fma32(-t, dx[s], px), fma32(-t, dy[s], py)
            m = np.minimum(m, fma32(ey, ey, ex * ex))
        x = half + (r - np.sqrt(m)) / delta
        cov = np.where(x > zero, np.minimum(x, one), zero).astype(F32).reshape(H, ss, H, ss)
        rs = cov[..., 0]
        for b in range(1, ss):
            rs = rs + cov[..., b]
        px_sum = rs[:, 0, :]
        for k in range(1, ss):
            px_sum = px_sum + rs[:, k, :]
        image[i] = (px_sum * F32(1.0 / (ss * ss))).reshape(-1)
        # 6. img_l2
        if target is not None:
            e = image[i] - np.asarray(target[i], dtype=F32)
            acc = np.zeros(THREADS, dtype=F32)
            for _, items, th in _strided(npx):
                acc[th] = fma32(e[items], e[items], acc[th])
            img_l2[i] = np.sqrt(tree32(acc))
    assert image.dtype == F32 and window.dtype == F32
    return dict(image=image, window=window, img_l2=img_l2, height_l2=height_l2)


# ------------------------------------------------------------------------------------------------ paths
FAMILIES = ("dot", "line_u", "line_v", "letter", "scribble", "outlier", "repeated")
CENTER = np.array([0.844, -0.357, 0.257])


def default_plane(scale=SCALE):
    return np.array([[0.0, -1.0 / scale, 0.0], [1.0 / scale, 0.0, 0.0], [0.0, 0.0, 1.0]])


def rotated_plane(seed=5, scale=SCALE):
    """an orthonormal frame in general position, u and v in units of ``scale``"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return np.array([q[0] / scale, q[1] / scale, q[2]])


def letter_uv(T, rng):
    """a smooth letter-like stroke in plane units, about 2 units across"""
    tau = np.linspace(0.0, 1.0, T)
    f, ph, amp = rng.uniform(0.5, 2.5, (2, 3)), rng.uniform(0, 2 * np.pi, (2, 3)), rng.uniform(0.2, 1.0, (2, 3))
    return np.stack([(amp[k][:, None] * np.sin(2 * np.pi * f[k][:, None] * tau[None, :] + ph[k][:, None])).sum(0) for k in range(2)], 1)


def path_uv(family, T, rng):
    tau = np.linspace(-1.0, 1.0, T) if T > 1 else np.zeros(1)
    if family == "dot":
        return np.tile(rng.uniform(-1, 1, (1, 2)), (T, 1))
    if family == "line_u":
        return np.stack([tau, np.zeros(T)], 1)
    if family == "line_v":
        return np.stack([np.zeros(T), tau], 1)
    if family == "letter":
        return letter_uv(T, rng)
    if family == "scribble":
        return rng.uniform(-1.0, 1.0, (T, 2))
    if family == "outlier":
        c = letter_uv(T, rng)
        c[T // 2] = c[T // 2] + np.array([25.0, -40.0])
        return c
    if family == "repeated":
        c = letter_uv((T + 1) // 2, rng)
        return np.repeat(c, 2, axis=0)[:T]
    if family == "diagonal":                                            # the box test passes everywhere: the distance culls alone
        return np.stack([tau, tau], 1)
    if family == "frame":                                               # the square's outline, once: ink at the window's edge
        s = np.linspace(0.0, 8.0, T)                                    # around an empty middle
        side = np.minimum(s // 2.0, 3.0).astype(int)
        a = s - 2.0 * side - 1.0                                        # -1 .. 1 along the side
        one = np.ones(T)
        u = np.select([side == 0, side == 1, side == 2, side == 3], [a, one, -a, -one])
        v = np.select([side == 0, side == 1, side == 2, side == 3], [-one, a, one, -a])
        return np.stack([u, v], 1)
    raise ValueError(family)


def lift(uv, plane, rng, scale=SCALE):
    """plane coordinates -> points in space whose projection with ``plane`` they are, on a paper with a little relief"""
    pl = np.asarray(plane, dtype=np.float64)
    uh, vh, nh = pl[0] * scale, pl[1] * scale, pl[2]
    h = 0.002 * rng.standard_normal(len(uv))
    return CENTER + scale * (uv[:, :1] * uh + uv[:, 1:] * vh) + h[:, None] * nh


def batches(shape, seed=0):
    """The calls of one (T, H, ss): [(name, plane float32 [3, 3], path float32 [rows, T, 3], height float32 [rows])] with 5, 2, 4, 1
    and 3 rows, every family under the default plane and four of them under a rotated one."""
    T = shape[0]
    plans = (("a", default_plane(), ("dot", "line_u", "line_v", "letter", "scribble")),
             ("b", default_plane(), ("outlier", "repeated")),
             ("c", rotated_plane(), ("letter", "outlier", "scribble", "repeated")),
             ("d", rotated_plane(), ("line_u",)),
             ("e", default_plane(), ("letter", "scribble", "dot")))
    out = []
    for name, plane, fams in plans:
        rng = np.random.default_rng([seed, T, ord(name)])
        path = np.stack([lift(path_uv(f, T, rng), plane, rng) for f in fams]).astype(F32)
        pl32 = plane.astype(F32)
        height = (path.astype(np.float64) @ pl32[2].astype(np.float64)).mean(1).astype(F32)
        out.append((name, pl32, path, height))
    return out


_CACHE = {}


def render_refs(shape, seed=0):
    """[(name, plane, path, height, target, r64, r32)] of ``batches(shape)``, computed once per process: the float64 definition and
    the float32 restatement with every output, the target a seeded picture in [0, 1]"""
    key = (tuple(shape), seed)
    if key not in _CACHE:
        T, H, ss = shape
        out = []
        for name, plane, path, height in batches(shape, seed):
            target = np.random.default_rng([seed, H, ord(name)]).random((path.shape[0], H * H)).astype(F32)
            r, mg = F32(HALF_WIDTH), F32(MARGIN)
            out.append((name, plane, path, height, target, render64(path, plane, r, mg, H, ss, target, height),
                        render32(path, plane, r, mg, H, ss, target, height)))
        _CACHE[key] = out
    return _CACHE[key]


CLASS_FAMILIES = FAMILIES + ("diagonal", "frame")
SHORT_FAMILIES = ("dot", "line_u", "line_v", "diagonal", "scribble")     # what a path of two or three points can be


def class_batches(shape, seed=0):
    """The calls of one class shape: [(name, plane, path, height)], one call under the default plane and one under the rotated
    one.  Every family under the first and six of them under the second; paths of two or three points take the families that
    make sense at that length; the largest shape takes two rows a call."""
    T = shape[0]
    if tuple(shape) == RENDER_BIG:
        plans = (("f", default_plane(), ("diagonal", "letter")), ("g", rotated_plane(), ("frame", "scribble")))
    elif T < 5:
        plans = (("f", default_plane(), SHORT_FAMILIES), ("g", rotated_plane(), ("diagonal", "scribble", "line_u")))
    else:
        plans = (("f", default_plane(), CLASS_FAMILIES),
                 ("g", rotated_plane(), ("letter", "outlier", "scribble", "repeated", "diagonal", "frame")))
    out = []
    for name, plane, fams in plans:
        rng = np.random.default_rng([seed, T, ord(name)])
        path = np.stack([lift(path_uv(f, T, rng), plane, rng) for f in fams]).astype(F32)
        pl32 = plane.astype(F32)
        height = (path.astype(np.float64) @ pl32[2].astype(np.float64)).mean(1).astype(F32)
        out.append((name, pl32, path, height))
    return out


def class_target(shape, name, rows, seed=0):
    return np.random.default_rng([seed, shape[1], ord(name)]).random((rows, shape[1] * shape[1])).astype(F32)


def class_refs(shape, params, seed=0):
    """[(name, plane, path, height, target, r64, r32)] of ``class_batches(shape)`` drawn with params = (half_width, margin),
    computed once per process"""
    key = ("class", tuple(shape), tuple(params), seed)
    if key not in _CACHE:
        T, H, ss = shape
        r, mg = F32(params[0]), F32(params[1])
        out = []
        for name, plane, path, height in class_batches(shape, seed):
            target = class_target(shape, name, path.shape[0], seed)
            out.append((name, plane, path, height, target, render64(path, plane, r, mg, H, ss, target, height),
                        render32(path, plane, r, mg, H, ss, target, height)))
        _CACHE[key] = out
    return _CACHE[key]


def class_coverage(shape, refs):
    """What a class case has to exercise, from the definition alone -> (smallest inked share of a row, largest number of step-5
    items, inked pixels x ss, of a row) over the calls of ``refs``"""
    inked = np.concatenate([(r64["image"] > 0.0).sum(1) for _, _, _, _, _, r64, _ in refs])
    return float(inked.min()) / (shape[1] * shape[1]), int(inked.max()) * shape[2]


def render_errors(got, ref):
    """-> dict of the worst absolute image error and the worst |err| / (|ref| + 1) of window, img_l2 and height_l2"""
    return dict(image=float(np.abs(np.asarray(got["image"], dtype=np.float64) - ref["image"]).max()),
                window=rel_err(got["window"], ref["window"]), img_l2=rel_err(got["img_l2"], ref["img_l2"]),
                height_l2=rel_err(got["height_l2"], ref["height_l2"]))
