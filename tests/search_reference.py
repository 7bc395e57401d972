"""Reference of the black-box search (include/avae.h): the float64 definition of avae_search_sample and
avae_search_update, a restatement that follows csrc/avae_search.h operation for operation (float32 where the kernel is, the
kernel's order in every sum), the loop around them, and the cases the GPU tests run.

The stream: Philox4x32-10, key = (seed lo, seed hi ^ 'srch'), counter (problem_offset + p, r, dimension quad, iteration); the
normals are the Box-Muller pairs of the block, formed as the internal eps is (tests/denoise_reference.py)."""
import itertools

import numpy as np

from denoise_reference import philox4x32_10

SALT = 0x73726368
PIBB, CEM, CMAES = "PI-BB", "CEM", "CMA-ES"
THREADS = 256


def options(weighting=PIBB, cov_update=PIBB, eliteness=10.0, lr=1.0, rel_lower=0.1, abs_lower=-1.0, abs_upper=-1.0, tol=1e-6):
    return dict(weighting=weighting, cov_update=cov_update, eliteness=float(eliteness), lr=float(lr), rel_lower=float(rel_lower),
                abs_lower=float(abs_lower), abs_upper=float(abs_upper), tol=float(tol))


# ---------------------------------------------------------------------------------------------------------------- sample
def words(seed, iteration, P, R, n, problem_offset=0):
    """uint32 [P, R, n_quads, 4]: the Philox blocks of a call"""
    nq = (n + 3) // 4
    p = (problem_offset + np.arange(P, dtype=np.uint64))[:, None, None]
    r = np.arange(R, dtype=np.uint64)[None, :, None]
    q = np.arange(nq, dtype=np.uint64)[None, None, :]
    w = philox4x32_10(p, r, q, int(iteration), seed & 0xFFFFFFFF, ((seed >> 32) ^ SALT) & 0xFFFFFFFF)
    return np.stack(w, axis=-1)


def _uniforms(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normals(seed, iteration, P, R, n, problem_offset=0):
    """float64 [P, R, n]: the uniforms formed in float32 as on the device, log / sqrt / sin / cos in double"""
    u = _uniforms(words(seed, iteration, P, R, n, problem_offset)).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a, b = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    z = np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], axis=-1)
    return z.reshape(P, R, -1)[:, :, :n]


def normals_f32(seed, iteration, P, R, n, problem_offset=0):
    """float32 [P, R, n]: box_muller4 with every operation rounded to float32 (the device's log / sin / cos are the hardware's)"""
    f = np.float32
    u = _uniforms(words(seed, iteration, P, R, n, problem_offset))
    ra = np.sqrt(f(-2.0) * np.log(u[..., 0]).astype(f)).astype(f)
    rb = np.sqrt(f(-2.0) * np.log(u[..., 2]).astype(f)).astype(f)
    ang = lambda v: 2.0 * np.pi * v.astype(np.float64)
    c = lambda v: np.cos(ang(v)).astype(f)
    s = lambda v: np.sin(ang(v)).astype(f)
    z = np.stack([ra * c(u[..., 1]), ra * s(u[..., 1]), rb * c(u[..., 3]), rb * s(u[..., 3])], axis=-1).astype(f)
    return z.reshape(P, R, -1)[:, :, :n]


def _fma32(a, b, c):
    """float32 fma: the product is exact in double; the sum is rounded to double and then to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def sample(mean, var, seed, iteration, R, problem_offset=0, proj=None):
    """The definition in float64: x = mean + sqrt(var) N, then per group x <- A x + b.  mean, var [P, n]; proj = (A [G, g, g],
    b [P, n]) or None -> [P, R, n]"""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    P, n = mean.shape
    x = mean[:, None, :] + np.sqrt(var)[:, None, :] * normals(seed, iteration, P, R, n, problem_offset)
    if proj is not None:
        A, b = np.asarray(proj[0], dtype=np.float64), np.asarray(proj[1], dtype=np.float64)
        G, g = A.shape[0], A.shape[1]
        x = np.einsum("gjk,prgk->prgj", A, x.reshape(P, R, G, g)).reshape(P, R, n) + b[:, None, :]
    return x


def sample_restated(mean, var, seed, iteration, R, problem_offset=0, proj=None):
    """avae_search.h's k_search_sample in float32 -> float32 [P, R, n]"""
    f = np.float32
    mean, var = np.asarray(mean, dtype=f), np.asarray(var, dtype=f)
    P, n = mean.shape
    z = normals_f32(seed, iteration, P, R, n, problem_offset)
    sd = np.sqrt(var).astype(f)
    y = _fma32(np.broadcast_to(sd[:, None, :], z.shape), z, np.broadcast_to(mean[:, None, :], z.shape))
    if proj is None:
        return y
    A, b = np.asarray(proj[0], dtype=f), np.asarray(proj[1], dtype=f)
    G, g = A.shape[0], A.shape[1]
    yg = y.reshape(P, R, G, g)
    acc = np.broadcast_to(b.reshape(P, 1, G, g), yg.shape).astype(f)
    for k in range(g):
        acc = _fma32(np.broadcast_to(A[None, None, :, :, k], yg.shape), np.broadcast_to(yg[:, :, :, k:k + 1], yg.shape), acc)
    return acc.reshape(P, R, n)


# ---------------------------------------------------------------------------------------------------------------- update
def new_state(x0, var0):
    """The state of a run: float64 here, float32 on the device"""
    mean = np.array(x0, dtype=np.float64)
    P, n = mean.shape
    return dict(mean=mean, var=np.broadcast_to(np.asarray(var0, dtype=np.float64), (P, n)).copy(),
                n_applied=np.zeros(P, np.int32), frozen=np.zeros(P, np.int32), best_cost=np.full(P, np.inf),
                best_x=np.zeros((P, n)), iteration=0)


def _weights(c, ok, opt, mean_of, std_of):
    """unnormalised weights of one problem's costs c [R] (ok: the counting rollouts)"""
    w = np.zeros(len(c))
    cf = c[ok]
    cbar, sd = mean_of(cf), std_of(cf)
    if sd <= 1e-8 * abs(cbar):
        w[ok] = 1.0
        return w, cbar
    cmin, cmax = cf.min(), cf.max()
    if opt["weighting"] == PIBB:
        w[ok] = np.exp(-opt["eliteness"] * (cf - cmin) / ((cmax - cmin) + 1e-6))
        return w, cbar
    mu = int(opt["eliteness"])
    idx = np.nonzero(ok)[0]
    order = idx[np.argsort(cf, kind="stable")]                      # ties to the lower rollout
    for rank, r in enumerate(order[:mu]):
        w[r] = 1.0 / mu if opt["weighting"] == CEM else np.log(mu + 0.5) - np.log(rank + 1.0)
    return w, cbar


def _bounds(v, opt):
    if opt["abs_upper"] >= 0:
        v = np.where(v > opt["abs_upper"], opt["abs_upper"], v)
    lower = None
    if opt["abs_lower"] >= 0:
        lower = opt["abs_lower"]
    if opt["rel_lower"] >= 0:
        rel = opt["rel_lower"] * v.max()
        lower = rel if lower is None or rel > lower else lower
    if lower is not None:
        v = np.where(v < lower, lower, v)
    return v


def _update(x, cost, state, opt, restated):
    """One avae_search_update over every problem.  ``restated``: csrc/avae_search.h's order of every sum and float32 outputs; else
    NumPy's own sums and float64 outputs.  -> (new state, dict(avg_cost, min_cost, moved [P]))"""
    x, cost = np.asarray(x, dtype=np.float64), np.asarray(cost, dtype=np.float64)
    P, R, n = x.shape
    out_t = np.float32 if restated else np.float64
    st = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    hist = {k: np.full(P, np.nan, dtype=out_t) for k in ("avg_cost", "min_cost", "moved")}

    def tree(part):
        part = np.array(part, dtype=np.float64)
        s = THREADS // 2
        while s:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
        return part[0]

    def thread_sum(vals, idx, size):
        """values at positions idx (ascending) of a strided ownership: thread i owns i, i + 256, ... -> the tree of the partial sums"""
        part = np.zeros(THREADS)
        for v, i in zip(vals, idx):
            part[i % THREADS] = part[i % THREADS] + v
        return tree(part)

    for p in range(P):
        c = cost[p]
        ok = np.isfinite(c)
        F = int(ok.sum())
        if F:
            r_best = int(np.nonzero(ok)[0][np.argmin(c[ok])])      # (the first of equal minima)
            if c[r_best] < st["best_cost"][p]:
                st["best_cost"][p] = c[r_best]
                st["best_x"][p] = x[p, r_best]
        if F == 0 or st["frozen"][p]:
            continue
        idx = np.nonzero(ok)[0]
        if restated:
            mean_of = lambda cf: thread_sum(cf, idx, R) / F
            std_of = lambda cf: np.sqrt(thread_sum((cf - mean_of(cf)) ** 2, idx, R) / F)
        else:
            mean_of, std_of = np.mean, np.std
        w, cbar = _weights(c, ok, opt, mean_of, std_of)
        w = w / (thread_sum(w[ok], idx, R) if restated else w.sum())
        m0, v0 = st["mean"][p].astype(np.float64), st["var"][p].astype(np.float64)
        if restated:
            m1 = np.zeros(n)
            for r in range(R):
                if w[r] != 0.0:
                    m1 = m1 + w[r] * x[p, r]
            ctr = m1 if opt["cov_update"] == CEM else m0
            s = np.zeros(n)
            for r in range(R):
                if w[r] != 0.0:
                    e = x[p, r] - ctr
                    s = s + w[r] * (e * e)
        else:
            use = w != 0.0
            m1 = (w[use, None] * x[p, use]).sum(0)
            ctr = m1 if opt["cov_update"] == CEM else m0
            s = (w[use, None] * (x[p, use] - ctr) ** 2).sum(0)
        v1 = _bounds((1.0 - opt["lr"]) * v0 + opt["lr"] * s, opt)
        d2 = (m1 - m0) ** 2
        moved = np.sqrt(thread_sum(d2, range(n), n) if restated else d2.sum())
        st["mean"][p], st["var"][p] = m1.astype(out_t), v1.astype(out_t)
        st["n_applied"][p] += 1
        hist["avg_cost"][p], hist["min_cost"][p], hist["moved"][p] = cbar, c[ok].min(), moved
        if moved < opt["tol"]:
            st["frozen"][p] = 1
    return st, hist


def update(x, cost, state, opt):
    """The float64 definition of avae_search_update"""
    return _update(x, cost, state, opt, False)


def update_restated(x, cost, state, opt):
    """csrc/avae_search.h operation for operation: double arithmetic in the kernel's order, float32 state"""
    st = dict(state)
    for k in ("mean", "var", "best_cost", "best_x"):
        st[k] = np.asarray(state[k], dtype=np.float32)
    new, hist = _update(x, cost, st, opt, True)
    for k in ("mean", "var", "best_cost", "best_x"):
        new[k] = new[k].astype(np.float32)
    return new, hist


def search(cost_fn, x0, var0, n_rollouts=10, n_iters=10, opt=None, proj=None, seed=0, state=None, normals_fn=None):
    """The loop in float64 with the Philox stream (``normals_fn(P, R, n, iteration)`` replaces it): cost_fn maps [P, R, n] to
    [P, R].  -> (state, history dict of [n_iters, P])"""
    opt = options() if opt is None else opt
    st = new_state(x0, var0) if state is None else state
    P, n = st["mean"].shape
    hist = {k: [] for k in ("avg_cost", "min_cost", "moved")}
    for _ in range(n_iters):
        it = st["iteration"]
        if normals_fn is None:
            x = sample(st["mean"], st["var"], seed, it, n_rollouts, 0, proj)
        else:
            x = st["mean"][:, None, :] + np.sqrt(st["var"])[:, None, :] * normals_fn(P, n_rollouts, n, it)
        st, h = update(x, cost_fn(x), st, opt)
        st["iteration"] = it + 1
        for k in hist:
            hist[k].append(h[k])
    return st, {k: np.array(v).reshape(n_iters, P) for k, v in hist.items()}


# ---------------------------------------------------------------------------------------------------------------- cases
SAMPLE_SHAPES = [(1, 1, 1), (3, 10, 20), (2, 20, 147), (5, 7, 63), (2, 3, 1000)]
SAMPLE_GROUPS = {147: (7, 21), 1: (1, 1)}                               # n -> (G, g) of the cases run with a map
UPDATE_SHAPES = SAMPLE_SHAPES + [(2, 300, 1000), (1, 1024, 64)]
FAMILIES = ("spread", "equal", "two", "one_nan", "all_nan", "inf", "cem_ties")

# The classes k_search_sample's tiling distinguishes: a tile holds 1024 / (4 ceil(n / 4)) rows of P R.
#   (3, 100, 3)   256-row tiles, the one quad partial, a tile straddling three problems    (4, 1024, 2)  R = 1024, 16 such tiles
#   (2, 5, 1024)  256 full quads, one row a tile                                            (2, 3, 1021)  the last quad partial
#   (1, 7, 513)   129 quads: one row a tile, 508 floats of it idle                          (2, 9, 340)   a tile of 3 rows
#   (3, 6, 128)   8 rows a tile, g = 64 in 2 groups                                         (7, 50, 5)    g = 1 with G = n
#   (2, 17, 64)   G = 1 with g = n = 64
SAMPLE_CLASS_SHAPES = [(3, 100, 3), (4, 1024, 2), (2, 5, 1024), (2, 3, 1021), (1, 7, 513), (2, 9, 340), (3, 6, 128), (7, 50, 5),
                       (2, 17, 64)]
SAMPLE_CLASS_GROUPS = {1024: (16, 64), 128: (2, 64), 5: (5, 1), 64: (1, 64)}
# k_search_update: a thread owns the rollouts and the dimensions i, i + 256, ...: R and n at 255 / 256 / 257, both at 1024, n = 1
# under 255 rollouts, two rollouts under three dimensions a thread
UPDATE_CLASS_SHAPES = [(1, 257, 257), (3, 256, 256), (1, 1024, 1024), (2, 255, 1), (2, 2, 513)]


def option_grid():
    """every (family, weighting) pair twice: the covariance rule, the learning rate and the bounds alternate so that every value
    of each meets every weighting"""
    out = []
    for i, (family, (weighting, e)) in enumerate(itertools.product(FAMILIES, ((PIBB, 10.0), (CEM, 3), (CMAES, 3)))):
        for j in range(2):
            k = i + j
            bounds = dict(rel_lower=0.1, abs_lower=0.02, abs_upper=0.9) if (k // 2) % 2 == 0 else dict(rel_lower=-1.0)
            out.append((family, options(weighting=weighting, eliteness=e, cov_update=(PIBB, CEM)[j], lr=(1.0, 0.5)[k % 2],
                                        tol=1e-6, **bounds)))
    return out


def class_options():
    """[(family, options, rel)] run at every UPDATE_CLASS_SHAPES next to the grid of test_gpu_search.py.  ``rel`` is None or a
    factor: then ``abs_lower`` is to be set to rel_lower * vmax * rel, vmax the definition's own largest variance of problem 0 under
    the same options without an absolute floor (``with_abs_lower``), which puts rel_lower * vmax just below or just above it."""
    return [
        ("spread", options(weighting=PIBB, eliteness=2000.0), None),                # exp underflows: w == 0 under PI-BB
        ("spread", options(weighting=PIBB, eliteness=0.0, lr=0.5), None),           # every weight 1
        ("spread", options(weighting=CEM, eliteness=1, cov_update=CEM, rel_lower=-1.0, abs_lower=0.3), None),
        ("one_nan", options(weighting=CMAES, eliteness=4096, rel_lower=-1.0, abs_upper=0.2), None),    # mu >= R
        ("spread", options(lr=0.0, rel_lower=0.5), None),
        ("spread", options(rel_lower=0.0, abs_lower=0.0, abs_upper=0.0), None),
        ("spread", options(weighting=CEM, eliteness=3, lr=0.5, rel_lower=0.25), 1.0 + 1e-3),   # rel_lower * vmax just below abs_lower
        ("spread", options(weighting=CEM, eliteness=3, lr=0.5, rel_lower=0.25), 1.0 - 1e-3),   # ... just above
    ]


def with_abs_lower(x, cost, state, opt, rel):
    """``opt`` with the absolute floor ``class_options`` describes"""
    free, _ = update(x, cost, state, dict(opt, rel_lower=-1.0, abs_lower=-1.0))    # the variances behind the cap, before a floor
    assert free["n_applied"][0] == 1
    return dict(opt, abs_lower=float(opt["rel_lower"] * free["var"][0].max() * rel))


def costs(family, P, R, rng, mu=3):
    """float32 [P, R] of a family.  Spread costs are far from the 1e-8 threshold of the equal-cost test (relative spread ~0.3)"""
    c = (2.0 + rng.random((P, R))).astype(np.float32)
    if family == "equal":
        c[:] = np.float32(1.25)
    elif family == "two":
        c[:] = np.where(rng.random((P, R)) < 0.5, np.float32(1.5), np.float32(2.5))
        c[:, 0] = 1.5
        if R > 1:
            c[:, -1] = 2.5
    elif family == "one_nan":
        c[np.arange(P), rng.integers(0, R, P)] = np.nan
    elif family == "all_nan":
        c[P // 2] = np.nan                                              # (the other problems stay spread)
    elif family == "inf":
        c[np.arange(P), rng.integers(0, R, P)] = np.inf
        if R > 1:
            c[0, (R - 1) // 2] = -np.inf
    elif family == "cem_ties":
        if R > mu:                                                      # the mu-th and (mu + 1)-th lowest are equal
            order = np.argsort(c, axis=1, kind="stable")
            for p in range(P):
                c[p, order[p, mu]] = c[p, order[p, mu - 1]]
    return c


def update_case(P, R, n, family, rng, mu=3):
    """-> (x [P, R, n] float32, cost [P, R] float32, state with float32-valued fields)"""
    mean = rng.standard_normal((P, n)).astype(np.float32)
    var = (0.05 + rng.random((P, n))).astype(np.float32)
    x = (mean[:, None, :] + np.sqrt(var)[:, None, :] * rng.standard_normal((P, R, n))).astype(np.float32)
    st = new_state(mean, var)
    st["best_cost"] = np.where(rng.random(P) < 0.5, np.inf, 2.4).astype(np.float32).astype(np.float64)
    st["best_x"] = np.full((P, n), -7.0)
    return x, costs(family, P, R, rng, mu), st
