"""NumPy reference of the 2-D t-SNE map of the posteriors (include/avae.h, avae_embed_calibrate / avae_embed_iterate; DESIGN.md
section 22): the float64 definition, a float32 restatement of it (every operation in float32, sums included), the error measures
and helpers of tests/test_embed_cpu.py and tests/test_gpu_embed.py.

Rows are q_n = N(mu_n, diag exp(lv_n)) (lv None: points, metric "l2").  D_ij is avae_latent_topk's metric.  A row with a
non-finite entry is skipped; F is the number of used rows.  Per used row i
    m_i = min_{j != i} D_ij, e_ij = exp(-beta_i (D_ij - m_i)), S0_i = sum_{j != i} e_ij, S1_i = sum (D_ij - m_i) e_ij,
    H_i = log S0_i + beta_i S1_i / S0_i
with beta_i searched from 1 (double / halve while that side has no bound, else bisect) until |H_i - log(perplexity)| <= tol or
max_tries values were tried.  p_ij = (e_ij / S0_i + e_ji / S0_j) / (2 F), w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
    A_i = sum_j p_ij w_ij (y_i - y_j), R_i = sum_j w_ij^2 (y_i - y_j), grad_i = 4 (alpha A_i - R_i / Z),
    KL = sum_{p > 0} p_ij (log p_ij - log w_ij) + log Z.
The update is van der Maaten's (gains +0.2 / x0.8, floor 0.01, momentum); the state (y, vel, gain) is float32 between iterations."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SYMKL, L2 = "symkl", "l2"
BETA_MAX, BETA_MIN = 2.0 ** 100, 2.0 ** -100


# ------------------------------------------------------------------------------------------------ rows and distances
def used_rows(mu, lv, metric):
    ok = np.isfinite(mu).all(axis=1)
    if metric == SYMKL:
        ok &= np.isfinite(lv).all(axis=1)
    return ok


def _clean(mu, lv, metric, dtype):
    """the rows as ``dtype`` with the skipped rows' entries replaced by 0 (they are selected away everywhere)"""
    ok = used_rows(mu, lv, metric)
    m = np.where(ok[:, None], mu, 0).astype(dtype)
    l = None if metric == L2 else np.where(ok[:, None], lv, 0).astype(dtype)
    return m, l, ok


BLOCK = 256         # rows worked on at a time: the [BLOCK, N] temporaries stay in the cache (the arithmetic does not depend on it)


def _blocks(fn, N):
    """fn(row indices) for every block of BLOCK rows, in row order; NumPy's loops release the interpreter, so the blocks of a large
    problem run on a few threads (what a block computes does not depend on that)"""
    parts = [np.arange(r0, min(N, r0 + BLOCK)) for r0 in range(0, N, BLOCK)]
    if len(parts) < 4:
        return [fn(r) for r in parts]
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        return list(pool.map(fn, parts))


def _distances(mu, lv, metric, dtype):
    m, l, ok = _clean(mu, lv, metric, dtype)
    N, nz = m.shape
    D = np.empty((N, N), dtype)
    if metric == SYMKL:
        v, iv = np.exp(l), np.exp(-l)

    def block(r):
        acc = np.zeros((len(r), N), dtype)
        for j in range(nz):
            d = m[r, None, j] - m[None, :, j]
            if metric == L2:
                acc = acc + d * d
            else:
                t = v[r, None, j] - v[None, :, j]
                acc = acc + (t * iv[r, None, j]) * (t * iv[None, :, j])
                acc = acc + (d * d) * (iv[r, None, j] + iv[None, :, j])
        D[r] = acc if metric == L2 else dtype(0.5) * acc
    _blocks(block, N)
    assert D.dtype == dtype
    return D, ok


def distances64(mu, lv, metric):
    """-> (D [N, N] float64, used [N] bool): avae_latent_topk's chain over the dimensions in index order; entries of skipped rows
    are finite and meaningless"""
    return _distances(mu, lv, metric, np.float64)


def distances32(mu, lv, metric):
    """the same chain with every operation in float32 (no fused multiply-add)"""
    return _distances(mu, lv, metric, np.float32)


def _row_sums(x, dtype):
    """the sums along the rows of ``x`` in ``dtype``.  The float32 restatement adds one term after the other in index order (a
    running float32 sum, as tests/latent_prior_reference.py does: np.sum would add pairwise, which is more accurate than any
    float32 loop); the float64 definition is not sensitive to the order"""
    if dtype == np.float32:
        return np.cumsum(x, axis=1, dtype=dtype)[:, -1]
    return x.sum(axis=1, dtype=dtype)


def _total(x, dtype):
    """the sum of a vector, in the same way"""
    if dtype == np.float32:
        return dtype(np.cumsum(x, dtype=dtype)[-1]) if len(x) else dtype(0)
    return x.sum(dtype=dtype)


def pair_mask(ok):
    """[N, N] bool: both rows used and i != j"""
    on = ok[:, None] & ok[None, :]
    np.fill_diagonal(on, False)
    return on


# ------------------------------------------------------------------------------------------------ calibration
def entropy(D, ok, beta, shift, dtype=np.float64, rows=None):
    """-> (H [N], S0 [N]) of the given beta and shift, in ``dtype``; NaN on skipped rows (and, with ``rows`` [N] bool, on the rows
    left out: only the others are evaluated)"""
    if rows is not None:
        H, s0 = np.full(len(ok), np.nan, dtype), np.full(len(ok), np.nan, dtype)
        pick = np.flatnonzero(rows)
        on = ok[pick, None] & ok[None, :]
        on[np.arange(len(pick)), pick] = False
        h, s = _entropy(D[pick], on, np.asarray(beta)[pick], np.asarray(shift)[pick], dtype)
        H[pick], s0[pick] = np.where(ok[pick], h, np.nan), np.where(ok[pick], s, np.nan)
        return H, s0
    H, s0 = _entropy(D, pair_mask(ok), beta, shift, dtype)
    H[~ok] = np.nan
    return H, np.where(ok, s0, dtype(np.nan)).astype(dtype)


def _entropy(D, on, beta, shift, dtype):
    t = D.astype(dtype) - np.asarray(shift, dtype)[:, None]
    b = np.asarray(beta, dtype)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.where(on, np.exp(-(b * t)), dtype(0))
        s0 = _row_sums(e, dtype)
        s1 = _row_sums(np.where(on, t * e, dtype(0)), dtype)
        H = np.log(s0) + b[:, 0] * s1 / s0
    return H.astype(dtype), s0.astype(dtype)


def calibrate(D, ok, perplexity, tol=1e-5, max_tries=64, dtype=np.float64):
    """the search of every row (rows are independent: worked on in blocks of BLOCK) -> (beta, shift, norm in ``dtype``, tries int32);
    NaN / 0 on skipped rows and when F < 2.  ``dtype`` float64 is the definition, float32 its restatement (every operation up to H
    in float32; only the comparison with the target is made in float64)"""
    N = D.shape[0]
    out = [np.empty(N, dtype), np.empty(N, dtype), np.empty(N, dtype), np.empty(N, np.int32)]

    def block(r):
        for o, x in zip(out, _calibrate_rows(D[r], r, ok, perplexity, tol, max_tries, dtype)):
            o[r] = x
    _blocks(block, N)
    return tuple(out)


def _calibrate_rows(D, rows, ok, perplexity, tol, max_tries, dtype):
    """``D`` holds the rows ``rows`` of the distance matrix"""
    n = len(rows)
    nan = dtype(np.nan)
    live = ok[rows] & (ok.sum() >= 2)
    on = ok[rows, None] & ok[None, :]
    on[np.arange(n), rows] = False
    shift = np.where(live, np.where(on, D, np.inf).min(axis=1, initial=np.inf), nan).astype(dtype)
    beta = np.where(live, dtype(1), nan).astype(dtype)
    lo, hi = np.zeros(n, dtype), np.full(n, np.inf, dtype)
    norm = np.full(n, nan, dtype)
    tries = np.zeros(n, np.int32)
    done = ~live
    target = np.log(np.float64(perplexity))
    for _ in range(max_tries):
        if done.all():
            break
        run = ~done
        H, s0 = np.full(n, np.nan, dtype), np.full(n, np.nan, dtype)
        H[run], s0[run] = _entropy(D[run], on[run], beta[run], shift[run], dtype)
        diff = H.astype(np.float64) - target
        tries[run] += 1
        stop = run & ((np.abs(diff) <= tol) | (tries >= max_tries) | np.isnan(diff))
        norm[stop] = s0[stop]
        done |= stop
        up, down = run & ~stop & (diff > 0), run & ~stop & ~(diff > 0)
        lo[up] = beta[up]
        hi[down] = beta[down]
        with np.errstate(over="ignore", invalid="ignore"):
            nb = beta.copy()
            nb[up] = np.where(np.isinf(hi[up]), np.minimum(beta[up] * dtype(2), dtype(BETA_MAX)), (beta[up] + hi[up]) * dtype(0.5))
            nb[down] = np.where(lo[down] == 0, np.maximum(beta[down] * dtype(0.5), dtype(BETA_MIN)), (beta[down] + lo[down]) * dtype(0.5))
        beta = nb.astype(dtype)
    return beta, shift, norm, tries


# ------------------------------------------------------------------------------------------------ affinities and forces
def affinities(D, ok, beta, shift, norm, dtype=np.float64):
    """p_ij in ``dtype`` from a calibration (its arrays are taken as given, cast to ``dtype``); 0 on skipped rows and the diagonal"""
    on = pair_mask(ok)
    F = int(ok.sum())
    b, m, s0 = (np.where(ok, np.asarray(x, dtype), dtype(1))[:, None] for x in (beta, shift, norm))
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-(b * (D.astype(dtype) - m)))
        c = dtype(1) / (dtype(2 * F) * s0)
        ec = e * c
        P = np.where(on, ec + ec.T, dtype(0))
    assert P.dtype == dtype
    return P


def forces(P, Y, ok, dtype=np.float64):
    """-> (A [N, 2], R [N, 2], Z, KL) in ``dtype`` (sums in ``dtype`` too: along a row, then over the rows); Y is taken as given,
    cast to ``dtype``"""
    N = len(ok)
    y = np.where(ok[:, None], np.asarray(Y, dtype), dtype(0))
    A, R, zrow, krow = np.empty((N, 2), dtype), np.empty((N, 2), dtype), np.empty(N, dtype), np.empty(N, dtype)

    def block(r):
        on = ok[r, None] & ok[None, :]
        on[np.arange(len(r)), r] = False
        p = P[r]
        d0 = np.where(on, y[r, None, 0] - y[None, :, 0], dtype(0))
        d1 = np.where(on, y[r, None, 1] - y[None, :, 1], dtype(0))
        q = (dtype(1) + d0 * d0) + d1 * d1
        w = np.where(on, dtype(1) / q, dtype(0))
        pw, ww = p * w, w * w
        A[r, 0], A[r, 1] = _row_sums(pw * d0, dtype), _row_sums(pw * d1, dtype)
        R[r, 0], R[r, 1] = _row_sums(ww * d0, dtype), _row_sums(ww * d1, dtype)
        zrow[r] = _row_sums(w, dtype)
        pos = p > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            krow[r] = _row_sums(np.where(pos, p * (np.log(np.where(pos, p, dtype(1))) + np.log(q)), dtype(0)), dtype)
    _blocks(block, N)
    Z = _total(zrow, dtype)
    KL = _total(krow, dtype) + np.log(Z)
    return A, R, dtype(Z), dtype(KL)


def kl_of(P, Y, ok):
    return float(forces(P, Y, ok)[3])


def gradient(P, Y, ok, alpha=1.0, dtype=np.float64):
    A, R, Z, KL = forces(P, Y, ok, dtype)
    g = dtype(4) * (dtype(alpha) * A - R / Z)
    g[~ok] = np.nan
    return g.astype(dtype), KL


def schedule(t, early_exaggeration, exaggeration_iters, momentum):
    """(alpha, momentum) of the absolute iteration number t"""
    return (early_exaggeration, momentum[0]) if t < exaggeration_iters else (1.0, momentum[1])


def update(grad, y, vel, gain, lr, mom, dtype=np.float64):
    """one update of the float32 state (y, vel, gain) from ``grad``, evaluated in ``dtype`` -> new float32 (y, vel, gain); skipped
    rows (grad NaN) come back NaN"""
    f = np.float32
    g = np.asarray(grad, dtype)
    y, vel, gain = (np.asarray(x, f).astype(dtype) for x in (y, vel, gain))
    with np.errstate(invalid="ignore"):
        up = (g > 0) != (vel > 0)
        gain = np.where(up, gain + dtype(0.2), gain * dtype(0.8))
        gain = np.maximum(gain, dtype(0.01)).astype(f)
        vel = (dtype(f(mom)) * vel - (dtype(f(lr)) * gain.astype(dtype)) * g).astype(f)
        y = (y + vel.astype(dtype)).astype(f)
    bad = np.isnan(g)
    y[bad], vel[bad], gain[bad] = np.nan, np.nan, np.nan
    return y, vel, gain


def step64(D, ok, cal, y, vel, gain, alpha, mom, lr):
    """one pass of the definition from a calibration ``cal`` = (beta, shift, norm) taken as given -> (grad [N, 2], kl float64, the
    updated float32 (y, vel, gain))"""
    g, kl = gradient(affinities(D, ok, *cal), y, ok, alpha)
    return g, float(kl), update(g, y, vel, gain, lr, mom)


def step32(D32, ok, cal, y, vel, gain, alpha, mom, lr):
    """the same with every operation in float32, the float32 distances included"""
    f = np.float32
    g, kl = gradient(affinities(D32, ok, *cal, dtype=f), y, ok, f(alpha), f)
    return g, float(kl), update(g, y, vel, gain, lr, mom, f)


def iterate(P, ok, y, vel, gain, it0, n_iters, lr, early_exaggeration=12.0, exaggeration_iters=250, momentum=(0.5, 0.8),
            center=True, dtype=np.float64):
    """the loop on a given P -> (y, vel, gain float32, kl [n_iters + 1] float64, grads list of [N, 2] per pass).  ``dtype``
    float64 is the definition; float32 restates every operation (P must then be float32 too)"""
    f = np.float32
    y, vel, gain = (np.array(x, f) for x in (y, vel, gain))
    kl, grads = np.empty(n_iters + 1), []
    for s in range(n_iters):
        alpha, mom = schedule(it0 + s, f(early_exaggeration), exaggeration_iters, momentum)
        g, kl[s] = gradient(P, y, ok, alpha, dtype)
        grads.append(g)
        y, vel, gain = update(g, y, vel, gain, lr, mom, dtype)
    alpha, _ = schedule(it0 + n_iters, f(early_exaggeration), exaggeration_iters, momentum)
    g, kl[n_iters] = gradient(P, y, ok, alpha, dtype)
    grads.append(g)
    if center and n_iters > 0 and ok.sum() >= 2:
        mean = y[ok].astype(np.float64).mean(axis=0)
        y[ok] = (y[ok].astype(np.float64) - mean).astype(f)
    return y, vel, gain, kl, grads


def embed(mu, lv, metric=SYMKL, perplexity=30.0, n_iters=1000, learning_rate="auto", early_exaggeration=12.0,
          exaggeration_iters=250, momentum=(0.5, 0.8), seed=0, dtype=np.float64):
    """end to end in ``dtype`` -> dict(embedding, kl, beta, tries, P)"""
    D, ok = (distances64 if dtype == np.float64 else distances32)(mu, lv, metric)
    beta, shift, norm, tries = calibrate(D, ok, perplexity, dtype=dtype)
    P = affinities(D, ok, beta, shift, norm, dtype)
    N, F = mu.shape[0], int(ok.sum())
    lr = max(F / 48.0, 50.0) if learning_rate == "auto" else learning_rate
    y0 = np.random.default_rng(seed).normal(0.0, 1e-4, (N, 2)).astype(np.float32)
    y, vel, gain, kl, _ = iterate(P, ok, y0, np.zeros((N, 2), np.float32), np.ones((N, 2), np.float32), 0, n_iters, lr,
                                  early_exaggeration, exaggeration_iters, momentum, True, dtype)
    return {"embedding": y, "kl": kl, "beta": beta, "tries": tries, "P": P}


# ------------------------------------------------------------------------------------------------ measures
def nearest(Y, k=1):
    """indices [N, k] of every point's k nearest other points in the map"""
    y = np.asarray(Y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def purity(Y, label):
    """share of the points whose nearest map neighbour has their own label"""
    return float((label[nearest(Y)[:, 0]] == label).mean())


def rel_max(got, ref):
    """|err| relative to max |ref| over the used entries"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), ~fin), "NaN exactly on the skipped rows"
    if not fin.any():
        return 0.0
    return float(np.abs(got[fin] - ref[fin]).max() / np.abs(ref[fin]).max())


def kl_err(got, ref):
    """|err| / (|ref| + 1)"""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1.0)))
