"""The definition of ``aggregate_log_density`` and ``elbo_decomposition`` (avae_agg_logpdf in include/avae.h, DESIGN.md section
20), for the tests.

With c = 0.5 log(2 pi), E_n the gallery rows counted for query n (every row, minus row exclude[n] when it is one) and G' = |E_n|:

    l(n,g,j)      = -0.5 (lv_gj + (z_nj - mu_gj)^2 exp(-lv_gj))
    marginal[n,j] = log sum_{g in E_n} exp(l(n,g,j))        - log G' - c
    joint[n]      = log sum_{g in E_n} exp(sum_j l(n,g,j))  - log G' - n_z c

``logpdf64`` is that in float64, a max-shifted log-sum-exp over the whole gallery.  ``logpdf32`` restates it in NumPy float32 in
the operation order include/avae.h states (iv = exp(-lv), d = z - mu, l = -0.5 * (d*d*iv + lv) with every product and sum rounded,
no fused multiply-add; the joint exponent added over j in index order from +0.0; the sum of exp(l - max) over the gallery rows in
row order in float32; log G' and the constant subtracted in float64, one rounding).  ``decomposition64`` is the ELBO decomposition
KL = MI + TC + sum_j dimension-wise KL built on ``logpdf64``."""
import numpy as np

C = 0.5 * np.log(2.0 * np.pi)


def latents(rng, rows, nz):
    """The tests' random posteriors: mu ~ N(0, 1), lv ~ U(-6, 1), float32"""
    return rng.standard_normal((rows, nz)).astype(np.float32), rng.uniform(-6.0, 1.0, (rows, nz)).astype(np.float32)


def queries(rng, gallery, n=19):
    """The standard query set of a gallery: of every 19 queries 12 are samples of gallery rows' own posteriors (where the mixture
    has its mass) and 7 are draws from N(0, 9) (mostly far from every component) -> float32 [n, nz]; the far ones come last"""
    mu, lv = gallery
    G, nz = mu.shape
    far = (7 * n) // 19
    own = n - far
    rows = rng.integers(0, G, own)
    z_own = mu[rows].astype(np.float64) + np.exp(0.5 * lv[rows].astype(np.float64)) * rng.standard_normal((own, nz))
    z_far = 3.0 * rng.standard_normal((far, nz))
    return np.concatenate([z_own, z_far]).astype(np.float32)


def _counted(N, G, exclude):
    """[N, G] bool: gallery row g counts for query n"""
    keep = np.ones((N, G), bool)
    if exclude is not None:
        ex = np.asarray(exclude).astype(np.int64)
        hit = (ex >= 0) & (ex < G)
        keep[np.nonzero(hit)[0], ex[hit]] = False
    return keep


def _lse(x, keep, axis):
    """log sum exp over ``axis`` of the kept entries (dropped ones are selected away, whatever they hold), max-shifted; -inf where
    every kept entry is -inf"""
    x = np.where(keep, x, -np.inf)
    m = np.max(np.where(np.isnan(x), -np.inf, x), axis=axis, keepdims=True, initial=-np.inf)
    shift = np.where(np.isneginf(m), 0.0, m)
    s = np.exp(x - shift).sum(axis=axis, keepdims=True)
    return np.squeeze(np.log(s) + shift, axis)


def logpdf64(z, gallery, exclude=None):
    """(joint [N], marginal [N, nz]) in float64"""
    mu, lv = (np.asarray(a).astype(np.float64) for a in gallery)
    z = np.asarray(z).astype(np.float64)
    N, G, nz = z.shape[0], mu.shape[0], z.shape[1]
    keep = _counted(N, G, exclude)
    with np.errstate(all="ignore"):
        d = z[:, None, :] - mu[None]
        l = -0.5 * (lv[None] + d * d * np.exp(-lv)[None])                    # [N, G, nz]
        n_counted = keep.sum(1).astype(np.float64)
        log_g = np.where(n_counted > 0, np.log(np.maximum(n_counted, 1.0)), np.nan)
        joint = _lse(l.sum(-1), keep, 1) - log_g - nz * C
        marginal = _lse(l, keep[:, :, None], 1) - log_g[:, None] - C
    return joint, marginal


def logpdf32(z, gallery, exclude=None):
    """The same in float32, operation by operation -> (joint [N], marginal [N, nz]) float32"""
    f = np.float32
    mu, lv = (np.asarray(a).astype(f) for a in gallery)
    z = np.asarray(z).astype(f)
    N, G, nz = z.shape[0], mu.shape[0], z.shape[1]
    keep = _counted(N, G, exclude)
    with np.errstate(all="ignore"):
        iv = np.exp(-lv)
        d = z[:, None, :] - mu[None]
        l = f(-0.5) * ((d * d) * iv[None] + lv[None])                        # [N, G, nz]
        assert l.dtype == f
        lj = np.zeros((N, G), f)
        for j in range(nz):
            lj = lj + l[:, :, j]
        cols = np.concatenate([lj[:, :, None], l], axis=2)                    # column 0: the joint exponent
        cols = np.where(keep[:, :, None], cols, f(-np.inf))
        m = np.max(np.where(np.isnan(cols), f(-np.inf), cols), axis=1, initial=f(-np.inf))      # [N, 1 + nz]
        shift = np.where(np.isneginf(m), f(0), m)
        s = np.zeros((N, 1 + nz), f)
        for g in range(G):
            s = s + np.exp(cols[:, g, :] - shift)
        assert s.dtype == f
        n_counted = keep.sum(1).astype(np.float64)
        log_g = np.where(n_counted > 0, np.log(np.maximum(n_counted, 1.0)), np.nan)[:, None]
        const = np.concatenate([[nz * C], np.full(nz, C)])[None]
        out = (np.log(s.astype(np.float64)) + shift.astype(np.float64) - log_g - const).astype(f)
    return out[:, 0], out[:, 1:]


def joint_err(got, ref, nz):
    """the error measure of the joint: |err| / (|ref| + n_z)"""
    return np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + nz)


def marginal_err(got, ref):
    """... and of a marginal: |err| / (|ref| + 1)"""
    return np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1.0)


def decomposition64(posteriors, eps, leave_one_out=False):
    """The ELBO decomposition in float64.  ``posteriors``: list over modalities of (mu, logvar) [N, nz] or None; ``eps``
    [S, N, nz], shared by the modalities.  Returns the dict ``elbo_decomposition`` documents, plus ``scale [M]``: the mean of
    |log q_agg^m(z^m)| + n_z, what a tolerance on the entries of modality m is relative to, and ``cross_scale [M, M]``: the mean of
    |log q_agg^d(z^s)| + n_z, the same for ``cross[s, d]``."""
    eps = np.asarray(eps).astype(np.float64)
    S, N, nz = eps.shape
    M = len(posteriors)
    out = {"kl": np.full(M, np.nan), "mi": np.full(M, np.nan), "tc": np.full(M, np.nan), "dimwise_kl": np.full((M, nz), np.nan),
           "marginal_kl": np.full(M, np.nan), "cross": np.full((M, M), np.nan), "log_n": float(np.log(N)), "scale": np.full(M, np.nan),
           "cross_scale": np.full((M, M), np.nan)}
    own = np.tile(np.arange(N), S) if leave_one_out else None
    for s, post in enumerate(posteriors):
        if post is None:
            continue
        mu, lv = (np.asarray(a).astype(np.float64) for a in post)
        z = (mu[None] + np.exp(0.5 * lv)[None] * eps).reshape(S * N, nz)
        log_q = (-0.5 * eps * eps - 0.5 * lv[None] - C).sum(-1).reshape(S * N)
        log_pj = -0.5 * z * z - C
        joint, marginal = logpdf64(z, post, own)
        out["kl"][s] = (log_q - log_pj.sum(-1)).mean()
        out["mi"][s] = (log_q - joint).mean()
        out["tc"][s] = (joint - marginal.sum(-1)).mean()
        out["dimwise_kl"][s] = (marginal - log_pj).mean(0)
        out["marginal_kl"][s] = out["tc"][s] + out["dimwise_kl"][s].sum()
        out["scale"][s] = (np.abs(joint) + nz).mean()
        for d, other in enumerate(posteriors):
            if other is not None:
                under_d = joint if d == s else logpdf64(z, other, own)[0]
                out["cross"][s, d] = 0.0 if d == s else (joint - under_d).mean()
                out["cross_scale"][s, d] = (np.abs(under_d) + nz).mean()
    return out
