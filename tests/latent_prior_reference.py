"""NumPy reference of the mixture prior (include/avae.h, avae_gmm_fit / avae_gmm_score): the float64
definition, a float32 restatement of it (every operation in float32, sums included), the error measures and the seeded input
families of tests/test_latent_prior_cpu.py and tests/test_gpu_latent_prior.py.

The data are posteriors q_n = N(mu_n, diag v_n), v_n = exp(lv_n) (lv None: points, v = 0); the model is
p(z) = sum_k pi_k N(z; m_k, diag exp(s_k)).  One iteration over the used rows (a row with a non-finite entry is skipped):
    E_nk = log pi_k - 1/2 sum_j [log 2pi + s_kj + ((mu_nj - m_kj)^2 + v_nj) exp(-s_kj)]
    ll_n = logsumexp_k E_nk, r_nk = exp(E_nk - ll_n), bound = mean ll_n
    R_k = sum r_nk, S1_kj = sum r_nk (mu_nj - m_kj), S2_kj = sum r_nk ((mu_nj - m_kj)^2 + v_nj)
    pi_k = R_k / sum R, m'_kj = m_kj + S1_kj / R_k, s'_kj = log max(S2_kj / R_k - (S1_kj / R_k)^2, var_floor)
A component with R_k < 1e-8 keeps its mean and log-variance.  Parameters are float32 between iterations."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))
DEAD = 1e-8


# ------------------------------------------------------------------------------------------------ inputs
def clusters(rng, N, n_z, K, sep):
    """N posteriors around K centres ~ N(0, sep^2): within-cluster scale U(0.3, 1) per (k, j), lv ~ U(-6, 1) (the latent range
    the sibling tests use) -> (mu, lv) float32 and the labels"""
    centres = sep * rng.standard_normal((K, n_z))
    scale = rng.uniform(0.3, 1.0, size=(K, n_z))
    label = rng.integers(0, K, size=N)
    mu = centres[label] + scale[label] * rng.standard_normal((N, n_z))
    lv = rng.uniform(-6.0, 1.0, size=(N, n_z))
    return mu.astype(np.float32), lv.astype(np.float32), label


def with_offset(mu, offset=1e3):
    """the large-offset family: the same data plus ``offset`` on every mean"""
    return (mu.astype(np.float64) + offset).astype(np.float32)


def start(rng, mu, lv, K):
    """initial parameters for a test: K distinct rows of mu as means, the per-dimension total variance as every variance, weights
    slightly uneven (so that log pi matters) -> dict of float32 arrays"""
    N, nz = mu.shape
    rows = rng.permutation(N)[:K] if K <= N else rng.integers(0, N, size=K)
    means = mu[rows].astype(np.float64) + (0.0 if K <= N else 0.5 * rng.standard_normal((K, nz)))
    v = np.zeros_like(mu, dtype=np.float64) if lv is None else np.exp(lv.astype(np.float64))
    tot = mu.astype(np.float64).var(axis=0) + v.mean(axis=0) + 0.05
    w = rng.uniform(0.5, 1.5, size=K)
    return {"weights": (w / w.sum()).astype(np.float32), "means": means.astype(np.float32),
            "logvars": np.tile(np.log(tot), (K, 1)).astype(np.float32)}


def used_rows(mu, lv):
    ok = np.isfinite(mu).all(axis=1)
    if lv is not None:
        ok &= np.isfinite(lv).all(axis=1)
    return ok


# ------------------------------------------------------------------------------------------------ float64 definition
def estep64(mu, lv, prior):
    """-> (ll [N], r [N, K]) float64; NaN on skipped rows"""
    ok = used_rows(mu, lv)
    x = mu[ok].astype(np.float64)
    v = np.zeros_like(x) if lv is None else np.exp(lv[ok].astype(np.float64))
    w, m, s = (np.asarray(prior[k], np.float64) for k in ("weights", "means", "logvars"))
    d = x[:, None, :] - m[None]
    with np.errstate(divide="ignore"):
        E = np.log(w)[None] - 0.5 * (LOG_2PI + s[None] + (d * d + v[:, None, :]) * np.exp(-s)[None]).sum(axis=2)
    mx = E.max(axis=1, keepdims=True)
    ll_ok = mx[:, 0] + np.log(np.exp(E - mx).sum(axis=1))
    r_ok = np.exp(E - ll_ok[:, None])
    ll = np.full(mu.shape[0], np.nan)
    r = np.full((mu.shape[0], w.shape[0]), np.nan)
    ll[ok], r[ok] = ll_ok, r_ok
    return ll, r


def step64(mu, lv, prior, var_floor=1e-6):
    """one EM iteration in float64 -> (new prior rounded to float32, bound of the prior that came in, n_used)"""
    ok = used_rows(mu, lv)
    n = int(ok.sum())
    if n == 0:
        return {k: np.asarray(prior[k], np.float32).copy() for k in ("weights", "means", "logvars")}, float("nan"), 0
    ll, r = estep64(mu, lv, prior)
    ll, r = ll[ok], r[ok]
    x = mu[ok].astype(np.float64)
    v = np.zeros_like(x) if lv is None else np.exp(lv[ok].astype(np.float64))
    m, s = np.asarray(prior["means"], np.float64), np.asarray(prior["logvars"], np.float64)
    d = x[:, None, :] - m[None]
    R = r.sum(axis=0)
    S1 = (r[:, :, None] * d).sum(axis=0)
    S2 = (r[:, :, None] * (d * d + v[:, None, :])).sum(axis=0)
    live = R >= DEAD
    Rs = np.where(live, R, 1.0)[:, None]
    mean = m + S1 / Rs
    var = np.maximum(S2 / Rs - (S1 / Rs) ** 2, var_floor)
    out = {"weights": (R / R.sum()).astype(np.float32),
           "means": np.where(live[:, None], mean, m).astype(np.float32),
           "logvars": np.where(live[:, None], np.log(var), s).astype(np.float32)}
    return out, float(ll.mean()), n


def fit64(mu, lv, prior, n_iters, var_floor=1e-6):
    """-> (prior after n_iters iterations, bound [n_iters + 1] float64, n_used)"""
    bound = np.empty(n_iters + 1)
    for t in range(n_iters):
        prior, bound[t], _ = step64(mu, lv, prior, var_floor)
    ok = used_rows(mu, lv)
    bound[n_iters] = estep64(mu, lv, prior)[0][ok].mean() if ok.any() else np.nan
    return prior, bound, int(ok.sum())


def textbook_step(x, prior):
    """diagonal-covariance EM for points the textbook way (raw moments) -> (weights, means, variances) float64"""
    _, r = estep64(x, None, prior)
    x = x.astype(np.float64)
    R = r.sum(axis=0)
    mean = (r.T @ x) / R[:, None]
    var = (r.T @ (x * x)) / R[:, None] - mean * mean
    return R / x.shape[0], mean, var


# ------------------------------------------------------------------------------------------------ float32 restatement
def estep32(mu, lv, prior):
    """the definition with every operation in float32 -> (ll [N], r [N, K]) float32; NaN on skipped rows"""
    f = np.float32
    ok = used_rows(mu, lv)
    x = mu[ok].astype(f)
    v = np.zeros_like(x) if lv is None else np.exp(lv[ok].astype(f))
    w, m, s = (np.asarray(prior[k], f) for k in ("weights", "means", "logvars"))
    K, nz = m.shape
    hiv = f(-0.5) * np.exp(-s)
    acc = np.zeros(K, f)
    for j in range(nz):
        acc = acc + (s[:, j] + f(LOG_2PI))
    with np.errstate(divide="ignore"):
        E = np.tile(np.log(w) - f(0.5) * acc, (x.shape[0], 1)).astype(f)
    for j in range(nz):
        d = x[:, j, None] - m[None, :, j]
        E = E + (d * d + v[:, j, None]) * hiv[None, :, j]
    mx = E.max(axis=1)
    p = np.exp(E - mx[:, None])
    tot = np.zeros(x.shape[0], f)
    for k in range(K):
        tot = tot + p[:, k]
    ll = np.full(mu.shape[0], np.nan, f)
    r = np.full((mu.shape[0], K), np.nan, f)
    ll[ok], r[ok] = mx + np.log(tot), p / tot[:, None]
    assert ll.dtype == f and r.dtype == f
    return ll, r


def step32(mu, lv, prior, var_floor=1e-6):
    """one EM iteration with every operation in float32, the sums over the rows in row order -> (new prior, bound, n_used)"""
    f = np.float32
    ok = used_rows(mu, lv)
    n = int(ok.sum())
    if n == 0:
        return {k: np.asarray(prior[k], f).copy() for k in ("weights", "means", "logvars")}, f("nan"), 0
    ll, r = estep32(mu, lv, prior)
    ll, r = ll[ok], r[ok]
    x = mu[ok].astype(f)
    v = np.zeros_like(x) if lv is None else np.exp(lv[ok].astype(f))
    m, s = np.asarray(prior["means"], f), np.asarray(prior["logvars"], f)
    K, nz = m.shape
    d = x[:, None, :] - m[None]
    # the rows one after the other, in float32 (a running sum; np.sum would add pairwise along a contiguous axis)
    R = np.cumsum(r, axis=0, dtype=f)[-1]
    S1 = np.cumsum(r[:, :, None] * d, axis=0, dtype=f)[-1]
    S2 = np.cumsum(r[:, :, None] * (d * d + v[:, None, :]), axis=0, dtype=f)[-1]
    sll = np.cumsum(ll, dtype=f)[-1]
    live = R >= f(DEAD)
    Rs = np.where(live, R, f(1))[:, None]
    tot = f(0)
    for k in range(K):
        tot = tot + R[k]
    q = S1 / Rs
    var = np.maximum(S2 / Rs - q * q, f(var_floor))
    out = {"weights": R / tot, "means": np.where(live[:, None], m + q, m), "logvars": np.where(live[:, None], np.log(var), s)}
    assert all(a.dtype == f for a in out.values())
    return out, sll / f(n), n


def fit32(mu, lv, prior, n_iters, var_floor=1e-6):
    bound = np.empty(n_iters + 1, np.float32)
    for t in range(n_iters):
        prior, bound[t], _ = step32(mu, lv, prior, var_floor)
    _, bound[n_iters], _ = step32(mu, lv, prior, var_floor)
    return prior, bound


# ------------------------------------------------------------------------------------------------ error measures
def param_err(got, ref):
    """means and log-variances: |err| / (|ref| + 1)"""
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1.0)


def abs_err(got, ref):
    """weights and responsibilities: |err|"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))


def ll_err(got, ref, n_z):
    """ll and the bound: |err| / (|ref| + n_z)"""
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + n_z)


def prior_errs(got, ref, bound_got, bound_ref, n_z):
    """-> worst (weights, means, logvars, bound) errors of one result against another"""
    return (float(abs_err(got["weights"], ref["weights"]).max()), float(param_err(got["means"], ref["means"]).max()),
            float(param_err(got["logvars"], ref["logvars"]).max()), float(np.max(ll_err(bound_got, bound_ref, n_z))))
