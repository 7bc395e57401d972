"""The definition of ``latent_stats`` (avae_latent_stats in include/avae.h), for the tests.

With R_sd the rows that have both modality s and modality d (R_mm: that have m), population form (divide by the count):

    count[s, d]      |R_sd|
    mean[s, d, j]    mean of mu_s[:, j] over R_sd
    var[s, d, j]     variance of mu_s[:, j] over R_sd
    xcov[s, d, j]    covariance of mu_s[:, j] and mu_d[:, j] over R_sd
    assoc[s, d, j]   mean over R_sd of 0.5 * [(t * iv_s) * (t * iv_d) + d^2 * (iv_s + iv_d)],  v = exp(lv), iv = exp(-lv),
                     t = v_s - v_d, d = mu_s - mu_d;  the diagonal is exactly 0
    post_var[m, j]   mean of exp(lv_m[:, j]) over R_mm
    kl[m, j]         mean of 0.5 * (mu^2 + exp(lv) - lv - 1) over R_mm
    cov[m]           covariance matrix of mu_m over R_mm

An empty set has count 0 and NaN everywhere else.  ``stats64`` is that in float64, two-pass (the mean first, then the centred
sums).  ``stats32`` restates it in NumPy float32: two-pass, centred on the float32 mean, every sum a sequential float32 sum in row
order.  ``raw_var32`` is the variance a float32 raw-moment pass gives (E[x^2] - E[x]^2), the one the kernel must not be.
``families`` draws the tests' seeded inputs; ``errors`` is the normalised error of a result against ``stats64``'s."""
import numpy as np

TABLES = ("mean", "var", "xcov", "assoc")
PER_MOD = ("post_var", "kl")
NAMES = ("count",) + TABLES + PER_MOD + ("cov",)
FAMILIES = ("A", "B", "C")
ROWS = (1, 2, 65, 4099, 20000)
NZS = (7, 20, 64)


def family(rng, name, rows, nz, n_mod=2):
    """Posteriors of ``n_mod`` modalities: lv ~ U(-6, 1); mu = loc + scale * noise with (loc, scale) = A: (0, 1), B: (1000, 0.01),
    C: (3, 0.001).  The noise of modality m > 0 is 0.6 * (modality 0's) + 0.8 * (its own), so the encoders agree in part."""
    loc, scale = {"A": (0.0, 1.0), "B": (1000.0, 0.01), "C": (3.0, 0.001)}[name]
    base = rng.standard_normal((rows, nz))
    out = []
    for m in range(n_mod):
        noise = base if m == 0 else 0.6 * base + 0.8 * rng.standard_normal((rows, nz))
        out.append(((loc + scale * noise).astype(np.float32), rng.uniform(-6.0, 1.0, (rows, nz)).astype(np.float32)))
    return out


def seq_sum32(a, block=256):
    """Sequential float32 sum over axis 0, in row order (np.cumsum adds one element after the other, in the array's dtype)"""
    a = np.asarray(a)
    assert a.dtype == np.float32
    acc = np.zeros(a.shape[1:], np.float32)
    for lo in range(0, a.shape[0], block):
        acc = np.cumsum(np.concatenate([acc[None], a[lo:lo + block]]), axis=0, dtype=np.float32)[-1]
    return acc


def gram32(c, block=512):
    """sum over rows of the outer products c[n, :, None] * c[n, None, :], float32, sequential in row order"""
    acc = np.zeros((c.shape[1], c.shape[1]), np.float32)
    for lo in range(0, c.shape[0], block):
        b = np.ascontiguousarray(c[lo:lo + block].T)                # [nz, rows of the block]: the running sums go along memory
        prod = b[:, None, :] * b[None, :, :]
        prod[:, :, 0] += acc                                        # (acc + first product: the same sum, the operands swapped)
        acc = np.cumsum(prod, axis=2, dtype=np.float32, out=prod)[:, :, -1].copy()
    return acc


def _flags(posteriors, present, rows):
    M = len(posteriors)
    p = np.ones((rows, M), bool) if present is None else np.asarray(present) != 0
    for m, pair in enumerate(posteriors):
        if pair is None:
            p[:, m] = False
    return p


def _rows_of(posteriors, present):
    for pair in posteriors:
        if pair is not None:
            return pair[0].shape[0], pair[0].shape[1]
    raise ValueError("no modality given")


def _empty(M, nz, dt):
    out = {"count": np.zeros((M, M), np.int64)}
    for k in TABLES:
        out[k] = np.full((M, M, nz), np.nan, dt)
    for k in PER_MOD:
        out[k] = np.full((M, nz), np.nan, dt)
    out["cov"] = np.full((M, nz, nz), np.nan, dt)
    return out


def _stats(posteriors, present, dt, total, gram):
    """The definition in dtype ``dt`` with ``total`` as the sum over axis 0 and ``gram`` as the sum of the rows' outer products"""
    rows, nz = _rows_of(posteriors, present)
    M = len(posteriors)
    p = _flags(posteriors, present, rows)
    out = _empty(M, nz, dt)
    one, half = dt(1.0), dt(0.5)
    with np.errstate(all="ignore"):
        for s in range(M):
            for d in range(M):
                sel = p[:, s] & p[:, d]
                n = int(sel.sum())
                out["count"][s, d] = n
                if n == 0:
                    continue
                ms, ls = posteriors[s][0][sel].astype(dt), posteriors[s][1][sel].astype(dt)
                md, ld = posteriors[d][0][sel].astype(dt), posteriors[d][1][sel].astype(dt)
                cnt = dt(n)
                mean_s, mean_d = total(ms) / cnt, total(md) / cnt
                cs, cd = ms - mean_s, md - mean_d
                out["mean"][s, d] = mean_s
                out["var"][s, d] = total(cs * cs) / cnt
                out["xcov"][s, d] = total(cs * cd) / cnt
                vs, vd, is_, id_ = np.exp(ls), np.exp(ld), np.exp(-ls), np.exp(-ld)
                t, df = vs - vd, ms - md
                out["assoc"][s, d] = total(half * ((t * is_) * (t * id_) + (df * df) * (is_ + id_))) / cnt
                if s == d:
                    out["post_var"][s] = total(vs) / cnt
                    out["kl"][s] = total(half * (ms * ms + vs - ls - one)) / cnt
                    out["cov"][s] = gram(cs) / cnt
    for k in NAMES[1:]:
        assert out[k].dtype == dt
    return out


def stats64(posteriors, present=None):
    """``posteriors``: list over modalities of (mu, logvar) float32 [rows, nz] pairs or None; ``present`` [rows, M] or None"""
    return _stats(posteriors, present, np.float64, lambda a: a.sum(0), lambda c: c.T @ c)


def stats32(posteriors, present=None):
    return _stats(posteriors, present, np.float32, seq_sum32, gram32)


def brute64(posteriors, present=None):
    """``stats64`` written as loops over rows and columns: nothing shared with it but the formulas (small inputs only)"""
    from math import exp
    rows, nz = _rows_of(posteriors, present)
    M = len(posteriors)
    p = _flags(posteriors, present, rows)
    out = _empty(M, nz, np.float64)
    f = lambda m, n, j: (float(posteriors[m][0][n, j]), float(posteriors[m][1][n, j]))
    for s in range(M):
        for d in range(M):
            R = [n for n in range(rows) if p[n, s] and p[n, d]]
            out["count"][s, d] = len(R)
            if not R:
                continue
            for j in range(nz):
                ms = sum(f(s, n, j)[0] for n in R) / len(R)
                md = sum(f(d, n, j)[0] for n in R) / len(R)
                out["mean"][s, d, j] = ms
                out["var"][s, d, j] = sum((f(s, n, j)[0] - ms) ** 2 for n in R) / len(R)
                out["xcov"][s, d, j] = sum((f(s, n, j)[0] - ms) * (f(d, n, j)[0] - md) for n in R) / len(R)
                acc = 0.0
                for n in R:
                    (a, la), (b, lb) = f(s, n, j), f(d, n, j)
                    t = exp(la) - exp(lb)
                    acc += 0.5 * ((t * exp(-la)) * (t * exp(-lb)) + (a - b) ** 2 * (exp(-la) + exp(-lb)))
                out["assoc"][s, d, j] = acc / len(R)
                if s == d:
                    out["post_var"][s, j] = sum(exp(f(s, n, j)[1]) for n in R) / len(R)
                    out["kl"][s, j] = sum(0.5 * (f(s, n, j)[0] ** 2 + exp(f(s, n, j)[1]) - f(s, n, j)[1] - 1.0) for n in R) / len(R)
                    for i in range(nz):
                        mi = sum(f(s, n, i)[0] for n in R) / len(R)
                        out["cov"][s, i, j] = sum((f(s, n, i)[0] - mi) * (f(s, n, j)[0] - ms) for n in R) / len(R)
    return out


def raw_var32(mu):
    """E[x^2] - E[x]^2 with float32 sequential sums: [nz]"""
    x = np.asarray(mu, np.float32)
    n = np.float32(x.shape[0])
    m = seq_sum32(x) / n
    return seq_sum32(x * x) / n - m * m


def errors(got, ref):
    """Worst normalised error per statistic of ``got`` against ``ref`` (= stats64 of the same inputs) -> dict name -> float.
    Denominators: |mean| + std for mean; sqrt(var_i * var_j) for var, xcov and cov; the value for post_var; value + 1 for kl and
    assoc.  Where the denominator is 0 (a set of one row, a constant column) the entry must be equal, else the error is inf; an
    empty set's NaN must be NaN."""
    g = {k: np.asarray(got[k], np.float64) for k in NAMES[1:]}
    var = ref["var"]
    den = {"mean": np.abs(ref["mean"]) + np.sqrt(var), "var": var, "xcov": np.sqrt(var * np.swapaxes(var, 0, 1)),
           "assoc": ref["assoc"] + 1.0, "post_var": ref["post_var"], "kl": ref["kl"] + 1.0}
    dg = np.diagonal(ref["cov"], axis1=1, axis2=2)
    den["cov"] = np.sqrt(dg[:, :, None] * dg[:, None, :])
    out = {}
    with np.errstate(all="ignore"):
        for k in NAMES[1:]:
            r, x, dn = ref[k], g[k], den[k]
            nan = np.isnan(r)
            if not np.array_equal(np.isnan(x), nan):
                out[k] = np.inf
                continue
            diff = np.abs(x - r)
            e = np.where(nan | (diff == 0), 0.0, np.where(dn > 0, diff / dn, np.inf))
            out[k] = float(e.max()) if e.size else 0.0
    return out


def plan_slices(rows, row_tile, n_slices):
    """What avae_latent_stats_plan's numbers mean (include/avae.h): the slices' row ranges"""
    return [(i * row_tile, min(rows, (i + 1) * row_tile)) for i in range(n_slices)]


_CASES = {}


def case(name, rows, nz):
    """The arithmetic tests' inputs, seeded by (family, rows, n_z), with the float64 definition and the float32 restatement's
    errors against it; computed once per process."""
    key = (name, rows, nz)
    if key not in _CASES:
        rng = np.random.default_rng([FAMILIES.index(name), rows, nz])
        post = family(rng, name, rows, nz)
        ref = stats64(post)
        _CASES[key] = (post, ref, errors(stats32(post), ref))
    return _CASES[key]


def bound(nz):
    """Per statistic: 4 x the float32 restatement's worst error over the families x ROWS at this n_z"""
    worst = {k: 0.0 for k in NAMES[1:]}
    for name in FAMILIES:
        for rows in ROWS:
            for k, e in case(name, rows, nz)[2].items():
                worst[k] = max(worst[k], e)
    return {k: 4.0 * e for k, e in worst.items()}, worst
