"""NumPy definition of avae_impute / ``impute`` (include/avae.h), built on ``O.encode`` / ``O.decode``.

``ref`` is an ``OracleAssocVAE``; its ``quant`` is handed through, so the same code gives the bf16 reference.  Absent entries are
replaced by zeros before anything reads them and every gate is an ``np.where`` select, so NaN / Inf / None in an absent entry
cannot reach a result.  ``ref_impute(..., dtype=np.float64)`` is the definition: the fusion rule and a two-pass mean and population
variance over the K samples.  ``dtype=np.float32`` is the same definition in float32 arithmetic (float32 parameters, posteriors,
fusion, z and decoders; the sequential float32 Welford update of the kernels instead of the two passes; with ``quant='bf16'`` the
layers are ``encode32_bf16`` / ``decode32_bf16``: the oracle's roundings to bf16 with float32 products and sums between them,
because the oracle's own layers always compute in fp64).  Its distance from the fp64
result on a test's own inputs is the yardstick of the GPU tests: the kernels may differ from fp64 by rounding of that size.

``case`` builds the inputs the CPU and the GPU tests share."""
import numpy as np

from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O


def archs_for(nz, three):
    a = [make_arch("image", 784, 64, 48, nz), make_arch("joint", 147, 40, 32, nz)]
    if three:
        a.append(make_arch("aux", 50, 24, 16, nz))
    return a


def model_kw(three):
    return dict(binary=[True, False, False][:3 if three else 2], weights=[50.0, 1.0, 0.5][:3 if three else 2], assoc_lambda=8.0)


def init_flat(archs, seed):
    """Xavier weights from the oracle's initialiser and non-zero biases (the folded-bias column), as a flat float32 vector."""
    rng = np.random.default_rng(seed)
    flat = O.flatten_params(archs, O.init_params(archs, rng)).astype(np.float32)
    off = 0
    for na in archs:
        for _name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            if len(shp) == 1:
                flat[off:off + n] = 0.05 * rng.standard_normal(n)
            off += n
    return flat


def oracle_for(archs, three, act, B, flat, quant=None):
    kw = model_kw(three)
    return O.OracleAssocVAE(archs, kw["binary"], act, kw["weights"], kw["assoc_lambda"], 1e-3, B,
                            params_flat=np.asarray(flat, np.float64), quant=quant)


def pattern_rows(N, M, shift=0):
    """Presence [N, M]: row n has pattern (n + shift) mod 2^M, bit m = modality m -- every pattern, the empty one included, in any
    2^M consecutive rows."""
    code = (np.arange(N) + shift) % (1 << M)
    return ((code[:, None] >> np.arange(M)[None, :]) & 1).astype(bool)


def case(nz, three, N, K, seed):
    """-> (archs, X, present, eps or None): the inputs of one sampled-prediction case."""
    archs = archs_for(nz, three)
    rng = np.random.default_rng(seed)
    X = synth_batch(rng, N, [a["n_input"] for a in archs], model_kw(three)["binary"])
    eps = rng.standard_normal((N, K, nz)).astype(np.float32) if K else None
    return archs, X, pattern_rows(N, len(archs), shift=seed), eps


def fold(widths, X, present, N=None):
    """-> (presence [N, M] with None modalities folded in, X with absent entries selected to 0)"""
    M = len(widths)
    if present is None:
        N = next(np.asarray(x).shape[0] for x in X if x is not None) if N is None else N
        p = np.ones((N, M), bool)
    else:
        p = (np.asarray(present) != 0).copy()
    Xf = []
    for m in range(M):
        if X[m] is None:
            p[:, m] = False
            Xf.append(np.zeros((p.shape[0], widths[m])))
        else:
            Xf.append(np.where(p[:, m:m + 1], np.asarray(X[m], np.float64), 0.0))
    return p, Xf


def fuse(mu, lv, p):
    """The fusion rule.  mu, lv: [M, N, n_z] (their dtype is the arithmetic's), p: bool [N, M].  Max-shifted, modalities added in
    index order; one present modality is a select, none is the prior (zeros)."""
    mu, lv = np.asarray(mu), np.asarray(lv)
    dt = mu.dtype
    M, N, nz = mu.shape
    pm = [p[:, m][:, None] for m in range(M)]
    cnt = p.sum(1)[:, None]
    A = np.full((N, nz), -np.inf, dt)
    for m in range(M):
        A = np.where(pm[m], np.maximum(A, -lv[m]), A)
    A0 = np.where(cnt > 0, A, dt.type(0))
    sw, smu = np.zeros((N, nz), dt), np.zeros((N, nz), dt)
    one_mu, one_lv = np.zeros((N, nz), dt), np.zeros((N, nz), dt)
    with np.errstate(all="ignore"):
        for m in range(M):
            w = np.exp(np.where(pm[m], -lv[m] - A0, dt.type(0)))
            sw = np.where(pm[m], sw + w, sw)
            smu = np.where(pm[m], smu + w * np.where(pm[m], mu[m], dt.type(0)), smu)
            one_mu, one_lv = np.where(pm[m], mu[m], one_mu), np.where(pm[m], lv[m], one_lv)
        c = np.maximum(cnt, 1).astype(dt)
        mu_f = smu / np.where(cnt > 0, sw, dt.type(1))
        lv_f = -(A0 + np.log(np.where(cnt > 0, sw, dt.type(1)) / c))
    mu_f = np.where(cnt > 1, mu_f, np.where(cnt == 1, one_mu, dt.type(0)))
    lv_f = np.where(cnt > 1, lv_f, np.where(cnt == 1, one_lv, dt.type(0)))
    return mu_f.astype(dt), lv_f.astype(dt)


def fuse_naive(mu, lv, p):
    """The same Gaussian without the shift: precision = mean of exp(-lv), mean precision-weighted (rows with |S| >= 1)."""
    mu, lv = np.asarray(mu), np.asarray(lv)
    M = mu.shape[0]
    dt = mu.dtype
    with np.errstate(all="ignore"):
        sw = sum(np.where(p[:, m][:, None], np.exp(-lv[m]), dt.type(0)) for m in range(M))
        smu = sum(np.where(p[:, m][:, None], np.exp(-lv[m]) * mu[m], dt.type(0)) for m in range(M))
        return (smu / sw).astype(dt), (-np.log(sw / p.sum(1)[:, None].astype(dt))).astype(dt)


def kl_sum(mu, s, mus, lvs):
    """sum_m KL(N(mu, e^s) || N(mu_m, e^lv_m)) over one row: mu, s [n_z]; mus, lvs [|S|, n_z]."""
    return float(np.sum(0.5 * (lvs - s + (np.exp(s) + (mu - mus) ** 2) * np.exp(-lvs) - 1.0)))


def kl_sum_grad(mu, s, mus, lvs):
    """d kl_sum / d mu and d kl_sum / d s (s = log sigma^2)"""
    return np.sum((mu - mus) * np.exp(-lvs), 0), np.sum(0.5 * (np.exp(s) * np.exp(-lvs) - 1.0), 0)


def two_pass(x):
    """x [N, K, n] -> (mean, population variance) over the K axis in fp64, two passes"""
    x = np.asarray(x, np.float64)
    mean = x.sum(1) / x.shape[1]
    return mean, ((x - mean[:, None, :]) ** 2).sum(1) / x.shape[1]


def welford32(x):
    """x [N, K, n] -> (mean, population variance) by the kernels' sequential float32 update:
    delta = x_k - mean; mean += delta / (k + 1); M2 += delta * (x_k - mean); var = M2 / K"""
    x = np.asarray(x, np.float32)
    K = x.shape[1]
    mean = np.zeros((x.shape[0], x.shape[2]), np.float32)
    M2 = np.zeros_like(mean)
    for k in range(K):
        d = x[:, k] - mean
        mean = mean + d / np.float32(k + 1)
        M2 = M2 + d * (x[:, k] - mean)
    return mean, M2 / np.float32(K)


def _bf16_32(a):
    return O.bf16_round(a).astype(np.float32)


def encode32_bf16(na, p, x, act):
    """O.encode's MLP branch with quant='bf16' in float32 arithmetic: the same roundings to bf16, and float32 products and sums
    where the oracle has fp64 ones -- what the kernels' fp32 accumulators do between two roundings."""
    assert not na.get("hidden_conv")
    f, q = O.ACT[act][0], _bf16_32
    h = q(x)
    for i in range(len(O.hidden_sizes(na))):
        h = q(f(h @ q(p["enc_W%d" % (i + 1)]) + q(p["enc_b%d" % (i + 1)])))
    return h @ q(p["enc_Wmu"]) + q(p["enc_bmu"]), h @ q(p["enc_Wsig"]) + q(p["enc_bsig"])


def decode32_bf16(na, p, z, act, binary):
    """O.decode's MLP branch with quant='bf16' in float32 arithmetic (see encode32_bf16)"""
    assert not na.get("hidden_conv")
    f, q = O.ACT[act][0], _bf16_32
    g = q(z)
    for i in range(len(O.hidden_sizes(na))):
        g = q(f(g @ q(p["dec_W%d" % (i + 1)]) + q(p["dec_b%d" % (i + 1)])))
    logits = g @ q(p["dec_Wout"]) + q(p["dec_bout"])
    return (O._sigmoid(logits) if binary else logits).astype(np.float32)


def ref_impute(ref, X, present=None, n_samples=0, eps=None, dtype=np.float64, N=None):
    """-> {"mu", "logvar", "mean": [per modality], "var": [per modality] or None, "samples": [per modality [N, K, n_input]] or
    None} (the decoded samples are kept for the tests of the Welford update)."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    M = len(archs)
    dt = np.dtype(dtype)
    widths = [int(a["n_input"]) for a in archs]
    p, Xf = fold(widths, X, present, N)
    N, nz, K = p.shape[0], int(archs[0]["n_z"]), int(n_samples)
    params = ref.params if (q is not None or dt == np.float64) else \
        [{k: np.asarray(v, dt) for k, v in pm.items()} for pm in ref.params]
    enc = lambda m, x: O.encode(archs[m], params[m], x, act, q)[:2]                     # noqa: E731
    dec = lambda d, z: np.asarray(O.decode(archs[d], params[d], z, act, binary[d], q)[0])        # noqa: E731
    if q is not None and dt == np.float32:
        enc = lambda m, x: encode32_bf16(archs[m], params[m], x, act)                   # noqa: E731
        dec = lambda d, z: decode32_bf16(archs[d], params[d], z, act, binary[d])        # noqa: E731
    mu, lv = np.zeros((M, N, nz), dt), np.zeros((M, N, nz), dt)
    for m in range(M):
        if p[:, m].any():
            mu[m], lv[m] = enc(m, Xf[m].astype(dt))
    mu_f, lv_f = fuse(mu, lv, p)
    out = {"mu": mu_f, "logvar": lv_f, "var": None, "samples": None}
    if K == 0:
        out["mean"] = [dec(d, mu_f) for d in range(M)]
        return out
    e = np.asarray(eps, dt)
    assert e.shape == (N, K, nz), e.shape
    z = (mu_f[:, None, :] + np.exp(dt.type(0.5) * lv_f)[:, None, :] * e).astype(dt)
    out["samples"] = [dec(d, z.reshape(N * K, nz)).reshape(N, K, widths[d]) for d in range(M)]
    mv = [two_pass(x) if dt == np.float64 else welford32(x) for x in out["samples"]]
    out["mean"], out["var"] = [a for a, _ in mv], [b for _, b in mv]
    return out


def rounding_spread(ref, X, present, n_samples, eps):
    """The definition in float32 arithmetic against itself in fp64 on these inputs -> (fp64 result, per modality
    (max |mean32 - mean64| / max |mean64|, max |var32 - var64| / max var64), max |mu| and |logvar| deviations)."""
    r64 = ref_impute(ref, X, present, n_samples, eps, np.float64)
    r32 = ref_impute(ref, X, present, n_samples, eps, np.float32)
    dev = []
    for d in range(len(r64["mean"])):
        dm = np.abs(r32["mean"][d] - r64["mean"][d]).max() / max(np.abs(r64["mean"][d]).max(), 1e-30)
        dv = 0.0 if r64["var"] is None else np.abs(r32["var"][d] - r64["var"][d]).max() / max(r64["var"][d].max(), 1e-30)
        dev.append((float(dm), float(dv)))
    lat = (float(np.abs(r32["mu"] - r64["mu"]).max()), float(np.abs(r32["logvar"] - r64["logvar"]).max()))
    return r64, dev, lat
