"""score_samples / log_likelihood on a real MI355X at the shapes and values where a wave64 row kernel or a multi-pass reduction
goes wrong: the benchmark's nets at serving batch sizes (every pass layout of avae_loglik's host loop, both serve buckets, several
samples per lane in k_iw_reduce), batch-size and route invariance, a seeded sweep of odd models (1 and 4 modalities, n_z 1-64,
every transfer function), posteriors far from the prior (both two_sinh branches, saturated sigmoids), log-weights that spread
over more than 100 nats, NaN propagation, and the statistics of the internal eps.

Tolerances: fp32 compute against the fp64 oracle at 1e-5 of each column's max, bf16 compute (softplus on the fixed
architectures) against quant='bf16' at 3e-3, as tests/test_gpu_score.py and tests/test_gpu_loglik.py."""
import numpy as np
import pytest
import torch

from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O
from scoring_reference import logsumexp, recon_rows, ref_loglik, ref_scores
from test_gpu_loglik import assert_columns
from test_gpu_parity import check_step_parity

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 3e-3}
ACT = {"fp32": "relu", "bf16": "softplus"}


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def host_params(archs, seed, bias=0.05):
    """Per-modality parameter dicts: xavier weights, non-zero biases (the folded-bias column), rounded to fp32 so the handle and
    the oracle start from the same numbers.  Independent of batch_size, so several handles can share them."""
    rng = np.random.default_rng(seed)
    ps = O.init_params(archs, rng)
    for p in ps:
        for name in p:
            if p[name].ndim == 1:
                p[name] = bias * rng.standard_normal(p[name].shape)
    return [{k: v.astype(np.float32).astype(np.float64) for k, v in p.items()} for p in ps]


def make_pair(V, archs, binary, weights, lam, act, B, dtype, params, use_graph=True):
    """HIP handle + oracle (fp64 for fp32 compute, quant='bf16' for bf16 compute) on the same parameters."""
    flat = O.flatten_params(archs, params)
    model = V.AssocVariationalAutoEncoder(archs, binary=binary, transfer_fct=act, weights=weights, assoc_lambda=lam,
                                          learning_rate=1e-3, batch_size=B, compute_dtype=dtype, seed=5, use_graph=use_graph)
    model.set_params(flat.astype(np.float32))
    ref = O.OracleAssocVAE(archs, binary, act, weights, lam, 1e-3, B, params_flat=flat,
                           quant=None if dtype == "fp32" else "bf16")
    return model, ref


def c2(nz=20):
    """BASELINE C2's nets: 784-500-500 (Bernoulli) / 147-200-200 (Gaussian)."""
    return ([make_arch("image", 784, 500, 500, nz), make_arch("joint", 147, 200, 200, nz)], [True, False], [50.0, 1.0], 8.0)


def small_pair(nz=20):
    return ([make_arch("image", 784, 64, 48, nz), make_arch("joint", 147, 48, 32, nz)], [True, False], [50.0, 1.0], 8.0)


def inputs(archs, binary, N, K, seed):
    rng = np.random.default_rng(seed)
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    nz = archs[0]["n_z"]
    return X, rng.standard_normal((N, nz)).astype(np.float32), rng.standard_normal((N, K, nz)).astype(np.float32)


# ----------------------------------------------------------------------------- 1. serving shapes
# (N, K) per batch_size, with the pass layout of avae_loglik each one takes.  n = rows per pass, kb = samples per pass, nd = n * kc
# decoded rows; a pass with nd <= 64 in a handle with B > 64 decodes through the 64-row serve bucket, any other through the B bucket.
# K = None: the default n_samples (64).
SERVING = {
    256: [(9, 64),     # n = 4, kb = 64: two passes with nd = B = 256, then one row (nd = 64, the 64-row bucket)
          (8, 33),     # n = 7: nd = 231 < B, then one row (nd = 33, the 64-row bucket)
          (4, 65),     # n = 3: nd = 195 < B, then one row (nd = 65, just above the bucket)
          (2, 300),    # K >= B: one row spans a block of kc = 256 (4 samples per lane) and a 44-sample tail (64-row bucket)
          (5, None)],  # default K = 64: nd = 256, then nd = 64
    100: [(3, 64),     # one row per pass: nd = 64 through the 64-row bucket of a B > 64 handle
          (3, 65),     # one row per pass: nd = 65, the 100-row bucket
          (13, 9),     # n = 11: nd = 99, then two rows (nd = 18, the 64-row bucket)
          (2, 300),    # K >= B: three blocks of kc = 100 (lanes 0-35 fold two samples)
          (3, None)],  # default K = 64: nd = 64, the 64-row bucket
}


@pytest.mark.parametrize("B", [256, 100])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_c2_serving_shapes(V, B, dtype):
    archs, binary, weights, lam = c2()
    model, ref = make_pair(V, archs, binary, weights, lam, ACT[dtype], B, dtype, host_params(archs, 31))
    for N, K in SERVING[B]:
        X, _, eps = inputs(archs, binary, N, K or 64, 100 * N + (K or 0))
        got = model.log_likelihood(X, eps=eps) if K is None else model.log_likelihood(X, n_samples=K, eps=eps)
        assert_columns(got, ref_loglik(ref, X, eps), TOL[dtype], "B=%d %s N=%d K=%s " % (B, dtype, N, K))
    Nmax = 2 * B + 1
    X, eps, _ = inputs(archs, binary, Nmax, 1, 7)
    for N in (1, B - 1, B, Nmax):
        Xn = [x[:N] for x in X]
        got = model.score_samples(Xn, eps=eps[:N], cross_modal=True)
        assert_columns(got, ref_scores(ref, Xn, eps[:N], cross=True), TOL[dtype], "B=%d %s score N=%d " % (B, dtype, N))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_c2_nz64_serving(V, dtype):
    """n_z = 64 at B = 256: the serve route has no fused first layer and replays its graph."""
    archs, binary, weights, lam = c2(64)
    B = 256
    model, ref = make_pair(V, archs, binary, weights, lam, ACT[dtype], B, dtype, host_params(archs, 32))
    for N, K in ((9, 64), (2, 300)):
        X, _, eps = inputs(archs, binary, N, K, N + K)
        assert_columns(model.log_likelihood(X, n_samples=K, eps=eps), ref_loglik(ref, X, eps), TOL[dtype],
                       "nz=64 %s N=%d K=%d " % (dtype, N, K))
    X, eps, _ = inputs(archs, binary, B + 3, 1, 8)
    assert_columns(model.score_samples(X, eps=eps, cross_modal=True), ref_scores(ref, X, eps, cross=True), TOL[dtype],
                   "nz=64 %s score " % dtype)


# ----------------------------------------------------------------------------- 2. batch-size and route invariance
def _assert_close(a, b, tol, what):
    """|a - b| <= tol * max |b| per column."""
    for key in b:
        x = np.asarray(a[key], np.float64).reshape(len(a[key]), -1)
        y = np.asarray(b[key], np.float64).reshape(len(b[key]), -1)
        assert x.shape == y.shape, (what, key)
        for c in range(y.shape[1]):
            scale = max(np.abs(y[:, c]).max(), 1e-30)
            err = np.abs(x[:, c] - y[:, c]).max()
            assert err <= tol * scale, "%s%s column %d: max diff %.3e vs max %.3e" % (what, key, c, err, scale)


def test_batch_size_and_route_invariance(V):
    """One set of parameters on handles with B in {16, 64, 100, 256} (serve route) and B = 100 with use_graph = False (modality by
    modality): every handle matches the oracle, and they agree with each other within 2e-6 of each column's max (include/avae.h:
    the result depends on batch_size only through the order of fp32 sums).  generate shares the route choice."""
    archs, binary, weights, lam = small_pair()
    params = host_params(archs, 33)
    N = 203
    X, eps1, _ = inputs(archs, binary, N, 1, 34)
    epsk = {K: np.random.default_rng(K).standard_normal((N, K, 20)).astype(np.float32) for K in (5, 70)}
    z = np.random.default_rng(35).standard_normal((150, 20)).astype(np.float32)
    base = None
    for B, use_graph in ((100, True), (16, True), (64, True), (256, True), (100, False)):
        model, ref = make_pair(V, archs, binary, weights, lam, "relu", B, "fp32", params, use_graph=use_graph)
        what = "B=%d use_graph=%s " % (B, use_graph)
        got = {"score": model.score_samples(X, eps=eps1, cross_modal=True)}
        for K, e in epsk.items():
            got[K] = model.log_likelihood(X, n_samples=K, eps=e)
        if base is None:
            base = got
            want = {"score": ref_scores(ref, X, eps1, cross=True)}
            want.update({K: ref_loglik(ref, X, e) for K, e in epsk.items()})
        for key in got:
            assert_columns(got[key], want[key], 1e-5, what + "%s vs oracle: " % key)
            _assert_close(got[key], base[key], 2e-6, what + "%s vs B=100: " % key)
        if B == 100:
            gen, rgen = model.generate(z), ref.generate(z)
            for m in range(2):
                assert np.abs(gen[m] - rgen[m]).max() <= 1e-5 * max(1, np.abs(rgen[m]).max()), (what, m)
            if use_graph:
                gen_graph = gen
            else:
                for m in range(2):
                    assert np.abs(gen[m] - gen_graph[m]).max() <= 2e-6 * max(1, np.abs(gen_graph[m]).max()), m


# ----------------------------------------------------------------------------- 3. random shapes
def test_random_models_score_and_loglik(V):
    """20 seeded models: 1-4 modalities (M = 1 and M = 4 included), 1-8 hidden layers of widths 1-300, n_input 1 / 63 / 65 among
    them, n_z from {1, 2, 3, 5, 31, 33, 63, 64}, every transfer function, Bernoulli and Gaussian modalities mixed, B from
    {1, 7, 33, 64, 65, 100}, K from {1, 2, 63, 64, 65, 2B+3}.  Both APIs against the fp64 oracle; every third model also in bf16
    against quant='bf16'.  M = 1: no pairs, so assoc is [N, 0], joint is marginal bitwise and cost = w (recon + latent)."""
    rng = np.random.default_rng(4242)
    acts = ["relu", "softplus", "tanh", "sigmoid", "identity"]
    nzs = [1, 2, 3, 5, 31, 33, 63, 64]
    forced_n_in = {0: 1, 1: 63, 2: 65, 7: 65, 9: 63}
    for case in range(20):
        M = (1, 4, 2, 3)[case % 4]
        act, nz = acts[case % 5], nzs[case % 8]
        B = int(rng.choice([1, 7, 33, 64, 65, 100]))
        K = int(rng.choice([1, 2, 63, 64, 65, 2 * B + 3]))
        N = int(rng.choice([1, B + 1, 2 * B + 3]))
        N = max(1, min(N, 2048 // K))                          # bounds the oracle's N * K decoded rows
        archs, binary = [], []
        for m in range(M):
            hs = [int(rng.integers(1, 301)) for _ in range(int(rng.integers(1, 9)))]
            n_in = forced_n_in[case] if m == 0 and case in forced_n_in else int(rng.integers(1, 301))
            archs.append(make_arch("m%d" % m, n_in, 0, 0, nz, n_hidden=hs))
            binary.append((m + case) % 2 == 0)
        weights = [float(rng.choice([0.5, 1.0, 3.0, 50.0])) for _ in range(M)]
        lam = float(rng.choice([0.0, 1e-5, 0.3, 8.0]))
        params = host_params(archs, 500 + case)
        X, eps1, epsk = inputs(archs, binary, N, K, 600 + case)
        for dtype in ("fp32", "bf16") if case % 3 == 0 else ("fp32",):
            what = "case %d %s: M=%d nz=%d B=%d N=%d K=%d act=%s archs=%s: " % (
                case, dtype, M, nz, B, N, K, act, [(a["n_input"], a["n_hidden"]) for a in archs])
            try:
                model, ref = make_pair(V, archs, binary, weights, lam, act, B, dtype, params)
                sc = model.score_samples(X, eps=eps1, cross_modal=True)
                assert_columns(sc, ref_scores(ref, X, eps1, cross=True), TOL[dtype], "score ")
                ll = model.log_likelihood(X, n_samples=K, eps=epsk)
                assert_columns(ll, ref_loglik(ref, X, epsk), TOL[dtype], "loglik ")
                if M == 1:
                    assert sc["assoc"].shape == (N, 0)
                    assert np.array_equal(ll["joint"], ll["marginal"]), "joint != marginal"
                    want = np.float32(weights[0]) * (sc["recon"][:, 0] + sc["latent"][:, 0])
                    assert np.array_equal(sc["cost"], want), "cost != w (recon + latent)"
            except AssertionError as e:
                raise AssertionError(what + str(e))


# ----------------------------------------------------------------------------- 4. posteriors far from the prior
# log sigma^2 heads per latent dimension (n_z = 20) of three modalities, bf16-exact.  Pair (0, 1) spans 0-16 with differences of
# about 0.99 / 1.0 / 1.01 around two_sinh's switch (|lv_i - lv_j| = 1 in the score kernel, whose argument is half the difference);
# pair (0, 2) stays within 0-7.75, where the exponential branch is needed for accuracy and the column is not dominated by the
# e^8-sized terms of pair (0, 1).
_LV = np.array([
    # lv0    lv1         lv2
    [-12.0, 4.0, -12.0],
    [-12.0, 2.0, -12.0],
    [-10.0, 2.0, -10.0],
    [-8.0, 2.0, -8.0],
    [-4.0, 4.0, -4.0],
    [0.0, 0.9921875, -7.75],
    [0.0, 1.0, -7.0],
    [0.0, 1.0078125, -6.0],
    [-1.0, -0.0078125, -6.0],
    [2.0, 3.0, -2.5],
    [1.0, 1.5, -3.0],
    [3.0, 3.0, 0.0],
    [-2.0, 0.0, -4.5],
    [-3.0, 0.0, -5.0],
    [0.0, 0.9921875, -1.5],
    [-2.0, -1.0, -3.0],
    [0.0, 1.0078125, -0.5],
    [-6.0, -5.75, -6.0],
    [2.0, 4.0, -5.5],
    [-1.0, 3.0, -6.5]])


def far_models():
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 48, 32, 20), make_arch("aux", 96, 40, 32, 20)]
    return archs, [True, False, True], [50.0, 1.0, 2.0], 0.5


def far_params(archs, seed):
    """enc_bsig from _LV, enc_bmu at +-3 (modalities 0 and 2 share signs, 1 flips half of them), the heads' weights scaled by
    0.02 so mu / lv stay within a few hundredths of the biases, dec_bout at +-8 (saturated sigmoids)."""
    ps = host_params(archs, seed)
    rng = np.random.default_rng(seed + 1)
    sign = np.where(rng.random(20) < 0.5, -3.0, 3.0)
    flip = np.where(np.arange(20) % 2 == 0, 1.0, -1.0)
    for m, p in enumerate(ps):
        p["enc_bsig"] = _LV[:, m].copy()
        p["enc_bmu"] = sign * (flip if m == 1 else 1.0)
        p["enc_Wsig"] = (0.02 * p["enc_Wsig"]).astype(np.float32).astype(np.float64)
        p["enc_Wmu"] = (0.02 * p["enc_Wmu"]).astype(np.float32).astype(np.float64)
        p["dec_bout"] = np.where(rng.random(p["dec_bout"].shape) < 0.5, -8.0, 8.0)
    return ps


def _assert_far_from_prior(ref, X):
    lv = [O.encode(na, p, np.asarray(x, np.float64), ref.act, ref.quant)[1] for na, p, x in zip(ref.network_architectures, ref.params, X)]
    d = np.concatenate([np.abs(lv[i] - lv[j]).ravel() for i in range(3) for j in range(i + 1, 3)])
    # the score kernel's two_sinh(dlv / 2) and the training loss's two_sinh(dlv / 2), two_sinh(dlv) switch at |dlv| = 1 and 0.5
    assert np.any(d < 0.5) and np.any((d >= 0.5) & (d < 1.0)), "series branch not reached"
    assert np.any((d > 0.97) & (d < 1.0)) and np.any((d >= 1.0) & (d < 1.03)), "|dlv| does not straddle 1"
    assert np.any((d > 5.0) & (d < 8.0)) and d.max() >= 15.0, "exponential branch not reached"
    assert min(v.min() for v in lv) <= -11.5 and max(v.max() for v in lv) >= 3.5
    xh = O.decode(ref.network_architectures[0], ref.params[0], np.zeros((1, 20)), ref.act, True, ref.quant)[0]
    assert np.mean(np.minimum(xh, 1 - xh) < 1e-3) > 0.9, "decoder outputs not saturated"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_posteriors_far_from_prior(V, dtype):
    """score_samples(cross_modal=True), log_likelihood and one training step (latent_item shares two_sinh) against the oracle,
    after asserting from the oracle's lv that both two_sinh branches are reached.  The Adam check is scaled to |theta|: fp32 holds
    a head bias of -12 only to ~5e-7."""
    archs, binary, weights, lam = far_models()
    B = 64
    params = far_params(archs, 41)
    model, ref = make_pair(V, archs, binary, weights, lam, ACT[dtype], B, dtype, params)
    N, K = B + 5, 7
    X, eps1, epsk = inputs(archs, binary, N, K, 42)
    _assert_far_from_prior(ref, X)
    assert_columns(model.score_samples(X, eps=eps1, cross_modal=True), ref_scores(ref, X, eps1, cross=True), TOL[dtype],
                   "far %s score " % dtype)
    assert_columns(model.log_likelihood(X, n_samples=K, eps=epsk), ref_loglik(ref, X, epsk), TOL[dtype], "far %s loglik " % dtype)
    check_step_parity(V, archs, binary, weights, lam, ACT[dtype], B, dtype, steps=1, p0=O.flatten_params(archs, params),
                      adam_rel=True)


# ----------------------------------------------------------------------------- 5. log-weight spread and merge order
def ref_logweights(ref, X, eps):
    """Per-sample log-weights [N, K, M, 2 + M] of every output (marginal, joint, conditional[s][d]) under proposal s."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    X = [np.asarray(x, np.float64) for x in X]
    eps = np.asarray(eps, np.float64)
    N, K, nz = eps.shape
    M = len(archs)
    out = np.zeros((N, K, M, 2 + M))
    for s in range(M):
        mu, lv = O.encode(archs[s], ref.params[s], X[s], act, q)[:2]
        z = mu[:, None, :] + np.exp(0.5 * lv)[:, None, :] * eps
        r = np.sum(-0.5 * z ** 2 + 0.5 * eps ** 2 + 0.5 * lv[:, None, :], axis=2)
        ell = np.stack([-recon_rows(np.repeat(X[d], K, axis=0),
                                    O.decode(archs[d], ref.params[d], z.reshape(N * K, nz), act, binary[d], q)[0],
                                    binary[d]).reshape(N, K) for d in range(M)], axis=2)
        out[:, :, s, 0] = ell[:, :, s] + r
        out[:, :, s, 1] = ell.sum(2) + r
        out[:, :, s, 2:] = ell
    return out


def spread_eps(N, K, nz, dominant, seed):
    """Every sample at scale 6 except sample dominant[n] of row n at scale 0.05: z far from / at the posterior mean."""
    rng = np.random.default_rng(seed)
    eps = 6.0 * rng.standard_normal((N, K, nz))
    for n, k in enumerate(dominant):
        eps[n, k] = 0.05 * rng.standard_normal(nz)
    return eps.astype(np.float32)


@pytest.mark.parametrize("B,K,dominant", [
    (24, 77, [3, 30, 75]),           # blocks of 24: dominant sample in the first, a middle and the last (5-sample) block
    (256, 600, [70, 300, 590]),      # blocks 256, 256, 88: lane 6's second sample of the first block, a middle, the last block
])
def test_logweight_spread_and_merge_order(V, B, K, dominant):
    archs, binary, weights, lam = small_pair()
    params = host_params(archs, 51)
    for p in params:                  # posteriors mostly wider than the prior: a far sample also loses on r = log N(z) - log q(z)
        p["enc_bsig"] = p["enc_bsig"] + 1.0
    model, ref = make_pair(V, archs, binary, weights, lam, "relu", B, "fp32", params)
    N = len(dominant)
    X = synth_batch(np.random.default_rng(52), N, [784, 147], binary)
    eps = spread_eps(N, K, 20, dominant, 53)
    lw = ref_logweights(ref, X, eps)
    spread = lw.max(1) - lw.min(1)                                           # [N, M, 2 + M]
    assert spread.min() > 100.0, "log-weight spread only %.1f nats" % spread.min()
    for n, k in enumerate(dominant):
        assert np.all(lw[n].argmax(0) == k), "row %d: the dominant sample of some output is not %d" % (n, k)
    got = model.log_likelihood(X, n_samples=K, eps=eps)
    want = ref_loglik(ref, X, eps)
    assert_columns(got, want, 1e-5, "B=%d K=%d " % (B, K))
    # ref_loglik is the log-mean-exp of these log-weights
    lme = logsumexp(lw, 1) - np.log(K)
    assert np.allclose(lme[:, :, 0], want["marginal"]) and np.allclose(lme[:, :, 2:], want["conditional"])


# ----------------------------------------------------------------------------- 6. NaN propagation
def _same_rows(a, b, n):
    for key in b:
        x, y = np.delete(np.asarray(a[key]), n, axis=0), np.delete(np.asarray(b[key]), n, axis=0)
        assert np.array_equal(x, y), "%s: a row other than %d changed" % (key, n)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_nan_propagation(V, act):
    """NaN propagates through every log-sum-exp merge.  A NaN eps entry of row n at sample k* reaches every proposal's
    r, so marginal[n, :] and joint[n, :] are NaN wherever k* sits (lane 0 of the first block, a lane above 0, the last block, or
    a pass of several rows); a NaN in x_d of row n makes marginal[n, d], joint[n, :], conditional[n, :, d], recon[n, d],
    cost[n] and cross[n, :, d] NaN.  Every other row is bitwise the clean call.  The encoder-side outputs of a NaN input are
    not asserted (the kernels' relu maps NaN to 0)."""
    archs, binary, weights, lam = small_pair()
    B, N, n = 24, 5, 2
    model, _ = make_pair(V, archs, binary, weights, lam, act, B, "fp32", host_params(archs, 61))
    X, eps1, _ = inputs(archs, binary, N, 1, 62)
    for K, kstar in ((77, 0), (77, 5), (77, 75), (5, 3)):
        eps = np.random.default_rng(63).standard_normal((N, K, 20)).astype(np.float32)
        clean = model.log_likelihood(X, n_samples=K, eps=eps)
        bad = eps.copy()
        bad[n, kstar, 7] = np.nan
        got = model.log_likelihood(X, n_samples=K, eps=bad)
        assert np.all(np.isnan(got["marginal"][n])) and np.all(np.isnan(got["joint"][n])), (K, kstar)
        _same_rows(got, clean, n)
        for key in clean:
            assert np.all(np.isfinite(clean[key])), key
    K = 77
    eps = np.random.default_rng(64).standard_normal((N, K, 20)).astype(np.float32)
    clean = model.log_likelihood(X, n_samples=K, eps=eps)
    clean_sc = model.score_samples(X, eps=eps1, cross_modal=True)
    for d in range(2):
        Xb = [x.copy() for x in X]
        Xb[d][n, 11] = np.nan
        got = model.log_likelihood(Xb, n_samples=K, eps=eps)
        assert np.isnan(got["marginal"][n, d]) and np.all(np.isnan(got["joint"][n])), d
        assert np.all(np.isnan(got["conditional"][n, :, d])), d
        _same_rows(got, clean, n)
        sc = model.score_samples(Xb, eps=eps1, cross_modal=True)
        assert np.isnan(sc["recon"][n, d]) and np.isnan(sc["cost"][n]) and np.all(np.isnan(sc["cross"][n, :, d])), d
        _same_rows(sc, clean_sc, n)


# ----------------------------------------------------------------------------- 7. internal eps, from the outside
def constant_params(archs, seed, mu=None):
    """Every decoder weight 0 (the output is a function of the biases only); with mu given, every encoder weight 0 as well, with
    enc_bmu = mu and enc_bsig = 0."""
    ps = host_params(archs, seed, bias=0.5)
    for p in ps:
        for name in p:
            if p[name].ndim == 2 and (name.startswith("dec_") or mu is not None):
                p[name] = np.zeros_like(p[name])
        if mu is not None:
            p["enc_bmu"] = np.asarray(mu, np.float64).copy()
            p["enc_bsig"] = np.zeros_like(p["enc_bsig"])
    return ps


def test_constant_decoders_conditional_is_exact(V):
    """z does not matter: conditional[n, s, d] is an LSE of K equal values l_d = -recon_d(x_d, dec_d(.)) minus log K, across any
    number of sample blocks."""
    archs, binary, weights, lam = small_pair()
    B, N = 100, 7
    model, ref = make_pair(V, archs, binary, weights, lam, "relu", B, "fp32", constant_params(archs, 71))
    X = synth_batch(np.random.default_rng(72), N, [784, 147], binary)
    ell = np.stack([-recon_rows(np.asarray(X[d], np.float64),
                                O.decode(archs[d], ref.params[d], np.zeros((N, 20)), "relu", binary[d])[0], binary[d])
                    for d in range(2)], 1)                                                 # [N, M]
    for K in (1, 64, 65, 300):
        got = model.log_likelihood(X, n_samples=K)["conditional"].astype(np.float64)
        for s in range(2):
            err = np.abs(got[:, s, :] - ell) / np.maximum(1.0, np.abs(ell))
            assert err.max() <= 1e-6, "K=%d s=%d: rel err %.3e" % (K, s, err.max())


def test_internal_eps_importance_weight_statistics(V):
    """Constant encoders (mu fixed with sum mu^2 = 0.5, lv = 0) and decoders: w = exp(marginal[:, s] - conditional[:, s, s]) is
    the mean of K importance weights exp(r_k) with E = 1 and Var = (e^{sum mu^2} - 1) / K.  Eps reused across samples gives K
    times the variance, eps reused across rows none, eps that is not N(0, 1) moves the mean.  Deterministic: the Philox stream is
    fixed by the seed."""
    archs, binary, weights, lam = small_pair()
    mu = np.random.default_rng(81).standard_normal(20)
    mu *= np.sqrt(0.5 / np.sum(mu ** 2))
    mu = mu.astype(np.float32).astype(np.float64)
    model, _ = make_pair(V, archs, binary, weights, lam, "relu", 100, "fp32", constant_params(archs, 82, mu=mu))
    N, K = 4096, 16
    X = synth_batch(np.random.default_rng(83), N, [784, 147], binary)
    ll = model.log_likelihood(X, n_samples=K)
    var1 = np.expm1(np.sum(mu ** 2))
    for s in range(2):
        w = np.exp(ll["marginal"][:, s].astype(np.float64) - ll["conditional"][:, s, s].astype(np.float64))
        sigma = np.sqrt(var1 / K / N)
        assert abs(w.mean() - 1.0) <= 5 * sigma, "s=%d: mean %.5f, 5 sigma = %.5f" % (s, w.mean(), 5 * sigma)
        v = w.var()
        assert abs(v / (var1 / K) - 1.0) <= 0.25, "s=%d: variance %.5f vs %.5f" % (s, v, var1 / K)


def test_internal_eps_shared_by_every_proposal(V):
    """Two identical modalities (architecture, parameters, inputs): with the internal eps every output of proposal 0 equals
    proposal 1's (bitwise expected), across sample blocks and with several rows per pass."""
    archs = [make_arch("a", 96, 40, 32, 12), make_arch("b", 96, 40, 32, 12)]
    binary = [True, True]
    p = host_params(archs[:1], 91)[0]
    model, _ = make_pair(V, archs, binary, [1.0, 1.0], 0.5, "tanh", 32, "fp32", [p, dict(p)])
    x = synth_batch(np.random.default_rng(92), 45, [96], [True])[0]
    for K in (5, 70):
        ll = model.log_likelihood([x, x], n_samples=K)
        pairs = [(ll["marginal"][:, 0], ll["marginal"][:, 1]), (ll["joint"][:, 0], ll["joint"][:, 1]),
                 (ll["conditional"][:, 0, :], ll["conditional"][:, 1, :])]
        for a, b in pairs:
            a, b = a.astype(np.float64), b.astype(np.float64)
            assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(b))), K
