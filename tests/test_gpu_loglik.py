"""log_likelihood / avae_loglik on a real MI355X: importance-weighted marginal, joint and conditional log-likelihoods against the
CPU oracle (fp64, and quant='bf16' for the bf16 path), every pass boundary, the K = 1 identity with score_samples, Jensen's
inequality, determinism and no side effects on training."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import shadow_err, synth_batch
from scoring_reference import logsumexp, ref_loglik
from test_gpu_score import MODELS, build_pair, c1_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def assert_columns(got, want, tol, what=""):
    for key, r in want.items():
        g = np.asarray(got[key], np.float64)
        assert g.shape == r.shape, "%s%s shape %s vs %s" % (what, key, g.shape, r.shape)
        g2, r2 = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
        assert np.all(np.isfinite(g2)), "%s%s not finite" % (what, key)
        for c in range(r2.shape[1]):
            scale = max(np.abs(r2[:, c]).max(), 1e-30)
            err = np.abs(g2[:, c] - r2[:, c]).max()
            assert err <= tol * scale, "%s%s column %d: max err %.3e vs max |ref| %.3e" % (what, key, c, err, scale)


@pytest.mark.parametrize("name", ["c1", "three", "conv"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loglik_parity(V, name, dtype):
    """Every output against the fp64 oracle (fp32 compute, relu, 1e-5 of the column's max) or the quant='bf16' oracle (bf16
    compute, softplus, 3e-3); 2B+3 rows and K = 5, so several rows share a pass and a chunk is partial."""
    archs, binary, weights, lam = MODELS[name]()
    B = 24
    fp32 = dtype == "fp32"
    model, ref = build_pair(V, archs, binary, weights, lam, "relu" if fp32 else "softplus", B, dtype,
                            quant=None if fp32 else "bf16")
    rng = np.random.default_rng(17)
    N, K, M = 2 * B + 3, 5, len(archs)
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, K, archs[0]["n_z"])).astype(np.float32)
    got = model.log_likelihood(X, n_samples=K, eps=eps)
    assert isinstance(got["marginal"], np.ndarray)
    assert got["marginal"].shape == (N, M) and got["joint"].shape == (N, M) and got["conditional"].shape == (N, M, M)
    assert_columns(got, ref_loglik(ref, X, eps), 1e-5 if fp32 else 3e-3, "%s/%s " % (name, dtype))


@pytest.mark.parametrize("nz", [48, 64])
def test_loglik_wide_latents(V, nz):
    archs, binary, weights, lam = c1_like(nz)
    B = 16
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(nz)
    N, K = B + 5, 3
    X = synth_batch(rng, N, [784, 147], binary)
    eps = rng.standard_normal((N, K, nz)).astype(np.float32)
    assert_columns(model.log_likelihood(X, n_samples=K, eps=eps), ref_loglik(ref, X, eps), 1e-5, "nz=%d " % nz)


def test_loglik_pass_boundaries(V):
    """B = 24: K in {1, 7, B-1, B, B+3, 3B+5} crosses every pass layout (several rows per pass, one row per pass, one row over
    several passes with a partial last block), rows in {0, 1, 2B+3}; device tensors as strided views of one matrix."""
    archs, binary, weights, lam = c1_like()
    B = 24
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(4)
    Nmax, Kmax = 2 * B + 3, 3 * B + 5
    data = np.concatenate(synth_batch(rng, Nmax, [784, 147], binary), axis=1)
    eps_all = rng.standard_normal((Nmax, Kmax, 20)).astype(np.float32)
    dev = torch.from_numpy(data).to(model.device)
    for K in (1, 7, B - 1, B, B + 3, Kmax):
        for N in (0, 1, Nmax):
            eps = np.ascontiguousarray(eps_all[:N, :K])
            got = model.log_likelihood([dev[:N, :784], dev[:N, 784:]], n_samples=K, eps=torch.from_numpy(eps).to(model.device))
            assert torch.is_tensor(got["marginal"]) and got["marginal"].device == model.device
            assert got["conditional"].shape == (N, 2, 2)
            if N:
                got = {k: v.cpu().numpy() for k, v in got.items()}
                assert_columns(got, ref_loglik(ref, [data[:N, :784], data[:N, 784:]], eps), 1e-5, "N=%d K=%d " % (N, K))


def _r_from_transform(model, X, eps):
    """r = log N(z;0,I) - log q_m(z|x_m) of every modality at one eps row per sample, from the HIP encoders' own mu / log sigma^2."""
    out = []
    e = np.asarray(eps, np.float64)
    for m, x in enumerate(X):
        mu, lv = model._encode(m, x, want_logvar=True)                 # fp32, as the kernel reads them
        z = (mu + np.exp(0.5 * lv) * eps).astype(np.float64)            # z in fp32, as the kernel forms it
        out.append(np.sum(-0.5 * z ** 2 + 0.5 * e ** 2 + 0.5 * lv.astype(np.float64), axis=1))
    return np.stack(out, 1)


@pytest.mark.parametrize("name", ["c1", "three"])
def test_loglik_k1_identity_with_score_samples(V, name):
    """K = 1 and the same eps row: conditional[n, m, m] = -recon[n, m] and marginal[n, m] = -recon[n, m] + r[n, m]."""
    archs, binary, weights, lam = MODELS[name]()
    B = 32
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(9)
    N = B + 7
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, archs[0]["n_z"])).astype(np.float32)
    recon = model.score_samples(X, eps=eps)["recon"].astype(np.float64)
    ll = model.log_likelihood(X, n_samples=1, eps=eps[:, None, :])
    M = len(archs)
    diag = np.stack([ll["conditional"][:, m, m] for m in range(M)], 1).astype(np.float64)
    want_m = -recon + _r_from_transform(model, X, eps)
    for m in range(M):
        assert np.abs(diag[:, m] + recon[:, m]).max() <= 1e-6 * np.abs(recon[:, m]).max(), m
        assert np.abs(ll["marginal"][:, m] - want_m[:, m]).max() <= 1e-6 * np.abs(want_m[:, m]).max(), m


def test_loglik_jensen_and_merge(V):
    """With eps slices of one draw: every output at K is log mean_k exp(K = 1 value on slice k), so it lies between the mean
    and the max of the K = 1 values and equals their float64 log-mean-exp (a wrong - log K or LSE merge fails here)."""
    archs, binary, weights, lam = MODELS["three"]()
    B = 16
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(12)
    N, K = 2 * B + 1, B + 5                         # K > B: the running state spans two passes
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, K, 12)).astype(np.float32)
    full = model.log_likelihood(X, n_samples=K, eps=eps)
    ones = [model.log_likelihood(X, n_samples=1, eps=eps[:, k:k + 1]) for k in range(K)]
    for key in full:
        f = np.asarray(full[key], np.float64)
        per_k = np.stack([np.asarray(o[key], np.float64) for o in ones], 0)        # [K, N, ...]
        tol = 1e-5 * np.abs(per_k).max()
        assert np.all(f >= per_k.mean(0) - tol), key
        assert np.all(f <= per_k.max(0) + tol), key
        lme = logsumexp(per_k, 0) - np.log(K)
        assert np.abs(f - lme).max() <= tol, key


def test_loglik_determinism_and_internal_eps(V):
    archs, binary, weights, lam = c1_like()
    B = 16
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(2)
    N, K = 2 * B + 1, 2 * B + 3
    X = synth_batch(rng, N, [784, 147], binary)
    eps = rng.standard_normal((N, K, 20)).astype(np.float32)
    a = model.log_likelihood(X, n_samples=K, eps=eps)
    b = model.log_likelihood(X, n_samples=K, eps=eps)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    a = model.log_likelihood(X, n_samples=K)
    b = model.log_likelihood(X, n_samples=K)
    for d in (a, b):
        for v in d.values():
            assert np.all(np.isfinite(v))
    for key in a:
        assert np.any(a[key] != b[key]), key


def _train_state(model, n_hist):
    m, v, step = model.get_opt_state()
    return model.get_params(), m, v, step, model.cost_history(n_hist)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loglik_has_no_side_effects(V, dtype):
    """partial_fit -> log_likelihood -> partial_fit, and around a partial_fit_steps replay: bitwise the run without it."""
    archs, binary, weights, lam = c1_like()
    B = 24
    rng = np.random.default_rng(21)
    X = synth_batch(rng, 6 * B, [784, 147], binary)
    eps = rng.standard_normal((6 * B, 20)).astype(np.float32)
    Xs = synth_batch(rng, 2 * B + 7, [784, 147], binary)
    eps_s = rng.standard_normal((2 * B + 7, B + 3, 20)).astype(np.float32)
    runs = []
    for with_ll in (False, True):
        model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, dtype)
        model.partial_fit([x[:B] for x in X], eps[:B])
        if with_ll:
            model.log_likelihood(Xs, n_samples=5)
        model.partial_fit([x[B:2 * B] for x in X], eps[B:2 * B])
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:])
        if with_ll:
            model.log_likelihood(Xs, n_samples=B + 3, eps=eps_s)
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append(_train_state(model, 10))
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_loglik_errors(V):
    archs, binary, weights, lam = c1_like()
    B = 16
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(1)
    X = synth_batch(rng, 9, [784, 147], binary)
    with pytest.raises(ValueError):
        model.log_likelihood(X, n_samples=0)
    with pytest.raises(ValueError):
        model.log_likelihood(X, n_samples=4, eps=np.zeros((9, 3, 20), np.float32))     # K does not match
    with pytest.raises(ValueError):
        model.log_likelihood(X, n_samples=4, eps=np.zeros((9, 20), np.float32))        # not [N, K, n_z]
    with pytest.raises(ValueError):
        model.log_likelihood([X[0], X[1][:8]])                                         # row counts differ
    with pytest.raises(ValueError):
        model.log_likelihood([X[0]])                                                   # one modality short
    # the C ABI: n_samples < 1, NULL out_dev, x_ld below n_input -> non-zero with a message
    L = model._L
    ts = [torch.from_numpy(x).to(model.device) for x in X]
    out = torch.empty((9, 8), dtype=torch.float32, device=model.device)
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    lds = (C.c_int32 * 2)(784, 147)
    assert L.avae_loglik(model._h, ptrs, lds, 9, 0, None, out.data_ptr(), None) != 0
    assert b"n_samples" in L.avae_last_error(model._h)
    assert L.avae_loglik(model._h, ptrs, lds, 9, 2, None, None, None) != 0
    assert b"out_dev" in L.avae_last_error(model._h)
    bad = (C.c_int32 * 2)(784, 100)
    assert L.avae_loglik(model._h, ptrs, bad, 9, 2, None, out.data_ptr(), None) != 0
    assert b"x_ld" in L.avae_last_error(model._h)
    assert L.avae_loglik(model._h, ptrs, lds, 0, 2, None, None, None) == 0      # zero rows: a no-op
    torch.cuda.synchronize()
    # the handle still works
    eps = rng.standard_normal((9, 3, 20)).astype(np.float32)
    assert_columns(model.log_likelihood(X, n_samples=3, eps=eps), ref_loglik(ref, X, eps), 1e-5, "after errors ")
