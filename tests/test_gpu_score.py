"""score_samples / avae_score on a real MI355X: per-row cost terms and cross-modal prediction error against the CPU oracle
(fp64, and quant='bf16' for the bf16 path), any row count, the identity with evaluate_cost, and no side effects on training."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_arch, shadow_err, synth_batch
from oracle import vae_assoc_oracle as O
from scoring_reference import recon_rows, ref_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def build_pair(V, archs, binary, weights, lam, act, B, dtype, seed=5, quant=None):
    """HIP model + oracle on the same weights, with non-zero biases (the folded-bias column)."""
    model = V.AssocVariationalAutoEncoder(archs, binary=binary, transfer_fct=act, weights=weights, assoc_lambda=lam,
                                          learning_rate=1e-3, batch_size=B, compute_dtype=dtype, seed=seed)
    rng = np.random.default_rng(seed)
    p0 = model.get_params()
    off = 0
    for na in archs:
        for name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            if len(shp) == 1:
                p0[off:off + n] = 0.05 * rng.standard_normal(n)
            off += n
    model.set_params(p0)
    ref = O.OracleAssocVAE(archs, binary, act, weights, lam, 1e-3, B, params_flat=p0.astype(np.float64), quant=quant)
    return model, ref


def assert_columns(got, want, tol, what=""):
    for key, r in want.items():
        g = np.asarray(got[key], np.float64)
        assert g.shape == r.shape, "%s%s shape %s vs %s" % (what, key, g.shape, r.shape)
        g2, r2 = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
        for c in range(r2.shape[1]):
            scale = max(np.abs(r2[:, c]).max(), 1e-30) if r2.shape[0] else 1.0
            err = np.abs(g2[:, c] - r2[:, c]).max() if r2.shape[0] else 0.0
            assert err <= tol * scale, "%s%s column %d: max err %.3e vs max |ref| %.3e" % (what, key, c, err, scale)


def c1_like(nz=20):
    return ([make_arch("image", 784, 64, 48, nz), make_arch("joint", 147, 48, 32, nz)], [True, False], [50.0, 1.0], 8.0)


def three_mod():
    return ([make_arch("a", 96, 40, 32, 12), make_arch("b", 40, 32, 24, 12), make_arch("c", 24, 24, 16, 12)],
            [True, False, False], [2.0, 1.0, 0.5], 0.7)


def conv_pair():
    img = dict(make_arch("image", 784, 16, 64, 20), hidden_conv=True, n_hidden_gener_1=64, n_hidden_gener_2=16)
    return ([img, make_arch("joint", 147, 48, 32, 20)], [True, False], [50.0, 1.0], 8.0)


MODELS = {"c1": c1_like, "three": three_mod, "conv": conv_pair}


@pytest.mark.parametrize("name", ["c1", "three", "conv"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_parity(V, name, dtype):
    """Every column against the fp64 oracle (fp32 compute, 1e-5 of the column's max) or the quant='bf16' oracle (bf16 compute,
    softplus, 3e-3); 2B+3 rows, so a chunk boundary and a partial chunk are crossed."""
    archs, binary, weights, lam = MODELS[name]()
    B = 24
    fp32 = dtype == "fp32"
    act = "relu" if fp32 else "softplus"
    model, ref = build_pair(V, archs, binary, weights, lam, act, B, dtype, quant=None if fp32 else "bf16")
    rng = np.random.default_rng(11)
    N = 2 * B + 3
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, archs[0]["n_z"])).astype(np.float32)
    got = model.score_samples(X, eps=eps, cross_modal=True)
    assert isinstance(got["cost"], np.ndarray) and got["cost"].shape == (N,)
    M = len(archs)
    assert got["recon"].shape == (N, M) and got["latent"].shape == (N, M) and got["assoc"].shape == (N, M * (M - 1) // 2)
    assert got["cross"].shape == (N, M, M)
    assert_columns(got, ref_scores(ref, X, eps, cross=True), 1e-5 if fp32 else 3e-3, "%s/%s " % (name, dtype))
    plain = model.score_samples(X, eps=eps)
    assert "cross" not in plain
    for key in ("cost", "recon", "latent", "assoc"):
        assert np.array_equal(plain[key], got[key]), key


@pytest.mark.parametrize("nz", [48, 64])
def test_score_wide_latents(V, nz):
    archs, binary, weights, lam = c1_like(nz)
    B = 16
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(nz)
    N = B + 5
    X = synth_batch(rng, N, [784, 147], binary)
    eps = rng.standard_normal((N, nz)).astype(np.float32)
    assert_columns(model.score_samples(X, eps=eps, cross_modal=True), ref_scores(ref, X, eps, cross=True), 1e-5, "nz=%d " % nz)


def test_score_row_counts_and_chunking(V):
    """Column slices of one [N, 931] matrix, rows 0 .. 3B+5; scoring [0,N) equals scoring [0,k) and [k,N)."""
    archs, binary, weights, lam = c1_like()
    B = 20
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(3)
    Nmax = 3 * B + 5
    data = np.concatenate(synth_batch(rng, Nmax, [784, 147], binary), axis=1)
    eps_all = rng.standard_normal((Nmax, 20)).astype(np.float32)
    dev = torch.from_numpy(data).to(model.device)
    for N in (0, 1, 7, B - 1, B, B + 1, Nmax):
        X = [dev[:N, :784], dev[:N, 784:]]                 # strided views, row stride 931
        got = model.score_samples(X, eps=torch.from_numpy(eps_all[:N]).to(model.device), cross_modal=True)
        assert torch.is_tensor(got["cost"]) and got["cost"].device == model.device and got["cost"].shape == (N,)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        if N:
            assert_columns(got, ref_scores(ref, [data[:N, :784], data[:N, 784:]], eps_all[:N], cross=True), 1e-5, "N=%d " % N)
    X = [data[:, :784], data[:, 784:]]
    full = model.score_samples(X, eps=eps_all, cross_modal=True)
    for k in (1, B - 3, B, 2 * B + 1):
        a = model.score_samples([x[:k] for x in X], eps=eps_all[:k], cross_modal=True)
        b = model.score_samples([x[k:] for x in X], eps=eps_all[k:], cross_modal=True)
        for key in full:
            joined = np.concatenate([a[key], b[key]])
            assert np.abs(joined - full[key]).max() <= 1e-6 * np.abs(full[key]).max(), (k, key)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_identity_with_evaluate_cost(V, dtype):
    """rows = B, one eps: evaluate_cost == sum_m w_m [mean latent + (binary ? mean recon : sum recon)] + lambda sum_p sum_n assoc."""
    for name in ("c1", "three"):
        archs, binary, weights, lam = MODELS[name]()
        B = 32
        model, _ = build_pair(V, archs, binary, weights, lam, "relu" if dtype == "fp32" else "softplus", B, dtype)
        rng = np.random.default_rng(8)
        X = synth_batch(rng, B, [a["n_input"] for a in archs], binary)
        eps = rng.standard_normal((B, archs[0]["n_z"])).astype(np.float32)
        sc = model.score_samples(X, eps=eps)
        c_eval = model.evaluate_cost(X, eps)
        r, k, a = (sc[key].astype(np.float64) for key in ("recon", "latent", "assoc"))
        total = sum(w * (k[:, m].mean() + (r[:, m].mean() if b else r[:, m].sum())) for m, (w, b) in enumerate(zip(weights, binary)))
        total += lam * a.sum()
        tol = 1e-5 if dtype == "fp32" else 1e-4
        assert abs(total - c_eval) <= tol * abs(c_eval), "%s/%s: %.7f vs evaluate_cost %.7f" % (name, dtype, total, c_eval)


def test_score_internal_eps(V):
    archs, binary, weights, lam = c1_like()
    B = 16
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    X = synth_batch(np.random.default_rng(2), 2 * B + 1, [784, 147], binary)
    a = model.score_samples(X, cross_modal=True)
    b = model.score_samples(X, cross_modal=True)
    for key in ("latent", "assoc", "cross"):
        assert np.array_equal(a[key], b[key]), key
    assert np.any(a["recon"] != b["recon"])
    for d in (a, b):
        for v in d.values():
            assert np.all(np.isfinite(v))


def test_score_cross_diagonal_is_noise_free_reconstruction(V):
    archs, binary, weights, lam = c1_like()
    B = 16
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    N = B + 3
    X = synth_batch(np.random.default_rng(5), N, [784, 147], binary)
    cr = model.score_samples(X, cross_modal=True)["cross"]
    rec = model.reconstruct(X, eps=[np.zeros((N, 20), np.float32)] * 2)
    for m in range(2):
        host = recon_rows(X[m].astype(np.float64), rec[m].astype(np.float64), binary[m])
        assert np.abs(cr[:, m, m] - host).max() <= 1e-5 * np.abs(host).max(), m


def _train_state(model, n_hist):
    m, v, step = model.get_opt_state()
    return model.get_params(), m, v, step, model.cost_history(n_hist)


def _assert_same_state(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_has_no_side_effects(V, dtype):
    """partial_fit -> score -> partial_fit, and around a partial_fit_steps replay: bitwise the run without the score call."""
    archs, binary, weights, lam = c1_like()
    B = 24
    rng = np.random.default_rng(21)
    X = synth_batch(rng, 6 * B, [784, 147], binary)
    eps = rng.standard_normal((6 * B, 20)).astype(np.float32)
    Xs = synth_batch(rng, 2 * B + 7, [784, 147], binary)
    runs = []
    for with_score in (False, True):
        model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, dtype)
        model.partial_fit([x[:B] for x in X], eps[:B])
        if with_score:
            model.score_samples(Xs, cross_modal=True)
        model.partial_fit([x[B:2 * B] for x in X], eps[B:2 * B])
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:])
        if with_score:
            model.score_samples(Xs, eps=eps[:2 * B + 7])
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append(_train_state(model, 10))
    _assert_same_state(runs[0], runs[1])


def test_score_errors(V):
    archs, binary, weights, lam = c1_like()
    B = 16
    model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(1)
    X = synth_batch(rng, 9, [784, 147], binary)
    with pytest.raises(ValueError):
        model.score_samples([X[0]])                              # one modality short
    with pytest.raises(ValueError):
        model.score_samples([X[0], X[1][:8]])                    # row counts differ
    with pytest.raises(ValueError):
        model.score_samples([X[0][:, :700], X[1]])               # wrong width
    with pytest.raises(ValueError):
        model.score_samples(X, eps=np.zeros((8, 20), np.float32))
    # the C ABI: NULL out_dev, x_ld below n_input, unknown flags -> non-zero with a message
    L = model._L
    ts = [torch.from_numpy(x).to(model.device) for x in X]
    out = torch.empty((9, 64), dtype=torch.float32, device=model.device)
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    lds = (C.c_int32 * 2)(784, 147)
    assert L.avae_score(model._h, ptrs, lds, 9, None, 0, None, None) != 0
    assert b"out_dev" in L.avae_last_error(model._h)
    bad = (C.c_int32 * 2)(784, 100)
    assert L.avae_score(model._h, ptrs, bad, 9, None, 0, out.data_ptr(), None) != 0
    assert b"x_ld" in L.avae_last_error(model._h)
    assert L.avae_score(model._h, ptrs, lds, 9, None, 6, out.data_ptr(), None) != 0
    assert b"flags" in L.avae_last_error(model._h)
    assert L.avae_score(model._h, ptrs, lds, 0, None, 0, None, None) == 0      # zero rows: a no-op
    torch.cuda.synchronize()
