"""score_samples_masked / log_likelihood_masked / train() on presence-carrying data sets, on a real MI355X (include/avae.h,
DESIGN.md section 12): parity with the fp64 (and quant='bf16') reference of tests/masked_scoring_reference.py at the tolerances of
tests/test_gpu_score.py / tests/test_gpu_loglik.py, the bitwise ties with the unmasked calls, absent entries that change no bit,
the identity with evaluate_cost(present=), no side effects on training, one draw counter, errors, and the masked train loop
against a hand-written one.

Presence patterns are deterministic (masked_scoring_reference.all_patterns_mask: row n -> a fixed permutation of n mod 2^M) and
batch_size >= 2^M everywhere, so every pattern, the empty one included, occurs in every full chunk (asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_arch, shadow_err, synth_batch
from masked_reference import masked_cost_and_grads
from masked_scoring_reference import (all_patterns_mask, assert_masked_columns, has_every_pattern, ref_loglik_masked,
                                      ref_scores_masked)
from oracle import vae_assoc_oracle as O
from test_gpu_score import MODELS, build_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _pair(V, name, dtype, B):
    archs, binary, weights, lam = MODELS[name]()
    fp32 = dtype == "fp32"
    model, ref = build_pair(V, archs, binary, weights, lam, "relu" if fp32 else "softplus", B, dtype,
                            quant=None if fp32 else "bf16")
    return archs, binary, weights, lam, model, ref, (1e-5 if fp32 else 3e-3)


def _assert_chunks_have_every_pattern(p, B):
    assert B >= 1 << p.shape[1]
    for r0 in range(0, p.shape[0] - B + 1, B):
        assert has_every_pattern(p[r0:r0 + B]), r0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _garbage(X, p, rng):
    """X with NaN / Inf / 1e30 in every absent entry"""
    out = []
    for m, x in enumerate(X):
        g = x.copy()
        junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), size=x.shape)
        out.append(np.where(p[:, m:m + 1], g, junk).astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["c1", "three", "conv"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_score_parity(V, name, dtype):
    """N < B, N = B and N = 2B + 3 rows, cross terms included, against the reference: 1e-5 of the column's max (fp32 vs fp64),
    3e-3 (bf16 vs the quant='bf16' oracle); NaN exactly where the reference has it."""
    B = 24
    archs, binary, weights, lam, model, ref, tol = _pair(V, name, dtype, B)
    M = len(archs)
    rng = np.random.default_rng(11)
    for N in (B - 5, B, 2 * B + 3):
        p = all_patterns_mask(N, M, shift=N)
        _assert_chunks_have_every_pattern(p, B)
        assert has_every_pattern(p)
        X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
        eps = rng.standard_normal((N, archs[0]["n_z"])).astype(np.float32)
        got = model.score_samples_masked(X, p, eps=eps, cross_modal=True)
        assert isinstance(got["cost"], np.ndarray) and got["cost"].shape == (N,)
        assert got["recon"].shape == (N, M) and got["cross"].shape == (N, M, M)
        assert_masked_columns(got, ref_scores_masked(ref, X, p, eps, cross=True), tol, "%s/%s N=%d " % (name, dtype, N))
        for key in ("recon", "latent"):                      # absent entries are +0.0, not -0.0
            assert np.all(_bits(got[key])[~p] == 0), key
        plain = model.score_samples_masked(X, p, eps=eps)
        assert "cross" not in plain
        for key in ("cost", "recon", "latent", "assoc"):
            assert _same_bits(plain[key], got[key]), key


@pytest.mark.parametrize("name", ["c1", "three", "conv"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_loglik_parity(V, name, dtype):
    """(N, K) over N < B, N = B, N = 2B + 3 and K < B, K = B, K > B (several rows per pass, one row per pass, one row over several
    passes), every pattern among the rows of every case."""
    B = 16
    archs, binary, weights, lam, model, ref, tol = _pair(V, name, dtype, B)
    M = len(archs)
    rng = np.random.default_rng(17)
    for N, K in ((2 * B + 3, 5), (B, B), (B - 5, B + 3), (B - 5, 5), (2 * B + 3, B)):
        p = all_patterns_mask(N, M, shift=K)
        assert B >= 1 << M and has_every_pattern(p)
        X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
        eps = rng.standard_normal((N, K, archs[0]["n_z"])).astype(np.float32)
        got = model.log_likelihood_masked(X, p, n_samples=K, eps=eps)
        assert got["marginal"].shape == (N, M) and got["joint"].shape == (N, M) and got["conditional"].shape == (N, M, M)
        assert_masked_columns(got, ref_loglik_masked(ref, X, p, eps), tol, "%s/%s N=%d K=%d " % (name, dtype, N, K))
        empty = ~p.any(1)
        assert empty.any()
        for v in got.values():
            assert np.all(np.isnan(v[empty]))


# ------------------------------------------------------------------------------------------------ bitwise ties
@pytest.mark.parametrize("name", ["c1", "three"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_score_bitwise_ties(V, name, dtype):
    B = 16
    archs, binary, weights, lam, model, ref, tol = _pair(V, name, dtype, B)
    M = len(archs)
    rng = np.random.default_rng(23)
    N = 2 * B + 3
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)          # finite everywhere: the unmasked call reads it all
    eps = rng.standard_normal((N, archs[0]["n_z"])).astype(np.float32)
    un = model.score_samples(X, eps=eps, cross_modal=True)
    # all present == the unmasked call
    full = model.score_samples_masked(X, np.ones((N, M), np.uint8), eps=eps, cross_modal=True)
    for key in un:
        assert _same_bits(full[key], un[key]), key
    # present entries of every column but cost == the unmasked call's
    p = all_patterns_mask(N, M)
    _assert_chunks_have_every_pattern(p, B)
    got = model.score_samples_masked(X, p, eps=eps, cross_modal=True)
    for key in ("recon", "latent"):
        assert np.array_equal(_bits(got[key])[p], _bits(un[key])[p]), key
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
    for k, (i, j) in enumerate(pairs):
        both = p[:, i] & p[:, j]
        assert np.array_equal(_bits(got["assoc"][:, k])[both], _bits(un["assoc"][:, k])[both]), (i, j)
        assert np.all(_bits(got["assoc"][:, k])[~both] == 0)
    for s in range(M):
        for d in range(M):
            both = p[:, s] & p[:, d]
            assert np.array_equal(_bits(got["cross"][:, s, d])[both], _bits(un["cross"][:, s, d])[both]), (s, d)
            assert np.all(np.isnan(got["cross"][:, s, d][~both]))
    # garbage in every absent entry, presence as a device bool tensor / int64 array: the same bits; so does a second call
    for pp in (torch.from_numpy(p).to(model.device), p.astype(np.int64) * 7):
        again = model.score_samples_masked(_garbage(X, p, rng), pp, eps=eps, cross_modal=True)
        for key in got:
            assert _same_bits(again[key], got[key]), key
    # a column absent on every row: X[m] = None == garbage there
    p1 = p.copy()
    p1[:, M - 1] = False
    a = model.score_samples_masked(_garbage(X, p1, rng), p1, eps=eps, cross_modal=True)
    Xn = list(X)
    Xn[M - 1] = None
    b = model.score_samples_masked(Xn, p, eps=eps, cross_modal=True)       # (p's own last column is overruled by the None)
    for key in a:
        assert _same_bits(a[key], b[key]), key


@pytest.mark.parametrize("name", ["c1", "three"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_loglik_bitwise_ties(V, name, dtype):
    B = 16
    archs, binary, weights, lam, model, ref, tol = _pair(V, name, dtype, B)
    M = len(archs)
    rng = np.random.default_rng(29)
    for N, K in ((2 * B + 3, 5), (B + 1, B + 3)):
        X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
        eps = rng.standard_normal((N, K, archs[0]["n_z"])).astype(np.float32)
        un = model.log_likelihood(X, n_samples=K, eps=eps)
        full = model.log_likelihood_masked(X, np.ones((N, M), bool), n_samples=K, eps=eps)
        for key in un:
            assert _same_bits(full[key], un[key]), key
        p = all_patterns_mask(N, M, shift=1)
        assert has_every_pattern(p)
        got = model.log_likelihood_masked(X, p, n_samples=K, eps=eps)
        assert np.array_equal(_bits(got["marginal"])[p], _bits(un["marginal"])[p])
        assert np.all(np.isnan(got["marginal"][~p])) and np.all(np.isnan(got["joint"][~p]))
        assert np.all(np.isfinite(got["joint"][p]))
        both = p[:, :, None] & p[:, None, :]
        assert np.array_equal(_bits(got["conditional"])[both], _bits(un["conditional"])[both])
        assert np.all(np.isnan(got["conditional"][~both]))
        # rows that have only s: joint[s] is marginal[s], bit for bit
        for s in range(M):
            only = p[:, s] & (p.sum(1) == 1)
            assert only.any()
            assert np.array_equal(_bits(got["joint"][:, s])[only], _bits(got["marginal"][:, s])[only]), s
        again = model.log_likelihood_masked(_garbage(X, p, rng), torch.from_numpy(p).to(model.device), n_samples=K, eps=eps)
        for key in got:
            assert _same_bits(again[key], got[key]), key
        p1 = p.copy()
        p1[:, 0] = False
        a = model.log_likelihood_masked(_garbage(X, p1, rng), p1, n_samples=K, eps=eps)
        b = model.log_likelihood_masked([None] + list(X[1:]), p, n_samples=K, eps=eps)
        for key in a:
            assert _same_bits(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ identity with evaluate_cost
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_score_identity_with_evaluate_cost(V, dtype):
    """rows = B, one eps: evaluate_cost(present=) == sum_m w_m [(1/B) sum latent + (binary ? 1/B : 1) sum recon] + lambda sum
    assoc over the masked columns, with no need for the presence (1e-5 fp32, 1e-4 bf16)."""
    for name in ("c1", "three"):
        B = 32
        archs, binary, weights, lam, model, ref, _ = _pair(V, name, dtype, B)
        M = len(archs)
        rng = np.random.default_rng(8)
        X = synth_batch(rng, B, [a["n_input"] for a in archs], binary)
        eps = rng.standard_normal((B, archs[0]["n_z"])).astype(np.float32)
        p = all_patterns_mask(B, M, shift=2)
        _assert_chunks_have_every_pattern(p, B)
        sc = model.score_samples_masked(X, p, eps=eps)
        c_eval = model.evaluate_cost(X, eps, present=p)
        r, k, a = (sc[key].astype(np.float64) for key in ("recon", "latent", "assoc"))
        total = sum(w * (k[:, m].sum() / B + (r[:, m].sum() / B if b else r[:, m].sum()))
                    for m, (w, b) in enumerate(zip(weights, binary)))
        total += lam * a.sum()
        tol = 1e-5 if dtype == "fp32" else 1e-4
        print("%s/%s: columns %.7f, evaluate_cost %.7f" % (name, dtype, total, c_eval))
        assert abs(total - c_eval) <= tol * abs(c_eval), "%s/%s: %.7f vs evaluate_cost %.7f" % (name, dtype, total, c_eval)


# ------------------------------------------------------------------------------------------------ state and interleaving
def _train_state(model, n_hist):
    m, v, step = model.get_opt_state()
    return model.get_params(), m, v, step, model.cost_history(n_hist), model.get_grads()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_scoring_has_no_side_effects(V, dtype):
    """partial_fit -> masked scoring -> partial_fit (plain and masked steps), and around a partial_fit_steps replay: parameters,
    Adam slots, step counter, cost history and the last gradient are bitwise those of the run without the scoring calls."""
    archs, binary, weights, lam = MODELS["c1"]()
    B = 24
    rng = np.random.default_rng(21)
    X = synth_batch(rng, 6 * B, [784, 147], binary)
    eps = rng.standard_normal((6 * B, 20)).astype(np.float32)
    pt = all_patterns_mask(6 * B, 2, shift=3)
    Ns = 2 * B + 7
    Xs = synth_batch(rng, Ns, [784, 147], binary)
    ps = all_patterns_mask(Ns, 2)
    eps_s = rng.standard_normal((Ns, B + 3, 20)).astype(np.float32)
    runs = []
    for with_calls in (False, True):
        model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, dtype)
        model.partial_fit([x[:B] for x in X], eps[:B])
        if with_calls:
            model.score_samples_masked(Xs, ps, cross_modal=True)
            model.log_likelihood_masked(Xs, ps, n_samples=5)
        model.partial_fit([x[B:2 * B] for x in X], eps[B:2 * B], present=pt[B:2 * B])
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:])
        if with_calls:
            model.score_samples_masked([Xs[0], None], ps, eps=eps[:Ns])
            model.log_likelihood_masked(Xs, ps, n_samples=B + 3, eps=eps_s)
        model.partial_fit_steps([x[2 * B:] for x in X], 4, eps=eps[2 * B:], present=pt[2 * B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append(_train_state(model, 10))
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_masked_and_unmasked_calls_share_one_draw_counter(V):
    """Internal eps: an all-present masked call is the unmasked call at the same draw, and either kind advances the counter."""
    archs, binary, weights, lam = MODELS["c1"]()
    B = 16
    N = 2 * B + 1
    X = synth_batch(np.random.default_rng(2), N, [784, 147], binary)
    ones = np.ones((N, 2), bool)
    seqs = []
    for masked_first in (False, True):
        model, _ = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
        out = []
        for i in range(4):
            use_masked = (i % 2 == 0) == masked_first
            if i < 2:
                out.append(model.score_samples_masked(X, ones) if use_masked else model.score_samples(X))
            else:
                out.append(model.log_likelihood_masked(X, ones, n_samples=3) if use_masked else model.log_likelihood(X, n_samples=3))
        seqs.append(out)
    for a, b in zip(*seqs):                        # call i of both sequences: the same draw, whichever kind made it
        for key in a:
            assert _same_bits(a[key], b[key]), key
    assert np.any(seqs[0][0]["recon"] != seqs[0][1]["recon"])                  # ... and successive draws differ
    assert np.any(seqs[0][2]["marginal"] != seqs[0][3]["marginal"])


# ------------------------------------------------------------------------------------------------ errors
def test_masked_scoring_errors(V):
    archs, binary, weights, lam = MODELS["c1"]()
    B = 16
    model, ref = build_pair(V, archs, binary, weights, lam, "relu", B, "fp32")
    rng = np.random.default_rng(1)
    N = 9
    X = synth_batch(rng, N, [784, 147], binary)
    p = all_patterns_mask(N, 2)
    for bad in (np.ones((N + 1, 2), bool), np.ones((N, 1), bool), np.ones((N, 3), bool), np.ones((N,), bool)):
        with pytest.raises(ValueError):
            model.score_samples_masked(X, bad)
        with pytest.raises(ValueError):
            model.log_likelihood_masked(X, bad, n_samples=2)
    with pytest.raises(ValueError):
        model.score_samples_masked([X[0]], p)
    with pytest.raises(ValueError):
        model.score_samples_masked([X[0], X[1][:8]], p)
    with pytest.raises(ValueError):
        model.score_samples_masked(X, p, eps=np.zeros((8, 20), np.float32))
    with pytest.raises(ValueError):
        model.log_likelihood_masked(X, p, n_samples=0)
    with pytest.raises(ValueError):
        model.log_likelihood_masked(X, p, n_samples=4, eps=np.zeros((N, 3, 20), np.float32))
    # the C ABI: NULL present_dev, unknown flags, n_samples < 1, NULL out_dev -> non-zero with a message, no fault
    L = model._L
    ts = [torch.from_numpy(x).to(model.device) for x in X]
    pd = torch.from_numpy(p.astype(np.uint8)).to(model.device)
    out = torch.empty((N, 64), dtype=torch.float32, device=model.device)
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    lds = (C.c_int32 * 2)(784, 147)
    assert L.avae_score_masked(model._h, ptrs, lds, None, N, None, 0, out.data_ptr(), None) != 0
    assert b"present_dev" in L.avae_last_error(model._h)
    assert L.avae_loglik_masked(model._h, ptrs, lds, None, N, 2, None, out.data_ptr(), None) != 0
    assert b"present_dev" in L.avae_last_error(model._h)
    assert L.avae_score_masked(model._h, ptrs, lds, pd.data_ptr(), N, None, 6, out.data_ptr(), None) != 0
    assert b"flags" in L.avae_last_error(model._h)
    assert L.avae_loglik_masked(model._h, ptrs, lds, pd.data_ptr(), N, 0, None, out.data_ptr(), None) != 0
    assert b"n_samples" in L.avae_last_error(model._h)
    assert L.avae_score_masked(model._h, ptrs, lds, pd.data_ptr(), N, None, 0, None, None) != 0
    assert b"out_dev" in L.avae_last_error(model._h)
    assert L.avae_score_masked(model._h, ptrs, lds, pd.data_ptr(), 0, None, 0, None, None) == 0      # zero rows: a no-op
    assert L.avae_loglik_masked(model._h, ptrs, lds, pd.data_ptr(), 0, 2, None, None, None) == 0
    torch.cuda.synchronize()
    # the handle still works
    eps = rng.standard_normal((N, 20)).astype(np.float32)
    assert_masked_columns(model.score_samples_masked(X, p, eps=eps), ref_scores_masked(ref, X, p, eps), 1e-5, "after errors ")


# ------------------------------------------------------------------------------------------------ train()
TRAIN_ARCHS = [make_arch("image", 784, 32, 24, 4), make_arch("joint", 147, 24, 16, 4)]
TRAIN_KW = dict(binary=[True, False], weights=[50.0, 1.0], assoc_lambda=8.0)


def _hand_masked_loop(dataset, data, present, p_init, eps_all, B, epochs, early_stop):
    """The loop of train() written out by hand on the oracle: masked cost and gradient of tests/masked_reference.py, the oracle's
    Adam, presence rows taken from the data set next to its data rows."""
    np.random.seed(42)
    ds = dataset.construct_datasets(data.copy(), present=present.copy())
    ref = O.OracleAssocVAE(TRAIN_ARCHS, TRAIN_KW["binary"], "relu", TRAIN_KW["weights"], TRAIN_KW["assoc_lambda"], 1e-3, B,
                           params_flat=p_init.astype(np.float64))
    n = ds.train._data.shape[0]
    split = lambda a: [a[:, :784], a[:, 784:]]
    k, hist, valid = 0, [], None

    def cost_grad(x, p):
        nonlocal k
        c, g = masked_cost_and_grads(TRAIN_ARCHS, ref.get_params(), split(x), eps_all[k], p, TRAIN_KW["binary"], TRAIN_KW["weights"],
                                     TRAIN_KW["assoc_lambda"], "relu")
        k += 1
        return c, g

    for epoch in range(epochs):
        avg = 0.0
        if early_stop and epoch % early_stop == 0:
            nv = ds.validation._data.shape[0] // B
            cur = 0
            for _ in range(nv):
                x, _l = ds.validation.next_batch(B)
                cur += cost_grad(x, ds.validation.last_present())[0] / nv
            if valid is not None and cur > valid:
                break
            valid = cur
        for _ in range(n // B):
            x, _l = ds.train.next_batch(B)
            c, g = cost_grad(x, ds.train.last_present())
            ref.apply_gradients(g)
            avg += c / n * B
            hist.append(avg)
    return hist, ref.get_params()


@pytest.mark.parametrize("feeder", ["host", "device"])
def test_masked_train_loop_matches_hand_written_loop(V, feeder):
    """train() on a presence-carrying data set (host DataSet and DeviceDataSet), early_stop on: avg_cost_hist (rtol 2e-5) and the
    parameters (5e-5) of the hand-written masked loop, as test_train_loop_matches_oracle_loop compares the unmasked one."""
    from vae_assoc_amd import dataset
    rng = np.random.default_rng(6)
    N, B, epochs = 400, 32, 3
    data = np.concatenate(synth_batch(rng, N, [784, 147], [True, False]), axis=1)
    present = all_patterns_mask(N, 2, shift=1)
    eps_all = rng.standard_normal((96, B, 4)).astype(np.float32)

    class Fed(V.AssocVariationalAutoEncoder):
        _k = 0

        def partial_fit(self, X, eps=None, return_cost=True, present=None):
            e = eps_all[Fed._k]
            Fed._k += 1
            return super().partial_fit(X, e, return_cost, present=present)

        def partial_fit_steps(self, X, n_steps, eps=None, return_cost=True, present=None):
            e = np.concatenate(eps_all[Fed._k:Fed._k + n_steps])
            Fed._k += n_steps
            return super().partial_fit_steps(X, n_steps, e, return_cost, present=present)

        def evaluate_cost(self, X, eps=None, present=None):
            e = eps_all[Fed._k]
            Fed._k += 1
            return super().evaluate_cost(X, e, present=present)

    np.random.seed(42)
    ds = dataset.construct_datasets(data.copy(), present=present.copy())
    if feeder == "device":
        ds = dataset.to_device(ds)
        assert ds.train._present.dtype == torch.uint8 and ds.train._present.is_cuda
    orig = V.AssocVariationalAutoEncoder
    V.AssocVariationalAutoEncoder = Fed
    try:
        model, hist = V.train(ds, TRAIN_ARCHS, batch_size=B, training_epochs=epochs, display_step=10, early_stop=1,
                              compute_dtype="fp32", seed=8, **TRAIN_KW)
    finally:
        V.AssocVariationalAutoEncoder = orig
    p_init = V.AssocVariationalAutoEncoder(TRAIN_ARCHS, binary=[True, False], transfer_fct="relu", batch_size=B,
                                           compute_dtype="fp32", seed=8).get_params()
    h_ref, p_ref = _hand_masked_loop(dataset, data, present, p_init, eps_all, B, epochs, 1)
    assert len(hist) == len(h_ref) == epochs * (320 // B)
    print("max rel hist err %.3e, max |dtheta| %.3e" % (np.max(np.abs(np.array(hist) - h_ref) / np.abs(h_ref)),
                                                       np.abs(model.get_params() - p_ref).max()))
    assert np.allclose(hist, h_ref, rtol=2e-5)
    assert np.abs(model.get_params() - p_ref).max() <= 5e-5


def test_masked_train_refuses_data_parallel_model(V):
    """A one-rank comm='ipc' model is a data-parallel replica: train() on a data set with presence refuses before any step."""
    from vae_assoc_amd import dataset
    rng = np.random.default_rng(3)
    data = np.concatenate(synth_batch(rng, 100, [784, 147], [True, False]), axis=1)
    ds = dataset.construct_datasets(data, present=all_patterns_mask(100, 2))
    with pytest.raises(RuntimeError, match="one replica"):
        V.train(ds, TRAIN_ARCHS, batch_size=16, training_epochs=1, compute_dtype="fp32", comm="ipc", **TRAIN_KW)
    model = V.AssocVariationalAutoEncoder(TRAIN_ARCHS, transfer_fct="relu", batch_size=16, compute_dtype="fp32", comm="ipc",
                                          **TRAIN_KW)
    with pytest.raises(RuntimeError, match="one replica"):
        V.train_loop(model, ds, TRAIN_ARCHS, 16, training_epochs=1)
    assert model.get_opt_state()[2] == 0
    # scoring itself works on such a replica, as score_samples does: local rows, no collective
    X = [data[:20, :784], data[:20, 784:]]
    p = all_patterns_mask(20, 2)
    eps = rng.standard_normal((20, 4)).astype(np.float32)
    plain = V.AssocVariationalAutoEncoder(TRAIN_ARCHS, transfer_fct="relu", batch_size=16, compute_dtype="fp32", **TRAIN_KW)
    plain.set_params(model.get_params())
    a, b = model.score_samples_masked(X, p, eps=eps), plain.score_samples_masked(X, p, eps=eps)
    for key in a:
        assert _same_bits(a[key], b[key]), key
