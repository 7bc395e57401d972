"""The mixture prior checked without a GPU: the definitions of tests/latent_prior_reference.py against closed forms, the float32
restatement's own error, avae_gmm_plan (host-only: the partition is a function of rows alone, no slice is empty, the scratch is
bounded, the error messages) and the argument handling of the Python helpers.  No model is constructed here."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_prior_reference as P


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    return vae_assoc


# ------------------------------------------------------------------------------------------------ the reference
def test_one_component_gives_the_global_mean_and_total_variance_in_one_step():
    rng = np.random.default_rng(0)
    for nz in (3, 20):
        mu, lv, _ = P.clusters(rng, 200, nz, 4, 3.0)
        for logvar in (lv, None):
            init = {"weights": np.ones(1, np.float32), "means": mu[7:8].copy(), "logvars": np.zeros((1, nz), np.float32)}
            out, bound, n = P.step64(mu, logvar, init)
            x = mu.astype(np.float64)
            v = 0.0 if logvar is None else np.exp(logvar.astype(np.float64)).mean(axis=0)
            assert n == 200 and out["weights"].tolist() == [1.0] and np.isfinite(bound)
            assert np.abs(out["means"][0] - x.mean(axis=0)).max() < 1e-6
            assert np.abs(out["logvars"][0] - np.log(x.var(axis=0) + v)).max() < 1e-6
            out32, _, _ = P.step32(mu, logvar, init)
            assert P.param_err(out32["means"], out["means"]).max() < 1e-5
            assert P.param_err(out32["logvars"], out["logvars"]).max() < 1e-5


def test_the_bound_never_falls_in_float64():
    rng = np.random.default_rng(1)
    for nz, K, N in ((7, 3, 300), (20, 10, 600)):
        mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
        for logvar in (lv, None):
            _, bound, n = P.fit64(mu, logvar, P.start(rng, mu, logvar, K), 30)
            assert n == N and np.isfinite(bound).all()
            # parameters are rounded to float32 between iterations: the bound of the rounded ones may lie a rounding below
            assert (np.diff(bound) >= -1e-6 * (np.abs(bound[:-1]) + nz)).all(), np.diff(bound).min()
            assert bound[-1] > bound[0]


def test_points_equal_textbook_em():
    rng = np.random.default_rng(2)
    mu, _, _ = P.clusters(rng, 400, 5, 3, 3.0)
    prior = P.start(rng, mu, None, 3)
    for _ in range(3):
        w, mean, var = P.textbook_step(mu, prior)
        prior, _, _ = P.step64(mu, None, prior, var_floor=1e-12)
        assert np.abs(prior["weights"] - w).max() < 1e-6
        assert np.abs(prior["means"] - mean).max() < 1e-5
        assert np.abs(np.exp(prior["logvars"].astype(np.float64)) - var).max() < 1e-5 * var.max()


def test_skipped_rows_dead_components_and_the_floor():
    rng = np.random.default_rng(3)
    mu, lv, _ = P.clusters(rng, 50, 4, 2, 3.0)
    prior = P.start(rng, mu, lv, 2)
    bad_mu, bad_lv = np.vstack([mu, mu[:2]]), np.vstack([lv, lv[:2]])
    bad_mu[50, 1], bad_lv[51, 3] = np.nan, np.inf
    for step in (P.step64, P.step32):
        a, ba, na = step(mu, lv, prior)
        b, bb, nb = step(bad_mu, bad_lv, prior)
        assert na == nb == 50 and ba == bb and all(np.array_equal(a[k], b[k]) for k in a)
        none, bn, nn = step(bad_mu[50:], bad_lv[50:], prior)
        assert nn == 0 and np.isnan(bn) and all(np.array_equal(none[k], prior[k]) for k in prior)
        far = {k: v.copy() for k, v in prior.items()}
        far["means"][1] = 1e4
        out, bf, _ = step(mu, lv, far)
        assert np.isfinite(bf) and out["weights"][1] == 0 and np.array_equal(out["means"][1], far["means"][1])
        assert np.array_equal(out["logvars"][1], far["logvars"][1]) and all(np.isfinite(v).all() for v in out.values())
        x = np.eye(3, 4, dtype=np.float32)
        own = {"weights": np.full(3, 1 / 3, np.float32), "means": x.copy(), "logvars": np.full((3, 4), -8.0, np.float32)}
        out, _, _ = step(x, None, own, 1e-3)
        assert np.allclose(out["logvars"], np.log(1e-3), atol=1e-6) and np.array_equal(out["means"], x)
    ll, r = P.estep64(bad_mu, bad_lv, prior)
    assert np.isnan(ll[50:]).all() and np.isnan(r[50:]).all() and np.isfinite(ll[:50]).all()


def test_float32_restatement_is_close_to_the_definition():
    """the figures the GPU bounds are multiples of, and the 30-iteration deviation: the runs do not fork"""
    for nz, K, N in ((7, 3, 300), (20, 10, 2000)):
        rng = np.random.default_rng(300 + nz)
        mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
        init = P.start(rng, mu, lv, K)
        ref, b64, _ = P.fit64(mu, lv, init, 30)
        own, b32 = P.fit32(mu, lv, init, 30)
        ew, em, es, eb = P.prior_errs(own, ref, b32, b64, nz)
        print("n_z=%d K=%d N=%d: float32 restatement after 30 iterations: weights %.2e means %.2e logvars %.2e bound %.2e"
              % (nz, K, N, ew, em, es, eb))
        assert ew < 1e-4 and em < 1e-4 and es < 1e-3 and eb < 1e-4


# ------------------------------------------------------------------------------------------------ avae_gmm_plan
def _config(capi, n_z=20):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = 2
    for m, (n_in, h) in enumerate(((784, 96), (147, 72))):
        cfg.mod[m].n_input = n_in
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = h
        cfg.mod[m].n_hidden[1] = h
        cfg.mod[m].binary = 1 - m
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = n_z, 16, 1, 0
    cfg.learning_rate, cfg.assoc_lambda = 1e-3, 1.0
    return cfg


def _plan(capi, rows, K, n_z=20):
    L = capi.lib()
    sl, ns, sb = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    assert L.avae_gmm_plan(C.byref(_config(capi, n_z)), rows, K, C.byref(sl), C.byref(ns), C.byref(sb)) == 0
    return sl.value, ns.value, sb.value


def test_plan_is_a_function_of_rows_alone_with_no_empty_slice(capi):
    MAX = 256 * (2 + 64 + 2 * 64 * 64) * 8 + 2 * (64 + 2 * 64 * 64) * 4
    assert MAX == 16978432
    for rows in (0, 1, 19, 64, 65, 101, 129, 255, 256, 257, 4096, 16384, 16385, 20000, 65536, 65537, 1048576, 2 ** 31 - 1):
        plans = {(K, nz): _plan(capi, rows, K, nz) for K in (1, 10, 64) for nz in (7, 20, 64)}
        assert len({p[:2] for p in plans.values()}) == 1, "the partition does not depend on K or n_z"
        slice_rows, n_slices, _ = plans[1, 7]
        assert slice_rows % 64 == 0 and slice_rows >= 64 and n_slices <= 256
        if rows == 0:
            assert n_slices == 0
        else:
            assert (n_slices - 1) * slice_rows < rows <= n_slices * slice_rows, "every row covered, no slice empty"
        for (K, nz), (_, _, scratch) in plans.items():
            assert scratch == n_slices * (2 + K + 2 * K * nz) * 8 + 2 * (K + 2 * K * nz) * 4 <= MAX
    assert _plan(capi, 101, 10)[:2] == (64, 2) and _plan(capi, 129, 10)[:2] == (64, 3) and _plan(capi, 4096, 10)[:2] == (64, 64)
    assert _plan(capi, 20000, 10)[:2] == (128, 157) and _plan(capi, 65536, 10)[:2] == (256, 256)
    assert _plan(capi, 1048576, 10)[:2] == (4096, 256)


def test_plan_errors_carry_a_message(capi):
    L = capi.lib()
    for rows, K, needle in ((-1, 10, "rows must be >= 0"), (10, 0, "n_components = 0 must be in [1, 64]"),
                            (10, 65, "n_components = 65 must be in [1, 64]")):
        assert L.avae_gmm_plan(C.byref(_config(capi)), rows, K, None, None, None) != 0
        msg = L.avae_last_error(None).decode()
        assert "avae_gmm_plan" in msg and needle in msg, msg
    assert L.avae_gmm_plan(None, 10, 10, None, None, None) != 0
    assert L.avae_gmm_plan(C.byref(_config(capi)), 10, 10, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ the Python helpers
def _args(V, post, K=3, T=5, init=None, seed=0, vf=1e-6, nz=4):
    return V.latent_prior_args(post, K, T, init, seed, vf, nz, "cpu")


def test_argument_shapes_and_bounds(V):
    rng = np.random.default_rng(5)
    mu, lv = rng.standard_normal((9, 4)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    m, l, K, T, vf, init, rows, was_np = _args(V, (mu, lv))
    assert was_np and K == 3 and T == 5 and vf == 1e-6 and init is None and m.shape == (9, 4) and l.shape == (9, 4)
    assert m.dtype == torch.float32 and m.is_contiguous() and rows.shape == (3,) and rows.dtype == torch.int64
    assert _args(V, (mu, None))[1] is None
    assert _args(V, (torch.from_numpy(mu), torch.from_numpy(lv)))[7] is False
    assert _args(V, (mu.astype(np.float64), lv))[0].dtype == torch.float32
    for bad, needle in (((mu[:, :3], lv[:, :3]), "[rows, 4]"), ((mu, lv[:8]), "logvar must be [9"), (mu, "pair"), ((mu, lv, lv), "pair"),
                        ([], "pair"), ([(mu, lv), (mu, None)], "every pair"), (None, "pair")):
        with pytest.raises(ValueError, match=needle.replace("[", r"\[")):
            _args(V, bad)
    for kw, needle in ((dict(K=0), "n_components"), (dict(K=65), "n_components"), (dict(K=2.0), "n_components"), (dict(K=True), "n_components"),
                       (dict(T=-1), "n_iters"), (dict(T=1.5), "n_iters"), (dict(vf=0.0), "var_floor"), (dict(vf=float("inf")), "var_floor"),
                       (dict(vf=-1.0), "var_floor"), (dict(vf=1e-60), "var_floor"), (dict(vf="x"), "var_floor"), (dict(seed=-1), "seed"),
                       (dict(seed=1.5), "seed"), (dict(K=10), "more than the 9 rows")):
        with pytest.raises(ValueError, match=needle):
            _args(V, (mu, lv), **kw)
    assert _args(V, (mu, lv), K=9)[6].shape == (9,) and _args(V, (mu, lv), T=0)[3] == 0


def test_a_list_of_pairs_is_the_concatenation(V):
    rng = np.random.default_rng(6)
    a, b = (rng.standard_normal((5, 4)).astype(np.float32) for _ in range(2))
    c, d = (rng.standard_normal((7, 4)).astype(np.float32) for _ in range(2))
    m, l = _args(V, [(a, b), (c, d)])[:2]
    assert np.array_equal(m.numpy(), np.vstack([a, c])) and np.array_equal(l.numpy(), np.vstack([b, d]))
    one = _args(V, (np.vstack([a, c]), np.vstack([b, d])))
    assert torch.equal(one[6], _args(V, [(a, b), (c, d)])[6])
    m, l = _args(V, [(a, None), (c, None)])[:2]
    assert l is None and m.shape == (12, 4)
    with pytest.raises(ValueError, match=r"posteriors\[1\]"):
        _args(V, [(a, b), (c, d[:, :3])])


def test_init_dict_validation(V):
    rng = np.random.default_rng(7)
    mu, lv = rng.standard_normal((9, 4)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    good = dict(weights=np.full(3, 1 / 3), means=mu[:3], logvars=np.zeros((3, 4)))
    w, m, s = _args(V, (mu, lv), init=good)[5]
    assert _args(V, (mu, lv), init=good)[6] is None
    assert w.dtype == m.dtype == s.dtype == torch.float32 and w.shape == (3,) and m.shape == (3, 4) and s.shape == (3, 4)
    m[0, 0] = 99.0
    assert mu[0, 0] != 99.0, "the fit works on copies"
    for change, needle in ((dict(weights=np.full(2, 0.5)), r"weights must be \[3\]"), (dict(means=mu[:2]), "means must be"),
                           (dict(logvars=np.zeros((3, 5))), "4"), (dict(weights=np.array([0.5, np.nan, 0.5])), "finite"),
                           (dict(weights=np.array([0.5, -0.1, 0.6])), "non-negative"), (dict(weights=np.zeros(3)), "not all zero"),
                           (dict(weights=np.full((3, 1), 1 / 3)), r"weights must be \[K\]"), (dict(means=None), "means is None")):
        with pytest.raises(ValueError, match=needle):
            _args(V, (mu, lv), init=dict(good, **change))
    for bad in ({"weights": good["weights"]}, [1, 2, 3], "kmeans"):
        with pytest.raises(ValueError, match="weights, means and logvars"):
            _args(V, (mu, lv), init=bad)
    with pytest.raises(ValueError, match="K <= 64"):
        V.prior_arrays(dict(weights=np.full(65, 1 / 65), means=np.zeros((65, 4)), logvars=np.zeros((65, 4))), 4, "cpu")


def test_seeded_init_is_reproducible_and_uses_finite_rows_only(V):
    rng = np.random.default_rng(8)
    mu, lv = rng.standard_normal((40, 4)).astype(np.float32), rng.standard_normal((40, 4)).astype(np.float32)
    mu[[3, 17], 1] = np.nan
    lv[[5, 17, 30], 2] = [np.inf, 0.0, -np.inf]
    finite = np.array([r for r in range(40) if r not in (3, 5, 17, 30)])
    for seed in (0, 1, 12345):
        rows = _args(V, (mu, lv), K=36, seed=seed)[6].numpy()
        assert np.array_equal(rows, _args(V, (mu, lv), K=36, seed=seed)[6].numpy())
        assert np.array_equal(rows, finite[np.random.default_rng(seed).permutation(36)[:36]])
        assert sorted(rows) == sorted(finite)
        assert np.array_equal(_args(V, (mu, lv), K=5, seed=seed)[6].numpy(), rows[:5])
    assert not np.array_equal(_args(V, (mu, lv), K=5, seed=0)[6].numpy(), _args(V, (mu, lv), K=5, seed=1)[6].numpy())
    with pytest.raises(ValueError, match="more than the 36 rows"):
        _args(V, (mu, lv), K=37)
    assert sorted(_args(V, (mu, None), K=38)[6].numpy()) == [r for r in range(40) if r not in (3, 17)]


def test_score_arguments(V):
    rng = np.random.default_rng(9)
    z, lv = rng.standard_normal((6, 4)).astype(np.float32), rng.standard_normal((6, 4)).astype(np.float32)
    prior = dict(weights=np.full(2, 0.5), means=z[:2], logvars=np.zeros((2, 4)), bound=np.zeros(3), n_used=6)
    mu, l, w, m, s, was_np = V.latent_score_args(z, prior, 4, "cpu")
    assert was_np and l is None and mu.shape == (6, 4) and w.shape == (2,) and m.shape == (2, 4) and s.shape == (2, 4)
    mu, l, _, _, _, was_np = V.latent_score_args((torch.from_numpy(z), torch.from_numpy(lv)), prior, 4, "cpu")
    assert not was_np and l.shape == (6, 4)
    for bad_z, needle in ((None, "z is None"), (z[:, :3], "z: "), ((z, lv[:5]), "z: logvar")):
        with pytest.raises(ValueError, match=needle):
            V.latent_score_args(bad_z, prior, 4, "cpu")
    with pytest.raises(ValueError, match="prior"):
        V.latent_score_args(z, dict(weights=prior["weights"]), 4, "cpu")
