"""The 2-D map of the posteriors checked without a GPU: the definitions of tests/embed_reference.py against their own properties
(sum p = 1, the analytic gradient against central differences, the realised perplexity, a falling KL, cluster purity), the float32
restatement's own error, avae_embed_plan (host-only: a function of rows alone, no empty split, the splits cover the rows, the
65,536-row rule) and the argument handling of embed_args.  No model is constructed here."""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_reference as E
import latent_prior_reference as P

CASES = [(300, 7, 3, 20.0), (600, 20, 6, 30.0)]       # N, n_z, clusters, perplexity


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


_DATA = {}


def _case(i, metric):
    if (i, metric) not in _DATA:
        N, nz, K, perp = CASES[i]
        mu, lv, label = P.clusters(np.random.default_rng(100 + i), N, nz, K, 3.0)
        D, ok = E.distances64(mu, lv, metric)
        beta, shift, norm, tries = E.calibrate(D, ok, perp)
        _DATA[i, metric] = (mu, lv, label, D, ok, beta, shift, norm, tries, E.affinities(D, ok, beta, shift, norm))
    return _DATA[i, metric]


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("metric", [E.SYMKL, E.L2])
@pytest.mark.parametrize("i", [0, 1])
def test_calibration_reaches_the_perplexity_and_p_sums_to_one(i, metric):
    perp = CASES[i][3]
    mu, lv, _, D, ok, beta, shift, norm, tries, Pm = _case(i, metric)
    assert ok.all() and (beta > 0).all() and (tries >= 1).all()
    H, s0 = E.entropy(D, ok, beta, shift)
    print("N=%d %s: at most %d tries, |H - log perplexity| <= %.2e" % (len(beta), metric, tries.max(), np.abs(H - np.log(perp)).max()))
    assert np.abs(H - np.log(perp)).max() <= 1e-5 and tries.max() < 64
    assert np.array_equal(s0, norm) and (norm >= 1.0).all(), "the minimum's own term is exp(0)"
    assert abs(Pm.sum() - 1.0) <= 1e-12 and np.array_equal(Pm, Pm.T) and (np.diag(Pm) == 0).all()
    assert np.array_equal(D, D.T) and (D - shift[:, None] >= 0)[E.pair_mask(ok)].all()


def test_analytic_gradient_equals_central_differences():
    mu, lv, _, D, ok, beta, shift, norm, _, Pm = _case(0, E.SYMKL)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((len(beta), 2))
    g, kl = E.gradient(Pm, Y, ok)
    assert abs(kl - E.kl_of(Pm, Y, ok)) == 0
    worst, h = 0.0, 1e-5
    for n, c in [(0, 0), (7, 1), (123, 0), (299, 1), (150, 1)]:
        up, dn = Y.copy(), Y.copy()
        up[n, c] += h
        dn[n, c] -= h
        num = (E.kl_of(Pm, up, ok) - E.kl_of(Pm, dn, ok)) / (2 * h)
        worst = max(worst, abs(num - g[n, c]) / np.abs(g).max())
    print("gradient against central differences: %.2e of max |grad|" % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("i", [0, 1])
def test_three_hundred_iterations_lower_the_kl_and_keep_the_clusters_apart(i):
    N, nz, K, perp = CASES[i]
    mu, lv, label, D, ok, beta, shift, norm, _, Pm = _case(i, E.SYMKL)
    y0 = np.random.default_rng(0).normal(0.0, 1e-4, (N, 2)).astype(np.float32)
    y, vel, gain, kl, _ = E.iterate(Pm, ok, y0, np.zeros_like(y0), np.ones_like(y0), 0, 300, max(N / 48.0, 50.0),
                                    exaggeration_iters=100)
    print("N=%d n_z=%d: KL %.3f -> %.3f, purity %.3f" % (N, nz, kl[0], kl[-1], E.purity(y, label)))
    assert np.isfinite(y).all() and kl[-1] < kl[0] and E.purity(y, label) == 1.0
    assert np.abs(y.astype(np.float64).mean(axis=0)).max() <= 1e-5 * np.abs(y).max(), "centred"
    # 120 + 180 continued from the state: the bits of 300 run without centring
    a = E.iterate(Pm, ok, y0, np.zeros_like(y0), np.ones_like(y0), 0, 120, max(N / 48.0, 50.0), exaggeration_iters=100, center=False)
    b = E.iterate(Pm, ok, a[0], a[1], a[2], 120, 180, max(N / 48.0, 50.0), exaggeration_iters=100, center=False)
    whole = E.iterate(Pm, ok, y0, np.zeros_like(y0), np.ones_like(y0), 0, 300, max(N / 48.0, 50.0), exaggeration_iters=100, center=False)
    assert all(np.array_equal(b[k], whole[k]) for k in range(3)) and np.array_equal(np.concatenate([a[3][:-1], b[3]]), whole[3])


def test_skipped_rows_change_no_other_row():
    mu, lv, _ = P.clusters(np.random.default_rng(9), 40, 5, 2, 3.0)
    bm, bl = np.vstack([mu, mu[:3]]), np.vstack([lv, lv[:3]])
    bm[40, 1], bl[41, 0], bm[42, 4] = np.nan, np.inf, -np.inf
    for dtype, dist in ((np.float64, E.distances64), (np.float32, E.distances32)):
        D, ok = dist(mu, lv, E.SYMKL)
        Db, okb = dist(bm, bl, E.SYMKL)
        assert okb.sum() == 40 and not okb[40:].any()
        ca, cb = E.calibrate(D, ok, 10.0, dtype=dtype), E.calibrate(Db, okb, 10.0, dtype=dtype)
        assert all(np.array_equal(x, y[:40]) for x, y in zip(ca, cb)) and np.isnan(cb[0][40:]).all() and (cb[3][40:] == 0).all()
        Pa, Pb = E.affinities(D, ok, *ca[:3], dtype=dtype), E.affinities(Db, okb, *cb[:3], dtype=dtype)
        assert np.array_equal(Pa, Pb[:40, :40]) and (Pb[40:] == 0).all() and (Pb[:, 40:] == 0).all()
        rng = np.random.default_rng(1)
        y = rng.standard_normal((43, 2)).astype(np.float32)
        one = np.ones((43, 2), np.float32)
        ra = E.iterate(Pa, ok, y[:40], 0 * one[:40], one[:40], 0, 3, 50.0, dtype=dtype)
        rb = E.iterate(Pb, okb, y, 0 * one, one, 0, 3, 50.0, dtype=dtype)
        assert all(np.array_equal(ra[k], rb[k][:40]) and np.isnan(rb[k][40:]).all() for k in range(3)) and np.array_equal(ra[3], rb[3])
    # L2 never reads the log-variances
    assert E.used_rows(bm, bl, E.L2).sum() == 41


def test_float32_restatement_is_close_to_the_definition():
    """the figures the GPU bounds are multiples of"""
    for i, metric in ((0, E.SYMKL), (1, E.L2)):
        N, nz, K, perp = CASES[i]
        mu, lv, _, D, ok, beta, shift, norm, tries, Pm = _case(i, metric)
        D32, _ = E.distances32(mu, lv, metric)
        b32, m32, s32, t32 = E.calibrate(D32, ok, perp, dtype=np.float32)
        H, _ = E.entropy(D, ok, b32, m32)
        print("N=%d %s: restatement beta %.2e relative, realised |H - log perplexity| %.2e, tries differ on %d rows"
              % (N, metric, np.abs(b32 / beta - 1).max(), np.abs(H - np.log(perp)).max(), (t32 != tries).sum()))
        assert np.abs(b32 / beta - 1).max() < 1e-3 and np.abs(H - np.log(perp)).max() <= 2e-5
        cal = [x.astype(np.float32) for x in (beta, shift, norm)]
        rng = np.random.default_rng(2)
        Y = rng.standard_normal((N, 2)).astype(np.float32)
        g64, kl64 = E.gradient(E.affinities(D, ok, *cal), Y, ok, 12.0)
        g32, kl32 = E.gradient(E.affinities(D32, ok, *cal, dtype=np.float32), Y, ok, 12.0, np.float32)
        print("    gradient %.2e of max |grad|, kl %.2e" % (E.rel_max(g32, g64), E.kl_err(kl32, kl64)))
        assert E.rel_max(g32, g64) < 1e-5 and E.kl_err(kl32, kl64) < 1e-5


# ------------------------------------------------------------------------------------------------ avae_embed_plan
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


def _plan(capi, rows, n_z=20):
    v = [C.c_int32(-1) for _ in range(3)]
    sb = C.c_size_t(0)
    assert capi.lib().avae_embed_plan(C.byref(_config(capi, n_z)), rows, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(sb)) == 0
    return v[0].value, v[1].value, v[2].value, sb.value


def test_plan_covers_the_rows_with_no_empty_split(capi):
    seen = set()
    for rows in list(range(0, 200)) + [64 * t + d for t in range(1, 1025) for d in (-1, 0, 1)]:
        if rows > 65536:
            continue
        tile, ns, per, scratch = _plan(capi, rows)
        assert tile == 64 and _plan(capi, rows, 64) == (tile, ns, per, scratch), "a function of rows alone"
        tiles = -(-rows // 64)
        if rows == 0:
            assert ns == 0
            continue
        assert ns >= 1 and (ns - 1) * per < tiles <= ns * per, "the splits cover the tiles, none is empty"
        assert tiles * ns <= 2048 and rows * ns <= 131072 and scratch == 66688 + 7 * rows * ns * 8 <= 7406720
        want = min(tiles, -(-1024 // tiles))
        assert per == -(-tiles // want), "about 1024 workgroups"
        seen.add(ns)
    assert set(range(1, 33)) <= seen, "small inputs are split too"
    assert _plan(capi, 300)[1:3] == (5, 1) and _plan(capi, 2048)[1:3] == (32, 1) and _plan(capi, 4097)[1:3] == (13, 5)
    assert _plan(capi, 16384)[1:3] == (4, 64) and _plan(capi, 65536)[1:3] == (1, 1024)


def test_plan_errors_carry_a_message(capi):
    L = capi.lib()
    for rows, needle in ((-1, "rows must be >= 0"), (65537, "rows = 65537 is more than 65536")):
        assert L.avae_embed_plan(C.byref(_config(capi)), rows, None, None, None, None) != 0
        msg = L.avae_last_error(None).decode()
        assert "avae_embed_plan" in msg and needle in msg, msg
    assert L.avae_embed_plan(None, 10, None, None, None, None) != 0
    assert L.avae_embed_plan(C.byref(_config(capi)), 65536, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ embed_args
def _args(V, post, perplexity=3.0, n_iters=10, metric="symkl", learning_rate="auto", early_exaggeration=12.0, exaggeration_iters=250,
          momentum=(0.5, 0.8), init=None, seed=0, state=None, nz=4):
    return V.embed_args(post, perplexity, n_iters, metric, learning_rate, early_exaggeration, exaggeration_iters, momentum, init,
                        seed, state, nz, "cpu")


def test_argument_shapes_defaults_and_bounds(V):
    rng = np.random.default_rng(5)
    mu, lv = rng.standard_normal((9, 4)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    a = _args(V, (mu, lv))
    assert a["was_numpy"] and a["rows"] == 9 and a["n_used"] == 9 and a["metric"] == 0 and a["it0"] == 0 and a["calibration"] is None
    assert a["learning_rate"] == 50.0 and a["mu"].dtype == torch.float32 and a["logvar"].shape == (9, 4)
    assert np.array_equal(a["y"].numpy(), np.random.default_rng(0).normal(0.0, 1e-4, (9, 2)).astype(np.float32))
    assert (a["vel"] == 0).all() and (a["gain"] == 1).all() and a["vel"].shape == (9, 2)
    assert _args(V, (mu, None), metric="l2")["logvar"] is None and _args(V, (mu, lv), metric="L2")["logvar"] is None
    assert _args(V, (torch.from_numpy(mu), torch.from_numpy(lv)))["was_numpy"] is False
    big = rng.standard_normal((4900, 4)).astype(np.float32)
    assert _args(V, (big, None), metric="l2")["learning_rate"] == 4900 / 48.0
    both = _args(V, [(mu, lv), (mu[:5], lv[:5])])
    assert both["rows"] == 14 and np.array_equal(both["mu"].numpy(), np.vstack([mu, mu[:5]]))
    init = rng.standard_normal((9, 2))
    given = _args(V, (mu, lv), init=init)["y"]
    assert given.dtype == torch.float32 and np.array_equal(given.numpy(), init.astype(np.float32))
    bad_mu = mu.copy()
    bad_mu[3, 1] = np.nan
    assert _args(V, (bad_mu, lv))["n_used"] == 8
    for kw, needle in ((dict(metric="cosine"), "metric"), (dict(n_iters=-1), "n_iters"), (dict(n_iters=1.5), "n_iters"),
                       (dict(perplexity=0.5), "perplexity"), (dict(perplexity=8.5), "perplexity"), (dict(perplexity="x"), "perplexity"),
                       (dict(perplexity=float("nan")), "perplexity"), (dict(learning_rate=0.0), "learning_rate"),
                       (dict(learning_rate="fast"), "learning_rate"), (dict(learning_rate=float("inf")), "learning_rate"),
                       (dict(early_exaggeration=0.0), "early_exaggeration"), (dict(exaggeration_iters=-1), "exaggeration_iters"),
                       (dict(momentum=0.5), "momentum"), (dict(momentum=(0.5, float("nan"))), r"momentum\[1\]"), (dict(seed=-1), "seed"),
                       (dict(init=init[:8]), "init"), (dict(init=np.zeros((9, 3))), "init")):
        with pytest.raises(ValueError, match=needle):
            _args(V, (mu, lv), **kw)
    assert _args(V, (mu, lv), perplexity=8.0)["perplexity"] == 8.0
    with pytest.raises(ValueError, match="perplexity"):
        _args(V, (bad_mu, lv), perplexity=8.0)                       # F - 1 = 7
    for bad, needle in (((mu[:, :3], lv[:, :3]), r"\[rows, 4\]"), ((mu, lv[:8]), "logvar must be"), (mu, "pair"), ([], "pair"),
                        ((mu, None), "logvar is None"), ([(mu, lv), (mu, None)], "logvar is None"), ((mu[:1], lv[:1]), "perplexity")):
        with pytest.raises(ValueError, match=needle):
            _args(V, bad)
    with pytest.raises(ValueError, match="more than the 65536"):
        _args(V, (np.zeros((65537, 4), np.float32), None), metric="l2")


def test_state_continues_a_run(V):
    rng = np.random.default_rng(6)
    mu, lv = rng.standard_normal((9, 4)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    state = {"embedding": rng.standard_normal((9, 2)).astype(np.float32), "velocity": rng.standard_normal((9, 2)).astype(np.float32),
             "gains": np.full((9, 2), 1.2, np.float32), "iteration": 40, "beta": np.full(9, 2.0, np.float32),
             "shift": np.full(9, 0.5, np.float32), "norm": np.full(9, 3.0, np.float32)}
    a = _args(V, (mu, lv), state=state)
    assert a["it0"] == 40 and np.array_equal(a["y"].numpy(), state["embedding"]) and np.array_equal(a["vel"].numpy(), state["velocity"])
    assert np.array_equal(a["gain"].numpy(), state["gains"]) and [tuple(c.shape) for c in a["calibration"]] == [(9,)] * 3
    assert np.array_equal(a["calibration"][0].numpy(), state["beta"])
    a["y"][0, 0] = 99.0
    assert state["embedding"][0, 0] != 99.0, "the run works on copies"
    other = rng.standard_normal((9, 2)).astype(np.float32)
    assert np.array_equal(_args(V, (mu, lv), state=state, init=other)["y"].numpy(), other)
    for change, needle in ((dict(velocity=state["velocity"][:8]), "state: velocity"), (dict(iteration=-1), "iteration"),
                           (dict(beta=state["beta"][:8]), "state: beta"), (dict(iteration=1.5), "iteration")):
        with pytest.raises(ValueError, match=needle):
            _args(V, (mu, lv), state=dict(state, **change))
    for bad in ({"embedding": state["embedding"]}, [1, 2], "resume"):
        with pytest.raises(ValueError, match="state must be the state dict"):
            _args(V, (mu, lv), state=bad)
