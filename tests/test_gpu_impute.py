"""impute / avae_impute on a real MI355X (include/avae.h) against tests/impute_reference.py: the fused
posterior, the bitwise ties with transform / generate, sampled mean and variance within 4x the definition's own float32 rounding
on the same inputs, absent entries that change no bit, the shared draw counter, determinism, no side effects on training, the
decode routes, edges and errors.  batch_size = 16 everywhere: N in {1, 15, 19} and K in {5, 16, 40} cross several rows per pass,
one row per pass, one row over three passes (16 + 16 + 8), a partial last pass and a partial last chunk.  The default route keeps
up to 16 passes (256 decoded rows here) between one sampling and one accumulate launch, so K = 40 carries the running (mean, M2)
across launches on the modality-by-modality route (use_graph=0, compared bitwise with the default route) and K = 300 = 256 + 44
carries it on the default route."""
import ctypes as C

import numpy as np
import pytest
import torch

import impute_reference as R
from conftest import shadow_err, synth_batch
from test_impute_cpu import SAMPLED

pytestmark = pytest.mark.gpu

B = 16


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _pair(V, nz, three, dtype, archs=None, **kw):
    """HIP model + oracle on the same weights: relu for fp32, softplus for bf16 (quant='bf16' oracle), as tests/test_gpu_score.py"""
    archs = R.archs_for(nz, three) if archs is None else archs
    fp32 = dtype == "fp32"
    act = "relu" if fp32 else "softplus"
    model = V.AssocVariationalAutoEncoder(archs, transfer_fct=act, learning_rate=1e-3, batch_size=B, compute_dtype=dtype, seed=5,
                                          **dict(R.model_kw(three), **kw))
    flat = R.init_flat(archs, 5)
    model.set_params(flat)
    return model, R.oracle_for(archs, three, act, B, flat, None if fp32 else "bf16")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_same(a, b, what=""):
    for key in ("mu", "logvar"):
        assert _same_bits(a[key], b[key]), what + key
    for key in ("mean", "var"):
        assert (a[key] is None) == (b[key] is None), what + key
        for d in range(len(a[key] or ())):
            assert _same_bits(a[key][d], b[key][d]), "%s%s[%d]" % (what, key, d)


def _lat_tol(dtype, r):
    return (1e-5 if dtype == "fp32" else 2e-3) * max(1.0, float(np.abs(r).max()))       # mu / lv


def _garbage(X, p, rng):
    """X with NaN / Inf / 1e30 in every absent entry"""
    out = []
    for m, x in enumerate(X):
        junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), size=x.shape)
        out.append(np.where(p[:, m:m + 1], x, junk).astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------ 1. fusion
@pytest.mark.parametrize("nz", [20, 7, 64])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fusion(V, nz, dtype):
    """Every presence pattern of three modalities, the empty one included, in 19 rows (a full chunk and a partial one)."""
    model, ref = _pair(V, nz, True, dtype)
    archs, X, p, _ = R.case(nz, True, 19, 0, seed=nz)
    assert len({tuple(r) for r in p.tolist()}) == 8
    got = model.impute(X, p)
    want = R.ref_impute(ref, X, p)
    assert got["var"] is None and got["mu"].shape == (19, nz) and got["logvar"].shape == (19, nz)
    assert [m.shape for m in got["mean"]] == [(19, 784), (19, 147), (19, 50)]
    for key in ("mu", "logvar"):
        err, tol = np.abs(got[key] - want[key]).max(), _lat_tol(dtype, want[key])
        print("nz=%d %s %s: max err %.3e, tol %.3e" % (nz, dtype, key, err, tol))
        assert err <= tol, key
    for m in range(3):
        only = p[:, m] & (p.sum(1) == 1)
        assert only.any()
        mu, lv = model._encode(m, X[m], want_logvar=True)
        assert np.array_equal(_bits(got["mu"])[only], _bits(mu)[only]) and np.array_equal(_bits(got["logvar"])[only], _bits(lv)[only])
    none = ~p.any(1)
    assert none.any() and not _bits(got["mu"])[none].any() and not _bits(got["logvar"])[none].any()      # +0.0 exactly
    # nothing given at all: every row is the prior predictive
    prior = model.impute([None, None, None], np.ones((5, 3), bool))
    assert not _bits(prior["mu"]).any() and not _bits(prior["logvar"]).any()
    gen = model.generate(np.zeros((5, nz), np.float32))
    for d in range(3):
        assert _same_bits(prior["mean"][d], gen[d]), d
    # present=None: every given modality on every row
    a, b = model.impute([X[0], None, X[2]]), model.impute(X, np.tile(np.array([[1, 0, 1]], bool), (19, 1)))
    _assert_same(a, b, "present=None ")


# ------------------------------------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("nz,three", [(20, False), (7, True), (64, False)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ties_to_the_existing_surface(V, nz, three, dtype):
    model, ref = _pair(V, nz, three, dtype)
    archs, X, p, _ = R.case(nz, three, 19, 0, seed=1)
    r0 = model.impute(X, p)
    gen = model.generate(r0["mu"])
    for d in range(len(archs)):
        assert _same_bits(r0["mean"][d], gen[d]), d                                     # n_samples = 0 is generate(mu)
    r3 = model.impute(X, p, n_samples=3, eps=np.zeros((19, 3, nz), np.float32))
    r1 = model.impute(X, p, n_samples=1, eps=np.random.default_rng(0).standard_normal((19, 1, nz)).astype(np.float32))
    assert _same_bits(r3["mu"], r0["mu"]) and _same_bits(r3["logvar"], r0["logvar"]) and _same_bits(r1["mu"], r0["mu"])
    for d in range(len(archs)):
        assert _same_bits(r3["mean"][d], r0["mean"][d]), d                              # Welford on equal values is exact
        assert np.all(r3["var"][d] == 0) and np.all(r1["var"][d] == 0), d


# ------------------------------------------------------------------------------------------------ 3. sampled mean and variance
@pytest.mark.parametrize("nz,three,N,K", SAMPLED)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampled_mean_and_variance(V, nz, three, N, K, dtype):
    """Against the definition with the caller's eps.  The bound is not invented: the definition in float32 arithmetic is compared
    with itself in fp64 on these very inputs (impute_reference.rounding_spread), and the kernels may deviate from fp64 by 4x that,
    relative to max |mean| and max var of the modality; mu / logvar at DESIGN.md section 2's tolerances."""
    model, ref = _pair(V, nz, three, dtype)
    archs, X, p, eps = R.case(nz, three, N, K, seed=100 + K)
    want, dev, lat = R.rounding_spread(ref, X, p, K, eps)
    got = model.impute(X, p, n_samples=K, eps=eps)
    for key in ("mu", "logvar"):
        assert np.abs(got[key] - want[key]).max() <= _lat_tol(dtype, want[key]), key
    fails = []
    for d in range(len(archs)):
        sm, sv = np.abs(want["mean"][d]).max(), want["var"][d].max()
        em, ev = np.abs(got["mean"][d] - want["mean"][d]).max() / sm, np.abs(got["var"][d] - want["var"][d]).max() / sv
        print("nz=%d M=%d N=%d K=%d %s modality %d: mean err %.3e (float32 definition %.3e), var err %.3e (float32 definition %.3e)"
              % (nz, len(archs), N, K, dtype, d, em, dev[d][0], ev, dev[d][1]))
        assert got["mean"][d].shape == (N, archs[d]["n_input"]) and np.all(got["var"][d] >= 0)
        if em > 4 * dev[d][0] or ev > 4 * dev[d][1]:
            fails.append((d, em, dev[d][0], ev, dev[d][1]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 4. never read, 6. determinism
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_absent_entries_are_never_read_and_calls_are_deterministic(V, dtype):
    model, ref = _pair(V, 7, True, dtype)
    rng = np.random.default_rng(9)
    for N, K in ((19, 0), (19, 5), (3, 40)):
        archs, X, p, eps = R.case(7, True, N, K, seed=K)
        clean = model.impute(X, p, n_samples=K, eps=eps)
        _assert_same(model.impute(X, p, n_samples=K, eps=eps), clean, "again ")
        _assert_same(model.impute(_garbage(X, p, rng), torch.from_numpy(p).to(model.device), n_samples=K, eps=eps), clean, "garbage ")
        p1 = p.copy()
        p1[:, 1] = False
        a = model.impute(_garbage(X, p1, rng), p1, n_samples=K, eps=eps)
        b = model.impute([X[0], None, X[2]], p, n_samples=K, eps=eps)       # (p's own column 1 is overruled by the None)
        _assert_same(a, b, "None ")
        for v in clean["mean"] + (clean["var"] or []) + [clean["mu"], clean["logvar"]]:
            assert np.all(np.isfinite(v))


# ------------------------------------------------------------------------------------------------ 5. internal generator
def test_internal_noise_shares_the_scoring_calls_draw_counter(V):
    archs, X, p, _ = R.case(20, False, 7, 0, seed=2)
    Xl = [np.concatenate([x, x[:5] + 1]) for x in X]
    pl = np.concatenate([p, p[:5]])
    a, _ = _pair(V, 20, False, "fp32")
    b, _ = _pair(V, 20, False, "fp32")
    a1, a2 = a.impute(X, p, n_samples=5), a.impute(X, p, n_samples=5)                    # draws 1, 2
    assert _same_bits(a1["mu"], a2["mu"]) and _same_bits(a1["logvar"], a2["logvar"])
    for d in range(2):
        assert np.all(np.any(a1["mean"][d] != a2["mean"][d], axis=1)), d                   # every row: a fresh draw
    b1 = b.impute(Xl, pl, n_samples=5)                                                   # draw 1, in a longer input
    for d in range(2):                                                                   # the key is the row of the whole input
        assert _same_bits(b1["mean"][d][:7], a1["mean"][d]) and _same_bits(b1["var"][d][:7], a1["var"][d]), d
    b.impute(X, p)                                                                       # n_samples = 0 draws nothing
    b.score_samples(X)                                                                   # draw 2
    b3 = b.impute(X, p, n_samples=5)                                                     # draw 3
    a3 = a.impute(X, p, n_samples=5)                                                     # draw 3
    _assert_same(a3, b3, "draw 3 ")
    assert not _same_bits(b3["mean"][1], a2["mean"][1])


# ------------------------------------------------------------------------------------------------ 7. state untouched
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_impute_has_no_side_effects_on_training(V, dtype):
    rng = np.random.default_rng(21)
    Xt = synth_batch(rng, 2 * B, [784, 147], [True, False])
    et = rng.standard_normal((2 * B, 20)).astype(np.float32)
    archs, X, p, eps = R.case(20, False, 19, 40, seed=4)
    state = lambda m: m.get_opt_state() + (m.get_params(), m.cost_history(1))
    runs = []
    for with_calls in (False, True):
        model, _ = _pair(V, 20, False, dtype)
        model.partial_fit([x[:B] for x in Xt], et[:B])
        before = state(model)
        if with_calls:
            model.impute(X, p)
            model.impute(X, p, n_samples=5)
            model.impute([X[0], None], n_samples=40, eps=eps)
            model.synchronize()
            for x, y in zip(before, state(model)):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        cost = model.partial_fit([x[B:] for x in Xt], et[B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append((np.float32(cost), model.get_grads()) + state(model))
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ------------------------------------------------------------------------------------------------ 8. routes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_modality_by_modality_route_and_replica_give_the_same_bits(V, dtype):
    archs, X, p, eps = R.case(7, True, 19, 5, seed=6)
    plain, _ = _pair(V, 7, True, dtype)
    eager, _ = _pair(V, 7, True, dtype, use_graph=0)
    rank, _ = _pair(V, 7, True, dtype, comm="ipc")
    for K, e in ((0, None), (5, eps), (40, np.random.default_rng(3).standard_normal((19, 40, 7)).astype(np.float32))):
        want = plain.impute(X, p, n_samples=K, eps=e)
        _assert_same(eager.impute(X, p, n_samples=K, eps=e), want, "use_graph=0 K=%d " % K)
        _assert_same(rank.impute(X, p, n_samples=K, eps=e), want, "ipc replica K=%d " % K)


def test_conv_modality(V):
    """fp32 conv + MLP (test_gpu_dataparallel's ARCHS_CONV), K = 3, at test_gpu_parity.test_conv_deconv_branch's tolerances:
    2e-5 on decoder outputs, 5x that on the posterior."""
    from test_gpu_dataparallel import ARCHS_CONV
    model, ref = _pair(V, 20, False, "fp32", archs=ARCHS_CONV)
    rng = np.random.default_rng(12)
    N, K = 19, 3
    X = synth_batch(rng, N, [784, 147], [True, False])
    p = R.pattern_rows(N, 2, shift=1)
    eps = rng.standard_normal((N, K, 20)).astype(np.float32)
    tol = 2e-5
    for k, e in ((0, None), (K, eps)):
        got, want = model.impute(X, p, n_samples=k, eps=e), R.ref_impute(ref, X, p, k, e)
        for key in ("mu", "logvar"):
            assert np.abs(got[key] - want[key]).max() <= 5 * tol * max(1.0, np.abs(want[key]).max()), key
        for d in range(2):
            em = np.abs(got["mean"][d] - want["mean"][d]).max()
            print("conv K=%d modality %d: mean err %.3e" % (k, d, em))
            assert em <= tol * max(1.0, np.abs(want["mean"][d]).max()), d
            if k:
                ev = np.abs(got["var"][d] - want["var"][d]).max()
                print("conv K=%d modality %d: var err %.3e" % (k, d, ev))
                assert ev <= tol * max(1.0, want["var"][d].max()), d


# ------------------------------------------------------------------------------------------------ 9. edges and errors
def test_edges_and_errors(V):
    model, ref = _pair(V, 20, False, "fp32")
    archs, X, p, eps = R.case(20, False, 9, 4, seed=8)
    empty = model.impute([x[:0] for x in X], n_samples=2)
    assert empty["mu"].shape == (0, 20) and empty["mean"][1].shape == (0, 147) and empty["var"][0].shape == (0, 784)
    dev = model.impute([torch.from_numpy(x).to(model.device) for x in X], torch.from_numpy(p), n_samples=4,
                       eps=torch.from_numpy(eps))
    assert torch.is_tensor(dev["mu"]) and dev["mu"].is_cuda and torch.is_tensor(dev["var"][1]) and dev["mean"][0].is_cuda
    full = model.impute(X, p, n_samples=4, eps=eps)
    _assert_same({k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in dev.items()}, full)
    with pytest.raises(ValueError, match="n_samples"):
        model.impute(X, p, n_samples=-1)
    with pytest.raises(ValueError):
        model.impute(X, p, n_samples=4, eps=np.zeros((9, 20), np.float32))
    with pytest.raises(ValueError):
        model.impute(X, p, n_samples=4, eps=np.zeros((9, 3, 20), np.float32))
    with pytest.raises(ValueError):
        model.impute(X, np.ones((9, 3), bool))
    with pytest.raises(ValueError):
        model.impute([X[0], X[1][:8]], p)
    with pytest.raises(ValueError):
        model.impute([None, None])
    # the C ABI: optional outputs, zero rows, n_samples < 0
    L = model._L
    ts = [torch.from_numpy(x).to(model.device) for x in X]
    pd = torch.from_numpy(p.astype(np.uint8)).to(model.device)
    ed = torch.from_numpy(eps).to(model.device)
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    lds = (C.c_int32 * 2)(784, 147)
    mean1 = torch.full((9, 147), -7.0, dtype=torch.float32, device=model.device)
    var0 = torch.full((9, 784), -7.0, dtype=torch.float32, device=model.device)
    lv = torch.full((9, 20), -7.0, dtype=torch.float32, device=model.device)
    mp, vp = (C.c_void_p * 2)(None, mean1.data_ptr()), (C.c_void_p * 2)(var0.data_ptr(), None)
    assert L.avae_impute(model._h, ptrs, lds, pd.data_ptr(), 9, 4, ed.data_ptr(), None, lv.data_ptr(), mp, vp, None) == 0
    torch.cuda.synchronize()
    assert _same_bits(mean1.cpu().numpy(), full["mean"][1]) and _same_bits(var0.cpu().numpy(), full["var"][0])
    assert _same_bits(lv.cpu().numpy(), full["logvar"])
    mean1.fill_(-7.0)
    var_before = var0.clone()
    assert L.avae_impute(model._h, ptrs, None, pd.data_ptr(), 9, 0, None, None, None, mp, vp, None) == 0      # var_dev ignored
    mu = torch.full((9, 20), -7.0, dtype=torch.float32, device=model.device)
    assert L.avae_impute(model._h, ptrs, lds, None, 9, 4, None, mu.data_ptr(), None, None, None, None) == 0    # no decoder output
    torch.cuda.synchronize()
    assert _same_bits(mean1.cpu().numpy(), model.impute(X, p)["mean"][1]) and torch.equal(var0, var_before)
    assert _same_bits(mu.cpu().numpy(), model.impute(X)["mu"])
    assert L.avae_impute(model._h, ptrs, lds, pd.data_ptr(), 0, 4, None, None, None, None, None, None) == 0    # zero rows: a no-op
    assert L.avae_impute(model._h, ptrs, lds, pd.data_ptr(), 9, -1, None, None, None, mp, vp, None) != 0
    assert b"n_samples" in L.avae_last_error(model._h)
    assert L.avae_impute(model._h, ptrs, lds, pd.data_ptr(), -1, 0, None, None, None, mp, vp, None) != 0
    assert b"rows" in L.avae_last_error(model._h)
    assert L.avae_impute(model._h, None, lds, pd.data_ptr(), 9, 0, None, None, None, mp, vp, None) != 0
    assert b"x_dev" in L.avae_last_error(model._h)
    torch.cuda.synchronize()
    _assert_same(model.impute(X, p, n_samples=4, eps=eps), full, "after errors ")        # the handle still works
