"""aggregate_log_density / avae_agg_logpdf and elbo_decomposition on a real MI355X (include/avae.h) against
tests/aggregate_reference.py.

1. arithmetic: joint and marginals of small galleries against the float64 definition, within 4x the float32 restatement's own
   worst error on the same inputs (error measures |err| / (|ref| + n_z) for the joint, |err| / (|ref| + 1) for a marginal);
2. several query tiles, gallery tiles, slices and chunks of launches, same bound on each case's own inputs;
3. determinism: a query's bits do not depend on the other queries, on repetition, on the stream or on which outputs are asked for;
4. exclusion; 5. edges and errors of the C ABI; 6. the Python surface and elbo_decomposition; 7. no side effects on training.

batch_size = 16, small MLPs, n_z in {7, 20, 64}; latents mu ~ N(0, 1), lv ~ U(-6, 1), seeded; the standard query set of a gallery
is 12 of 19 samples of gallery rows' own posteriors and 7 of 19 draws from N(0, 9)."""
import ctypes as C

import numpy as np
import pytest
import torch

import aggregate_reference as A
from conftest import make_arch, shadow_err, synth_batch

pytestmark = pytest.mark.gpu

B = 16
WIDTHS = (784, 147)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V, nz, fresh=False, **kw):
    """one fp32 relu model per n_z, shared by the tests that only look at latents"""
    if fresh or nz not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, nz), make_arch("joint", 147, 72, 40, nz)]
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          learning_rate=1e-3, batch_size=B, compute_dtype="fp32", device=0, seed=3, **kw)
        if fresh:
            return m
        _MODELS[nz] = m
    return _MODELS[nz]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("joint", "marginal"))


def _errs(got, ref, nz):
    return float(A.joint_err(got["joint"], ref[0], nz).max()), float(A.marginal_err(got["marginal"], ref[1]).max())


def _dev(model, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(model.device) for a in arrays)


# ------------------------------------------------------------------------------------------------ 1. arithmetic
_CASES = {}
SMALL = [(N, G) for N in (1, 19) for G in (1, 5, 64)]


def _arith_case(nz):
    """Test 1's inputs and tolerances: 64 gallery rows and their 19 standard queries; for every (N, G) of SMALL the float64
    definition on the first N queries and G gallery rows, and over all of them the worst error of the float32 restatement (joint,
    marginal)"""
    if nz not in _CASES:
        rng = np.random.default_rng(100 + nz)
        g = A.latents(rng, 64, nz)
        z = A.queries(rng, g)
        refs, own = {}, [0.0, 0.0]
        for N, G in SMALL:
            sub = (g[0][:G], g[1][:G])
            refs[N, G] = A.logpdf64(z[:N], sub)
            assert np.isfinite(refs[N, G][0]).all() and np.isfinite(refs[N, G][1]).all()
            r32 = A.logpdf32(z[:N], sub)
            own[0] = max(own[0], float(A.joint_err(r32[0], refs[N, G][0], nz).max()))
            own[1] = max(own[1], float(A.marginal_err(r32[1], refs[N, G][1]).max()))
        _CASES[nz] = (z, g, refs, tuple(own))
    return _CASES[nz]


@pytest.mark.parametrize("nz", [7, 20, 64])
def test_density_against_the_float64_definition(V, nz):
    """The bound is 4x the worst error of the float32 restatement over THESE inputs: the kernel runs the restatement's operations
    with the exponent joined by a fused multiply-add, the hardware exponential inside the sums and a different but fixed grouping
    of the gallery rows (blocks of 8 under a running max instead of one global max), each within a small multiple of the
    restatement's own roundings."""
    model = _model(V, nz)
    z, g, refs, own = _arith_case(nz)
    worst = [0.0, 0.0]
    for N, G in SMALL:
        r = model.aggregate_log_density(z[:N], (g[0][:G], g[1][:G]))
        assert r["joint"].shape == (N,) and r["joint"].dtype == np.float32
        assert r["marginal"].shape == (N, nz) and r["marginal"].dtype == np.float32
        ej, em = _errs(r, refs[N, G], nz)
        worst = [max(worst[0], ej), max(worst[1], em)]
    print("n_z=%d: float32 restatement worst error joint %.3e marginal %.3e; kernel worst joint %.3e marginal %.3e (bound 4x)"
          % (nz, own[0], own[1], worst[0], worst[1]))
    assert worst[0] <= 4.0 * own[0] and worst[1] <= 4.0 * own[1]


# ------------------------------------------------------------------------------------------------ 2. tiles, slices, chunks
def _plan(model, rows, G):
    """-> (query_tile, chunk_rows, slice_rows, n_slices)"""
    v = [C.c_int32(-1) for _ in range(4)]
    rc = model._L.avae_agg_logpdf_plan(C.byref(model._cfg), rows, G, *[C.byref(x) for x in v], None)
    assert rc == 0
    return tuple(x.value for x in v)


@pytest.mark.parametrize("N,G", [(65, 65), (130, 1025), (130, 2100), (3, 65537)])
@pytest.mark.parametrize("nz", [7, 64])
def test_several_tiles_slices_and_a_ragged_tail(V, nz, N, G):
    """(65, 65): a second query tile of one row and a second gallery tile of one row; (130, 1025): a second slice of one row;
    (130, 2100): three slices, the last of 52 rows (a tile of 52 = six blocks of 8 and one of 4); (3, 65537): 61 slices of 17
    tiles.  tests/test_aggregate_cpu.py pins these plan figures."""
    model = _model(V, nz)
    rng = np.random.default_rng(1000 * nz + G)
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    ref, r32 = A.logpdf64(z, g), A.logpdf32(z, g)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    own = (float(A.joint_err(r32[0], ref[0], nz).max()), float(A.marginal_err(r32[1], ref[1]).max()))
    ej, em = _errs(model.aggregate_log_density(z, g), ref, nz)
    print("n_z=%d N=%d G=%d: restatement joint %.3e marginal %.3e; kernel joint %.3e marginal %.3e" % (nz, N, G, own[0], own[1], ej, em))
    assert ej <= 4.0 * own[0] and em <= 4.0 * own[1]


def test_a_second_chunk_of_queries(V):
    nz, G = 7, 70
    model = _model(V, nz)
    chunk = _plan(model, 10 ** 6, G)[1]
    N = chunk + 1
    assert _plan(model, N, G)[1] == chunk
    rng = np.random.default_rng(77)
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    ref, r32 = A.logpdf64(z, g), A.logpdf32(z, g)
    own = (float(A.joint_err(r32[0], ref[0], nz).max()), float(A.marginal_err(r32[1], ref[1]).max()))
    ex = np.full(N, -1, np.int64)
    ex[-1] = 3                                                       # the second chunk reads its own exclude entries
    got = model.aggregate_log_density(z, g, exclude=ex)
    ej, em = _errs({k: v[:-1] for k, v in got.items()}, (ref[0][:-1], ref[1][:-1]), nz)
    print("N=%d G=%d: restatement joint %.3e marginal %.3e; kernel joint %.3e marginal %.3e" % (N, G, own[0], own[1], ej, em))
    assert ej <= 4.0 * own[0] and em <= 4.0 * own[1]
    last = A.logpdf64(z[-1:], g, [3])
    lj, lm = _errs({k: v[-1:] for k, v in got.items()}, last, nz)
    assert lj <= 4.0 * own[0] and lm <= 4.0 * own[1]
    assert not np.array_equal(_bits(got["joint"][-1:]), _bits(model.aggregate_log_density(z[-1:], g)["joint"]))


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("nz", [7, 20, 64])
def test_a_query_does_not_depend_on_the_call_it_is_in(V, nz):
    model = _model(V, nz)
    rng = np.random.default_rng(5 + nz)
    G, N = 2100, 130
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    zd, gm, gl = _dev(model, z, g[0], g[1])
    big = model.aggregate_log_density(zd, (gm, gl))
    for i in (0, 63, 64, 129):
        one = model.aggregate_log_density(zd[i:i + 1], (gm, gl))
        assert _same(one, {k: v[i:i + 1] for k, v in big.items()}), i
    assert _same(model.aggregate_log_density(zd, (gm, gl)), big)
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    with torch.cuda.stream(side):
        other = model.aggregate_log_density(zd, (gm, gl))
    side.synchronize()
    torch.cuda.current_stream(model.device).wait_stream(side)
    assert _same(other, big)
    # either output alone: the bits of the full call
    only_j = model.aggregate_log_density(zd, (gm, gl), marginals=False)
    assert only_j["marginal"] is None and np.array_equal(_bits(only_j["joint"]), _bits(big["joint"]))
    marg = torch.full((N, nz), -7.0, dtype=torch.float32, device=model.device)
    rc = model._L.avae_agg_logpdf(model._h, zd.data_ptr(), N, gm.data_ptr(), gl.data_ptr(), G, None, None, marg.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_bits(marg), _bits(big["marginal"]))


# ------------------------------------------------------------------------------------------------ 4. exclusion
@pytest.mark.parametrize("nz", [7, 20, 64])
def test_exclusion(V, nz):
    model = _model(V, nz)
    rng = np.random.default_rng(40 + nz)
    G, N = 133, 70                                                   # three gallery tiles (the last of 5 rows), two query tiles
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    ex = rng.integers(0, G, N)
    ex[:6] = (0, 7, 8, 63, 64, G - 1)                                # block and tile borders
    ex[6:10] = (-1, G, -2 ** 31, 2 ** 31 - 1)                        # these exclude nothing
    ref, r32 = A.logpdf64(z, g, ex), A.logpdf32(z, g, ex)
    own = (float(A.joint_err(r32[0], ref[0], nz).max()), float(A.marginal_err(r32[1], ref[1]).max()))
    got = model.aggregate_log_density(z, g, exclude=ex)
    ej, em = _errs(got, ref, nz)
    print("n_z=%d exclusion: restatement joint %.3e marginal %.3e; kernel joint %.3e marginal %.3e" % (nz, own[0], own[1], ej, em))
    assert ej <= 4.0 * own[0] and em <= 4.0 * own[1]
    plain = model.aggregate_log_density(z, g)
    assert _same({k: v[6:10] for k, v in got.items()}, {k: v[6:10] for k, v in plain.items()})
    assert not np.array_equal(_bits(got["joint"][:6]), _bits(plain["joint"][:6]))
    # NaN / Inf in the excluded row: no bit of that query changes; every other query that counts the row turns NaN where it enters
    row = int(ex[1])                                                 # row 7, excluded by query 1 (and by whoever drew it)
    bad = (g[0].copy(), g[1].copy())
    bad[0][row, 0], bad[1][row, nz - 1] = np.nan, np.inf          # (the other columns of the row stay as they are)
    dirty = model.aggregate_log_density(z, bad, exclude=ex)
    skip = ex == row
    assert skip[1] and _same({k: v[skip] for k, v in dirty.items()}, {k: v[skip] for k, v in got.items()})
    assert np.isnan(dirty["joint"][~skip]).all() and np.isnan(dirty["marginal"][~skip][:, 0]).all()
    # a gallery of one row, excluded: no estimate
    one = model.aggregate_log_density(z[:3], (g[0][:1], g[1][:1]), exclude=[0, -1, 1])
    assert np.isnan(one["joint"][0]) and np.isnan(one["marginal"][0]).all()
    assert np.isfinite(one["joint"][1:]).all() and np.isfinite(one["marginal"][1:]).all()


# ------------------------------------------------------------------------------------------------ 5. edges and errors
def test_edges_and_errors_of_the_c_abi(V):
    nz = 20
    model = _model(V, nz)
    L, h, dev = model._L, model._h, model.device
    rng = np.random.default_rng(9)
    G, N = 70, 6
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    zd, gm, gl = _dev(model, z, g[0], g[1])

    def call(z_, rows, gm_, gl_, G_, ex_, joint, marg):
        p = lambda x: None if x is None else x.data_ptr()
        rc = L.avae_agg_logpdf(h, p(z_), rows, p(gm_), p(gl_), G_, p(ex_), p(joint), p(marg), None)
        torch.cuda.synchronize()
        return rc

    def outs(rows=N):
        return (torch.full((rows,), -7.0, dtype=torch.float32, device=dev), torch.full((rows, nz), -7.0, dtype=torch.float32, device=dev))
    j0, m0 = outs()
    assert call(zd, N, gm, gl, G, None, j0, m0) == 0
    clean_j, clean_m = _bits(j0), _bits(m0)
    ref = A.logpdf64(z, g)
    assert A.joint_err(j0.cpu().numpy(), ref[0], nz).max() < 1e-5 and A.marginal_err(m0.cpu().numpy(), ref[1]).max() < 1e-5
    # rows = 0: nothing is written, nothing is read (NULL inputs are fine)
    j, m = outs()
    assert call(None, 0, gm, gl, G, None, j, m) == 0 and call(zd, 0, None, None, 0, None, j, m) == 0
    assert (j == -7.0).all() and (m == -7.0).all()
    # an empty gallery: NaN ("no estimate"), no gallery pointer needed
    assert call(zd, N, None, None, 0, None, j, m) == 0
    assert torch.isnan(j).all() and torch.isnan(m).all()
    # a query whose every term is -Inf: -Inf, not NaN; its neighbours keep their bits
    far = z.copy()
    far[2] = 1e30
    j, m = outs()
    assert call(_dev(model, far)[0], N, gm, gl, G, None, j, m) == 0
    assert torch.isneginf(j[2]) and torch.isneginf(m[2]).all()
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(_bits(j)[keep], clean_j[keep]) and np.array_equal(_bits(m)[keep], clean_m[keep])
    # a gallery row with lv = +Inf contributes 0: the density of the other rows times (G - 1) / G
    wide = g[1].copy()
    wide[65] = np.inf
    j, m = outs()
    assert call(zd, N, gm, _dev(model, wide)[0], G, None, j, m) == 0
    rest = A.logpdf64(z, (np.delete(g[0], 65, 0), np.delete(g[1], 65, 0)))
    shift = np.log((G - 1) / G)
    assert A.joint_err(j.cpu().numpy(), rest[0] + shift, nz).max() < 1e-5
    assert A.marginal_err(m.cpu().numpy(), rest[1] + shift).max() < 1e-5
    # a NaN at gallery (g, j): column j of the marginals and the joint of every query; every other bit stays
    for nan_mu in (True, False):
        bm, bl = g[0].copy(), g[1].copy()
        (bm if nan_mu else bl)[41, 3] = np.nan
        j, m = outs()
        assert call(zd, N, *_dev(model, bm, bl), G, None, j, m) == 0
        assert torch.isnan(j).all() and torch.isnan(m[:, 3]).all()
        other = [c for c in range(nz) if c != 3]
        assert np.array_equal(_bits(m)[:, other], clean_m[:, other])
    # a NaN at z[n, j]: marginal[n, j] and joint[n] only
    zn = z.copy()
    zn[4, 11] = np.nan
    j, m = outs()
    assert call(_dev(model, zn)[0], N, gm, gl, G, None, j, m) == 0
    mask = np.zeros((N, nz), bool)
    mask[4, 11] = True
    assert np.array_equal(np.isnan(m.cpu().numpy()), mask) and np.array_equal(np.isnan(j.cpu().numpy()), mask.any(1))
    rest_q = [0, 1, 2, 3, 5]
    assert np.array_equal(_bits(m)[~mask], clean_m[~mask]) and np.array_equal(_bits(j)[rest_q], clean_j[rest_q])
    # errors: nonzero, a message that names the argument, outputs untouched
    j, m = outs()
    for args, needle in (((zd, -1, gm, gl, G, None, j, m), "rows"),
                         ((zd, N, gm, gl, -1, None, j, m), "gallery_rows"),
                         ((None, N, gm, gl, G, None, j, m), "z_dev"),
                         ((zd, N, None, gl, G, None, j, m), "g_mu_dev"),
                         ((zd, N, gm, None, G, None, j, m), "g_logvar_dev"),
                         ((zd, N, gm, gl, G, None, None, None), "joint_dev and marginal_dev")):
        assert call(*args) != 0, needle
        assert needle in L.avae_last_error(h).decode(), needle
    assert (j == -7.0).all() and (m == -7.0).all()
    # ... and the handle still works
    assert call(zd, N, gm, gl, G, None, j, m) == 0 and np.array_equal(_bits(j), clean_j) and np.array_equal(_bits(m), clean_m)


# ------------------------------------------------------------------------------------------------ 6. Python
def _check_decomposition(got, want, tol, nz, given=(0, 1)):
    for m in given:
        scale = tol * want["scale"][m]
        for key in ("kl", "mi", "tc", "marginal_kl"):
            assert abs(got[key][m] - want[key][m]) <= scale, (key, m, got[key][m], want[key][m], scale)
        assert np.abs(got["dimwise_kl"][m] - want["dimwise_kl"][m]).max() <= scale, m
        for d in given:                                              # (the log-density behind cross[m, d] is q_agg^d's at z^m)
            assert abs(got["cross"][m, d] - want["cross"][m, d]) <= tol * want["cross_scale"][m, d], (m, d)
        assert got["cross"][m, m] == 0.0
        terms = [got["mi"][m], got["tc"][m]] + list(got["dimwise_kl"][m])
        assert abs(got["kl"][m] - sum(terms)) <= 1e-10 * sum(abs(t) for t in terms)


@pytest.mark.parametrize("nz", [7, 20, 64])
def test_python_surface_and_elbo_decomposition(V, nz):
    N = 48
    model = _model(V, nz, fresh=True, ema=0.9)
    rng = np.random.default_rng(13)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    for i in range(3):                                               # a few steps, so that the average differs from the weights
        model.partial_fit([x[:B] for x in X], rng.standard_normal((B, nz)).astype(np.float32))
    post = model.posterior(X)
    own = _arith_case(nz)[3]
    tol = 4.0 * max(own)
    # NumPy in, NumPy out; tensors in, device tensors out; marginals=False
    z = post[0][0] + np.exp(0.5 * post[0][1]) * rng.standard_normal((N, nz)).astype(np.float32)
    a = model.aggregate_log_density(z, post[1])
    assert isinstance(a["joint"], np.ndarray) and a["joint"].shape == (N,) and a["marginal"].shape == (N, nz)
    ref = A.logpdf64(z, post[1])
    assert A.joint_err(a["joint"], ref[0], nz).max() <= 1e-5 and A.marginal_err(a["marginal"], ref[1]).max() <= 1e-5
    t = model.aggregate_log_density(torch.from_numpy(z).to(model.device), tuple(_dev(model, *post[1])), marginals=False)
    assert torch.is_tensor(t["joint"]) and t["joint"].is_cuda and t["joint"].dtype == torch.float32 and t["marginal"] is None
    assert np.array_equal(_bits(t["joint"]), _bits(a["joint"]))
    with pytest.raises(ValueError, match="exclude"):
        model.aggregate_log_density(z, post[1], exclude=np.zeros(N - 1, np.int32))
    with pytest.raises(ValueError, match="pair"):
        model.aggregate_log_density(z, post[1][0])
    # the decomposition against the float64 definition on the model's own posteriors
    for S in (1, 3):
        eps = rng.standard_normal((S, N, nz)).astype(np.float32)
        for loo in (False, True):
            got = model.elbo_decomposition(X, n_samples=S, eps=eps, leave_one_out=loo)
            want = A.decomposition64(post, eps, leave_one_out=loo)
            assert got["kl"].dtype == np.float64 and got["kl"].shape == (2,) and got["dimwise_kl"].shape == (2, nz)
            assert got["cross"].shape == (2, 2) and got["log_n"] == np.log(N)
            _check_decomposition(got, want, tol, nz)
            if not loo:
                assert np.all(got["mi"] <= got["log_n"] + tol * want["scale"])
    # a None modality: NaN entries, the other modality's entries unchanged
    half = model.elbo_decomposition([X[0], None], n_samples=3, eps=eps)
    full = model.elbo_decomposition(X, n_samples=3, eps=eps)
    assert np.isnan(half["kl"][1]) and np.isnan(half["dimwise_kl"][1]).all() and np.isnan(half["cross"][1]).all() and np.isnan(half["cross"][0, 1])
    for key in ("kl", "mi", "tc", "marginal_kl", "dimwise_kl"):
        assert np.array_equal(half[key][0], full[key][0]), key
    assert half["cross"][0, 0] == 0.0
    # seed reproduces bit for bit, another seed does not; tensors in, tensors out
    s1, s2, s3 = (model.elbo_decomposition(X, n_samples=2, seed=s) for s in (5, 5, 6))
    assert all(np.array_equal(s1[k], s2[k]) for k in ("kl", "mi", "tc", "dimwise_kl", "cross")) and not np.array_equal(s1["kl"], s3["kl"])
    td = model.elbo_decomposition([torch.from_numpy(x).to(model.device) for x in X], n_samples=2, seed=5)
    assert torch.is_tensor(td["kl"]) and td["kl"].dtype == torch.float64 and np.array_equal(td["kl"].cpu().numpy(), s1["kl"])
    with pytest.raises(ValueError, match="n_samples"):
        model.elbo_decomposition(X, n_samples=0)
    with pytest.raises(ValueError, match="eps"):
        model.elbo_decomposition(X, n_samples=2, eps=eps)
    # inside averaged(): the averaged encoders' decomposition
    with model.averaged():
        avg_post = model.posterior(X)
        in_avg = model.elbo_decomposition(X, n_samples=3, eps=eps)
        given = model.aggregate_log_density(z, post[1])             # given latents: the switch changes nothing
    assert not np.array_equal(_bits(avg_post[0][0]), _bits(post[0][0]))
    _check_decomposition(in_avg, A.decomposition64(avg_post, eps), tol, nz)
    assert not np.array_equal(in_avg["kl"], full["kl"]) and _same(given, a)
    assert np.array_equal(model.elbo_decomposition(X, n_samples=3, eps=eps)["kl"], full["kl"])          # switched back


# ------------------------------------------------------------------------------------------------ 7. no side effects
def test_density_calls_have_no_side_effects_on_training(V):
    nz = 20
    rng = np.random.default_rng(21)
    Xt = synth_batch(rng, 2 * B, WIDTHS, [True, False])
    et = rng.standard_normal((2 * B, nz)).astype(np.float32)
    Xq = synth_batch(rng, 19, WIDTHS, [True, False])
    gal = A.latents(rng, 1100, nz)
    state = lambda m: m.get_opt_state() + (m.get_params(), m.cost_history(1))
    runs = []
    for with_calls in (False, True):
        model = _model(V, nz, fresh=True)
        model.partial_fit([x[:B] for x in Xt], et[:B])
        before = state(model)
        if with_calls:
            model.aggregate_log_density(A.queries(rng, gal), gal, exclude=np.arange(19))
            model.aggregate_log_density(A.queries(rng, gal), gal, marginals=False)
            model.elbo_decomposition(Xq, n_samples=2, leave_one_out=True)
            model.synchronize()
            for x, y in zip(before, state(model)):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        cost = model.partial_fit([x[B:] for x in Xt], et[B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append((np.float32(cost), model.get_grads()) + state(model))
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x), np.asarray(y))
