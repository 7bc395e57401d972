"""fit_latent_prior / latent_prior_score / sample_latent_prior (avae_gmm_fit, avae_gmm_score) on a real MI355X (include/avae.h,
DESIGN.md section 21) against tests/latent_prior_reference.py.

1. one iteration against the float64 definition, within 4x the float32 restatement's own worst error on the same inputs (error
   measures |err| for weights and responsibilities, |err| / (|ref| + 1) for means and log-variances, |err| / (|ref| + n_z) for ll
   and the bound); 2. several slices and tiles; 3. a 30-iteration fit against the float64 trajectory; 4. assignments;
5. consistency with the score and with aggregate_log_density; 6. determinism; 7. edges and errors of the C ABI; 8. the Python
surface; 9. no side effects on training.

batch_size = 16, small MLPs, n_z in {7, 20, 64}; the data are clusters(sep = 3): centres N(0, 9), within-cluster scale U(0.3, 1),
lv ~ U(-6, 1), seeded."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_prior_reference as P
from conftest import make_arch, shadow_err, synth_batch

pytestmark = pytest.mark.gpu

B = 16
WIDTHS = (784, 147)
KEYS = ("weights", "means", "logvars")


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
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_fit(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS + ("bound",)) and a["n_used"] == b["n_used"]


def _dev(model, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(model.device) for a in arrays)


def _step_errs(got, ref, bound_ref, nz):
    return P.prior_errs(got, ref, got["bound"][:1], [bound_ref], nz)


# ------------------------------------------------------------------------------------------------ 1. one iteration
SMALL = [(K, N) for K in (1, 3, 10, 64) for N in (1, 19, 64, 65, 300)]
_CASES = {}


def _step_case(nz):
    """Test 1's inputs and tolerances: for every (K, N) of SMALL, with and without logvar, the data, the initial parameters and
    the float64 iteration; over all of them the worst error of the float32 restatement (weights, means, logvars, bound)"""
    if nz not in _CASES:
        cases, own = [], [0.0] * 4
        for K, N in SMALL:
            rng = np.random.default_rng(1000 * nz + 10 * K + N)
            mu, lv, _ = P.clusters(rng, N, nz, min(K, 4), 3.0)
            for logvar in (lv, None):
                init = P.start(rng, mu, logvar, K)
                ref, bound, n = P.step64(mu, logvar, init)
                assert n == N and np.isfinite(bound) and all(np.isfinite(ref[k]).all() for k in KEYS)
                r32, b32, _ = P.step32(mu, logvar, init)
                own = [max(o, e) for o, e in zip(own, P.prior_errs(r32, ref, [b32], [bound], nz))]
                cases.append((K, N, mu, logvar, init, ref, bound))
        _CASES[nz] = (cases, tuple(own))
    return _CASES[nz]


@pytest.mark.parametrize("nz", [7, 20, 64])
def test_one_iteration_against_the_float64_definition(V, nz):
    """The bound is 4x the worst error of the float32 restatement over THESE inputs, per quantity: the kernel runs the
    restatement's operations with fused multiply-adds in the exponent and in the sums, fp32 sums over 64 rows and fp64 sums across
    the tiles and in the update -- if anything more accurate.  Measured on the MI355X, 2026-10-18, kernel worst / restatement
    worst (weights, means, logvars, bound): n_z = 7: 1.5e-7 / 1.8e-7, 9.4e-7 / 9.9e-7, 3.9e-6 / 5.9e-6, 5.9e-8 / 1.4e-7; n_z = 20:
    4.2e-7 / 5.4e-7, 4.8e-6 / 4.7e-6, 3.1e-5 / 4.9e-5, 1.0e-7 / 2.1e-7; n_z = 64: 4.6e-6 / 4.6e-6, 1.5e-5 / 1.5e-5, 4.2e-3 / 3.4e-3,
    1.9e-7 / 2.5e-7 (the log-variances' worst is a nearly empty component of K = 64 at N = 19, in both)."""
    model = _model(V, nz)
    cases, own = _step_case(nz)
    worst = [0.0] * 4
    for K, N, mu, logvar, init, ref, bound in cases:
        got = model.fit_latent_prior((mu, logvar), n_components=K, n_iters=1, init=init)
        assert got["weights"].shape == (K,) and got["means"].shape == (K, nz) and got["logvars"].shape == (K, nz)
        assert all(got[k].dtype == np.float32 for k in KEYS) and got["bound"].dtype == np.float64 and got["bound"].shape == (2,)
        assert got["n_used"] == N and np.isfinite(got["bound"]).all()
        errs = _step_errs(got, ref, bound, nz)
        assert all(e <= 4.0 * o for e, o in zip(errs, own)), (K, N, logvar is None, errs, own)
        worst = [max(w, e) for w, e in zip(worst, errs)]
    print("n_z=%d: float32 restatement worst error weights %.3e means %.3e logvars %.3e bound %.3e; "
          "kernel worst weights %.3e means %.3e logvars %.3e bound %.3e (bound 4x)" % ((nz,) + own + tuple(worst)))


def test_large_offset_keeps_the_variance(V):
    """The same data plus 1e3 on every mean: the sums are shifted by the current mean, so the variance does not come from a
    difference of large numbers.  Same rule.  Measured (weights, means, logvars, bound): kernel 7.5e-8, 6.1e-8, 1.6e-6, 2.1e-8;
    restatement 6.0e-8, 6.1e-8, 1.4e-6, 1.3e-7 -- the restatement takes its sums about the current mean too, so its own error
    stays small here as well; raw moments at this offset would lose the variance altogether (1e6 against 0.1 to 1 in float32)."""
    nz, K, N = 20, 3, 300
    model = _model(V, nz)
    rng = np.random.default_rng(4242)
    mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
    mu = P.with_offset(mu)
    init = P.start(rng, mu, lv, K)
    ref, bound, _ = P.step64(mu, lv, init)
    r32, b32, _ = P.step32(mu, lv, init)
    own = P.prior_errs(r32, ref, [b32], [bound], nz)
    got = model.fit_latent_prior((mu, lv), n_components=K, n_iters=1, init=init)
    errs = _step_errs(got, ref, bound, nz)
    print("offset 1e3, n_z=%d K=%d N=%d: restatement weights %.3e means %.3e logvars %.3e bound %.3e; kernel %.3e %.3e %.3e %.3e"
          % ((nz, K, N) + own + errs))
    assert all(e <= 4.0 * o for e, o in zip(errs, own)), (errs, own)
    assert np.abs(got["logvars"]).max() < 5.0, "the spread of the clusters, not of the offset"


# ------------------------------------------------------------------------------------------------ 2. slices and tiles
def _plan(model, rows, K):
    v = [C.c_int32(-1) for _ in range(2)]
    assert model._L.avae_gmm_plan(C.byref(model._cfg), rows, K, C.byref(v[0]), C.byref(v[1]), None) == 0
    return v[0].value, v[1].value


@pytest.mark.parametrize("which", ["slice+37", "2 slices+1", "20000", "40000"])
def test_several_slices_and_a_ragged_tail(V, which):
    """Measured, kernel / restatement (weights, means, logvars, bound), worst of the two variants: N = 101: 1.6e-7 / 1.6e-7,
    1.2e-6 / 1.8e-6, 2.5e-6 / 2.6e-6, 4.3e-8 / 6.3e-8; N = 129: 3.1e-7 / 3.4e-7, 1.1e-6 / 1.2e-6, 3.2e-6 / 3.2e-6, 5.3e-8 / 8.7e-8;
    N = 20,000: 1.3e-7 / 4.8e-7, 3.1e-7 / 6.8e-6, 5.0e-7 / 5.7e-5, 3.2e-8 / 1.5e-6; N = 40,000: 1.2e-7 / 2.6e-6, 3.1e-7 / 4.0e-5,
    1.5e-6 / 3.0e-4, 5.0e-8 / 1.5e-6 (fp64 across the tiles against one float32 running sum).  The bound is one number per case,
    so the restatement's own error on it is one rounding accident: over 40 seeds at N = 129 it ranges from 1.2e-9 to 3.3e-7
    (median 8.0e-8), the kernel's 2.4e-8 to 5.3e-8 here."""
    nz, K = 20, 10
    model = _model(V, nz)
    per = _plan(model, 1, K)[0]
    N = {"slice+37": per + 37, "2 slices+1": 2 * per + 1, "20000": 20000, "40000": 40000}[which]
    per = {20000: 2 * per, 40000: 3 * per}.get(N, per)               # 157 slices of two tiles (the last of 32 rows), 209 of three
    assert _plan(model, N, K) == (per, -(-N // per)) and per % 64 == 0
    rng = np.random.default_rng(N)
    mu, lv, _ = P.clusters(rng, N, nz, 4, 3.0)
    runs, own = [], [0.0] * 4
    for logvar in (lv, None):                                        # as in test 1, a case is its inputs with and without logvar
        init = P.start(rng, mu, logvar, K)
        ref, bound, _ = P.step64(mu, logvar, init)
        r32, b32, _ = P.step32(mu, logvar, init)
        own = [max(o, e) for o, e in zip(own, P.prior_errs(r32, ref, [b32], [bound], nz))]
        got = model.fit_latent_prior((mu, logvar), n_components=K, n_iters=1, init=init)
        assert got["n_used"] == N
        runs.append(_step_errs(got, ref, bound, nz))
    errs = tuple(max(e) for e in zip(*runs))
    print("N=%d (%d slices of %d): restatement weights %.3e means %.3e logvars %.3e bound %.3e; kernel %.3e %.3e %.3e %.3e"
          % ((N, -(-N // per), per) + tuple(own) + errs))
    assert all(e <= 4.0 * o for e, o in zip(errs, own)), (runs, own)


# ------------------------------------------------------------------------------------------------ 3. a 30-iteration fit
FITS = [(7, 3, 300), (20, 10, 2000), (64, 16, 2000)]
_FITS = {}


def _fit_case(V, nz, K, N):
    """clusters(sep = 3), its start, the float64 and float32 trajectories of 30 iterations and the device's fit (NumPy)"""
    if (nz, K, N) not in _FITS:
        rng = np.random.default_rng(7000 + nz)
        mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
        init = P.start(rng, mu, lv, K)
        ref, b64, _ = P.fit64(mu, lv, init, 30)
        r32, b32 = P.fit32(mu, lv, init, 30)
        got = _model(V, nz).fit_latent_prior((mu, lv), n_components=K, n_iters=30, init=init)
        _FITS[nz, K, N] = (mu, lv, init, ref, b64, r32, b32, got)
    return _FITS[nz, K, N]


@pytest.mark.parametrize("nz,K,N", FITS)
def test_thirty_iterations_follow_the_float64_trajectory(V, nz, K, N):
    """Final parameters and the whole bound history within 4x the float32 restatement's own deviation after its 30 iterations on
    the same inputs (the runs do not fork: tests/test_latent_prior_cpu.py).  The bound may fall between iterations by no more than
    test 1's allowance for the bound at this n_z.  Measured ratios kernel / restatement (weights, means, logvars, bound): (7, 3,
    300): 0.53, 3.00, 0.72, 0.10; (20, 10, 2000): 0 / 0, 0.46, 0.07, 0.17; (64, 16, 2000): 0.79, 0.77, 0.77, 1.79.  The bound fell
    once, by 9.5e-10 (n_z = 20, at convergence)."""
    mu, lv, init, ref, b64, r32, b32, got = _fit_case(V, nz, K, N)
    own = P.prior_errs(r32, ref, b32, b64, nz)
    errs = P.prior_errs(got, ref, got["bound"], b64, nz)
    print("n_z=%d K=%d N=%d, 30 iterations: restatement weights %.3e means %.3e logvars %.3e bound %.3e; kernel %.3e %.3e %.3e %.3e; "
          "ratios %s" % ((nz, K, N) + own + errs + (["%.2f" % (e / o) if o else ("0/0" if e == 0 else "inf") for e, o in zip(errs, own)],)))
    assert got["n_used"] == N and got["bound"].shape == (31,)
    assert all(e <= 4.0 * o for e, o in zip(errs, own)), (errs, own)
    allowance = 4.0 * _step_case(nz)[1][3] * (np.abs(got["bound"][:-1]) + nz)
    fall = got["bound"][:-1] - got["bound"][1:]
    print("largest fall of the bound %.3e (allowance %.3e)" % (fall.max(), allowance.min()))
    assert (fall <= allowance).all()
    assert got["bound"][-1] > got["bound"][0]


# ------------------------------------------------------------------------------------------------ 4. assignments
@pytest.mark.parametrize("nz,K,N", FITS)
def test_assignments_and_responsibilities(V, nz, K, N):
    mu, lv, _, _, _, _, _, got = _fit_case(V, nz, K, N)
    model = _model(V, nz)
    prior = {k: got[k] for k in KEYS}
    sc = model.latent_prior_score((mu, lv), prior, responsibilities=True)
    assert sc["log_density"].shape == (N,) and sc["log_density"].dtype == np.float32
    assert sc["component"].shape == (N,) and sc["component"].dtype == np.int32
    assert sc["responsibilities"].shape == (N, K) and sc["responsibilities"].dtype == np.float32
    ll64, r64 = P.estep64(mu, lv, prior)
    ll32, r32 = P.estep32(mu, lv, prior)
    top = np.sort(r64, axis=1)[:, ::-1]
    clear = (top[:, 0] - top[:, 1] >= 1e-3) if K > 1 else np.ones(N, bool)
    assert (~clear).mean() <= 0.01, (~clear).mean()
    assert np.array_equal(sc["component"][clear], r64.argmax(axis=1)[clear])
    own_r, own_ll = float(P.abs_err(r32, r64).max()), float(P.ll_err(ll32, ll64, nz).max())
    err_r, err_ll = float(P.abs_err(sc["responsibilities"], r64).max()), float(P.ll_err(sc["log_density"], ll64, nz).max())
    print("n_z=%d K=%d N=%d: %d rows left out; restatement resp %.3e ll %.3e; kernel resp %.3e ll %.3e"
          % (nz, K, N, int((~clear).sum()), own_r, own_ll, err_r, err_ll))
    assert err_r <= 4.0 * own_r and err_ll <= 4.0 * own_ll
    # r_k = p_k / sum with sum the float32 sum of K terms: |sum_k r_k - 1| <= K 2^-24 to first order
    assert np.abs(sc["responsibilities"].astype(np.float64).sum(axis=1) - 1.0).max() <= 4.0 * K * 2.0 ** -24
    assert np.array_equal(sc["component"], sc["responsibilities"].argmax(axis=1)), "argmax of r, ties to the lower index"


# ------------------------------------------------------------------------------------------------ 5. consistency
@pytest.mark.parametrize("nz,K,N", FITS)
def test_the_bound_is_the_mean_of_the_scores(V, nz, K, N):
    mu, lv, _, _, _, _, _, got = _fit_case(V, nz, K, N)
    ll = _model(V, nz).latent_prior_score((mu, lv), {k: got[k] for k in KEYS})["log_density"].astype(np.float64)
    # the same fp32 numbers, summed in fp64 in another order
    assert abs(ll.mean() - got["bound"][-1]) <= N * 2.0 ** -52 * np.abs(ll).max()


@pytest.mark.parametrize("nz", [7, 20, 64])
def test_points_under_uniform_weights_agree_with_aggregate_log_density(V, nz):
    """the mixture of K equally weighted components IS the aggregate posterior of a gallery of K rows: the two kernels agree within
    the sum of their test-1 bounds"""
    import aggregate_reference as A
    import test_gpu_aggregate as TA
    model = _model(V, nz)
    K, N = 10, 130
    rng = np.random.default_rng(50 + nz)
    mu, lv, _ = P.clusters(rng, N, nz, 4, 3.0)
    prior = P.start(rng, mu, lv, K)
    prior["weights"] = np.full(K, 1.0 / K, np.float32)
    prior["logvars"] = (prior["logvars"] + rng.uniform(-1, 1, size=(K, nz))).astype(np.float32)
    ref = P.estep64(mu, None, prior)[0]
    assert np.abs(ref - A.logpdf64(mu, (prior["means"], prior["logvars"]))[0]).max() <= 1e-9 * (np.abs(ref).max() + nz)
    ours = model.latent_prior_score(mu, prior)["log_density"]
    agg = model.aggregate_log_density(mu, (prior["means"], prior["logvars"]), marginals=False)["joint"]
    allowance = 4.0 * _step_case(nz)[1][3] + 4.0 * TA._arith_case(nz)[3][0]
    gap = np.abs(ours.astype(np.float64) - agg.astype(np.float64)) / (np.abs(ref) + nz)
    print("n_z=%d: largest gap to aggregate_log_density %.3e (allowance %.3e)" % (nz, gap.max(), allowance))
    assert gap.max() <= allowance


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_fits_and_scores_are_bit_reproducible(V):
    nz, K, N = 20, 10, 2000
    mu, lv, init, _, _, _, _, got = _fit_case(V, nz, K, N)
    model = _model(V, nz)
    md, ld = _dev(model, mu, lv)
    dinit = dict(zip(KEYS, _dev(model, *[init[k] for k in KEYS])))
    again = model.fit_latent_prior((md, ld), n_components=K, n_iters=30, init=dinit)
    assert torch.is_tensor(again["means"]) and _same_fit(again, got)
    assert np.array_equal(_bits(dinit["means"]), _bits(init["means"])), "the caller's init is not written"
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    with torch.cuda.stream(side):
        other = model.fit_latent_prior((md, ld), n_components=K, n_iters=30, init=dinit)
    side.synchronize()
    torch.cuda.current_stream(model.device).wait_stream(side)
    assert _same_fit(other, got)
    # 12 iterations, then 18 more from the output: the bits of 30
    first = model.fit_latent_prior((mu, lv), n_components=K, n_iters=12, init=init)
    rest = model.fit_latent_prior((mu, lv), n_components=K, n_iters=18, init={k: first[k] for k in KEYS})
    assert all(np.array_equal(_bits(rest[k]), _bits(got[k])) for k in KEYS)
    assert np.array_equal(_bits(first["bound"]), _bits(got["bound"][:13])) and np.array_equal(_bits(rest["bound"]), _bits(got["bound"][12:]))


def test_a_row_does_not_depend_on_the_call_it_is_in(V):
    nz, K, N = 20, 10, 20000
    model = _model(V, nz)
    rng = np.random.default_rng(66)
    mu, lv, _ = P.clusters(rng, N, nz, 4, 3.0)
    prior = dict(zip(KEYS, _dev(model, *[P.start(rng, mu, lv, K)[k] for k in KEYS])))
    md, ld = _dev(model, mu, lv)
    big = model.latent_prior_score((md, ld), prior, responsibilities=True)
    names = ("log_density", "component", "responsibilities")
    for i in (0, 63, 64, 300, 19999):
        one = model.latent_prior_score((md[i:i + 1], ld[i:i + 1]), prior, responsibilities=True)
        assert all(np.array_equal(_bits(one[k]), _bits(big[k][i:i + 1])) for k in names), i
    again = model.latent_prior_score((md, ld), prior, responsibilities=True)
    assert all(np.array_equal(_bits(again[k]), _bits(big[k])) for k in names)
    # each output alone: the bits of the full call
    outs = (torch.full((N,), -7.0, dtype=torch.float32, device=model.device), torch.full((N,), -7, dtype=torch.int32, device=model.device),
            torch.full((N, K), -7.0, dtype=torch.float32, device=model.device))
    for i, name in enumerate(names):
        ptrs = [None, None, None]
        ptrs[i] = outs[i].data_ptr()
        rc = model._L.avae_gmm_score(model._h, md.data_ptr(), ld.data_ptr(), N, K, prior["weights"].data_ptr(), prior["means"].data_ptr(),
                                     prior["logvars"].data_ptr(), ptrs[0], ptrs[1], ptrs[2], None)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(_bits(outs[i]), _bits(big[name])), name


# ------------------------------------------------------------------------------------------------ 7. edges and errors
def test_non_finite_rows_are_skipped(V):
    nz, K, N = 20, 3, 150
    model = _model(V, nz)
    rng = np.random.default_rng(70)
    mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
    init = P.start(rng, mu, lv, K)
    clean = model.fit_latent_prior((mu, lv), n_components=K, n_iters=5, init=init)
    # ... as the last two rows: bitwise the fit of the data without them
    bm, bl = np.vstack([mu, mu[:2]]), np.vstack([lv, lv[:2]])
    bm[N, 4], bl[N + 1, 0] = np.nan, np.inf
    tail = model.fit_latent_prior((bm, bl), n_components=K, n_iters=5, init=init)
    assert tail["n_used"] == N and _same_fit(tail, clean)
    # ... in the middle: the tiles shift, test 1's bound against the float64 iteration
    mm, ml = np.insert(mu, [7, 70], mu[:2], axis=0), np.insert(lv, [7, 70], lv[:2], axis=0)
    mm[7, 4], ml[71, 0] = np.nan, -np.inf
    ref, bound, n = P.step64(mm, ml, init)
    mid = model.fit_latent_prior((mm, ml), n_components=K, n_iters=1, init=init)
    own = _step_case(nz)[1]
    assert n == N and mid["n_used"] == N
    assert all(e <= 4.0 * o for e, o in zip(_step_errs(mid, ref, bound, nz), own))
    # their scores: NaN / -1 / NaN, the other rows keep their bits
    prior = {k: clean[k] for k in KEYS}
    sc = model.latent_prior_score((mm, ml), prior, responsibilities=True)
    ok = model.latent_prior_score((mu, lv), prior, responsibilities=True)
    bad = np.zeros(N + 2, bool)
    bad[[7, 71]] = True
    assert np.isnan(sc["log_density"][bad]).all() and (sc["component"][bad] == -1).all() and np.isnan(sc["responsibilities"][bad]).all()
    for k in ("log_density", "component", "responsibilities"):
        assert np.array_equal(_bits(sc[k][~bad]), _bits(ok[k]))
    # every row non-finite: the parameters stay as given, the bound is NaN
    none = model.fit_latent_prior((np.full((5, nz), np.nan, np.float32), None), n_components=K, n_iters=3, init=init)
    assert none["n_used"] == 0 and np.isnan(none["bound"]).all() and none["bound"].shape == (4,)
    assert all(np.array_equal(_bits(none[k]), _bits(init[k])) for k in KEYS)
    with pytest.raises(ValueError, match="more than the 0 rows"):
        model.fit_latent_prior((np.full((5, nz), np.nan, np.float32), None), n_components=K)


def test_zero_iterations_zero_rows_far_components_and_the_floor(V):
    nz, K, N = 7, 3, 100
    model = _model(V, nz)
    rng = np.random.default_rng(71)
    mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
    init = P.start(rng, mu, lv, K)
    # n_iters = 0 scores the initial parameters and returns them untouched
    zero = model.fit_latent_prior((mu, lv), n_components=K, n_iters=0, init=init)
    one = model.fit_latent_prior((mu, lv), n_components=K, n_iters=1, init=init)
    assert zero["bound"].shape == (1,) and zero["n_used"] == N and np.array_equal(_bits(zero["bound"]), _bits(one["bound"][:1]))
    assert all(np.array_equal(_bits(zero[k]), _bits(init[k])) for k in KEYS)
    # rows = 0: not an error
    empty = model.fit_latent_prior((mu[:0], lv[:0]), n_components=K, n_iters=2, init=init)
    assert empty["n_used"] == 0 and np.isnan(empty["bound"]).all() and all(np.array_equal(_bits(empty[k]), _bits(init[k])) for k in KEYS)
    sc = model.latent_prior_score(mu[:0], init, responsibilities=True)
    assert sc["log_density"].shape == (0,) and sc["component"].shape == (0,) and sc["responsibilities"].shape == (0, K)
    # a component 1e4 away stays where it is, its weight goes to 0, nothing turns NaN
    far = {k: v.copy() for k, v in init.items()}
    far["means"][1] = 1e4
    got = model.fit_latent_prior((mu, lv), n_components=K, n_iters=4, init=far)
    assert got["weights"][1] == 0.0 and np.array_equal(_bits(got["means"][1]), _bits(far["means"][1]))
    assert np.array_equal(_bits(got["logvars"][1]), _bits(far["logvars"][1]))
    assert all(np.isfinite(got[k]).all() for k in KEYS) and np.isfinite(got["bound"]).all()
    assert abs(float(got["weights"].sum()) - 1.0) < 1e-6
    # the floor: K = N = 3 points, every component on its own point
    x = (3.0 * np.eye(3, nz)).astype(np.float32)
    own = {"weights": np.full(3, 1 / 3, np.float32), "means": x.copy(), "logvars": np.full((3, nz), -4.0, np.float32)}
    got = model.fit_latent_prior((x, None), n_components=3, n_iters=3, init=own, var_floor=1e-3)
    assert np.array_equal(got["logvars"], np.full((3, nz), np.float32(np.log(np.float64(np.float32(1e-3)))), np.float32))
    assert np.array_equal(got["means"], x) and np.isfinite(got["bound"]).all()
    seeded = model.fit_latent_prior((x, None), n_components=3, n_iters=3)
    assert seeded["n_used"] == 3 and all(np.isfinite(seeded[k]).all() for k in KEYS) and np.isfinite(seeded["bound"]).all()


def test_errors_of_the_c_abi(V):
    nz, K, N = 20, 3, 40
    model = _model(V, nz)
    L, h, dev = model._L, model._h, model.device
    rng = np.random.default_rng(72)
    mu, lv, _ = P.clusters(rng, N, nz, K, 3.0)
    init = P.start(rng, mu, lv, K)
    md, ld, w, m, s = _dev(model, mu, lv, *[init[k] for k in KEYS])
    bound = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    used = torch.full((1,), -7, dtype=torch.int32, device=dev)
    p = lambda x: None if x is None else x.data_ptr()

    def fit(mu_=md, lv_=ld, rows=N, K_=K, T=2, vf=1e-6, w_=w, m_=m, s_=s, b_=bound, u_=used):
        rc = L.avae_gmm_fit(h, p(mu_), p(lv_), rows, K_, T, vf, p(w_), p(m_), p(s_), p(b_), p(u_), None)
        torch.cuda.synchronize()
        return rc
    for kw, needle in ((dict(rows=-1), "rows must be >= 0"), (dict(K_=0), "n_components = 0"), (dict(K_=65), "n_components = 65"),
                       (dict(T=-1), "n_iters"), (dict(vf=0.0), "var_floor"), (dict(vf=-1.0), "var_floor"), (dict(vf=float("inf")), "var_floor"),
                       (dict(vf=float("nan")), "var_floor"), (dict(mu_=None), "mu_dev"), (dict(w_=None), "weights_dev"),
                       (dict(m_=None), "means_dev"), (dict(s_=None), "logvars_dev"), (dict(b_=None), "bound_dev"), (dict(u_=None), "n_used_dev")):
        assert fit(**kw) != 0, needle
        msg = L.avae_last_error(h).decode()
        assert "avae_gmm_fit" in msg and needle in msg, msg
    assert (bound == -7.0).all() and used.item() == -7 and np.array_equal(_bits(m), _bits(init["means"])), "outputs untouched"
    ll = torch.full((N,), -7.0, dtype=torch.float32, device=dev)

    def score(mu_=md, rows=N, K_=K, w_=w, m_=m, s_=s, ll_=ll):
        rc = L.avae_gmm_score(h, p(mu_), p(ld), rows, K_, p(w_), p(m_), p(s_), p(ll_), None, None, None)
        torch.cuda.synchronize()
        return rc
    for kw, needle in ((dict(rows=-1), "rows must be >= 0"), (dict(K_=0), "n_components = 0"), (dict(K_=65), "n_components = 65"),
                       (dict(mu_=None), "mu_dev"), (dict(w_=None), "weights_dev"), (dict(m_=None), "means_dev"),
                       (dict(s_=None), "logvars_dev"), (dict(ll_=None), "ll_dev, component_dev and resp_dev")):
        assert score(**kw) != 0, needle
        msg = L.avae_last_error(h).decode()
        assert "avae_gmm_score" in msg and needle in msg, msg
    assert (ll == -7.0).all()
    # rows = 0 with NULL data, and the handle still works
    assert fit(mu_=None, lv_=None, rows=0) == 0 and torch.isnan(bound).all() and used.item() == 0
    assert np.array_equal(_bits(m), _bits(init["means"]))
    assert score(mu_=None, rows=0) == 0 and (ll == -7.0).all()
    assert fit() == 0 and used.item() == N and torch.isfinite(bound).all() and score() == 0 and torch.isfinite(ll).all()


# ------------------------------------------------------------------------------------------------ 8. the Python surface
@pytest.mark.parametrize("nz", [7, 20])
def test_python_surface(V, nz):
    N, K = 48, 4
    model = _model(V, nz, fresh=True, ema=0.9)
    rng = np.random.default_rng(13)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    for i in range(3):
        model.partial_fit([x[:B] for x in X], rng.standard_normal((B, nz)).astype(np.float32))
    post = model.posterior(X)
    # NumPy in, NumPy out; tensors in, device tensors out, the same bits
    a = model.fit_latent_prior(post[0], n_components=K, n_iters=5, seed=3)
    assert isinstance(a["means"], np.ndarray) and isinstance(a["n_used"], int) and a["n_used"] == N and a["bound"].shape == (6,)
    t = model.fit_latent_prior(tuple(_dev(model, *post[0])), n_components=K, n_iters=5, seed=3)
    assert torch.is_tensor(t["means"]) and t["means"].is_cuda and t["bound"].dtype == torch.float64 and _same_fit(a, t)
    assert not np.array_equal(a["means"], model.fit_latent_prior(post[0], n_components=K, n_iters=5, seed=4)["means"])
    # the default start: K rows of mu, the data's total variance, weights 1 / K
    d = model.fit_latent_prior(post[0], n_components=K, n_iters=0, seed=3)
    rows = np.random.default_rng(3).permutation(N)[:K]
    assert np.array_equal(d["means"], post[0][0][rows]) and np.array_equal(d["weights"], np.full(K, 1 / K, np.float32))
    total = post[0][0].astype(np.float64).var(axis=0) + np.exp(post[0][1].astype(np.float64)).mean(axis=0)
    assert P.param_err(d["logvars"], np.tile(np.log(total), (K, 1))).max() < 1e-5
    # a list of two modalities' posteriors is the fit of the concatenation
    both = model.fit_latent_prior(post, n_components=K, n_iters=5)
    cat = model.fit_latent_prior((np.vstack([post[0][0], post[1][0]]), np.vstack([post[0][1], post[1][1]])), n_components=K, n_iters=5)
    assert both["n_used"] == 2 * N and _same_fit(both, cat)
    ref, b64, _ = P.fit64(np.vstack([post[0][0], post[1][0]]), np.vstack([post[0][1], post[1][1]]),
                          model.fit_latent_prior(post, n_components=K, n_iters=0), 5)
    assert max(P.prior_errs(both, ref, both["bound"], b64, nz)) < 1e-4
    assert np.all(np.diff(both["bound"]) > -1e-5)
    # scores
    sc = model.latent_prior_score(post[1], both)
    assert isinstance(sc["log_density"], np.ndarray) and sc["responsibilities"] is None and sc["component"].dtype == np.int32
    st = model.latent_prior_score(torch.from_numpy(post[1][0]).to(model.device), both, responsibilities=True)
    assert torch.is_tensor(st["log_density"]) and st["responsibilities"].shape == (N, K)
    assert P.ll_err(st["log_density"].cpu().numpy(), P.estep64(post[1][0], None, both)[0], nz).max() < 1e-5
    with pytest.raises(ValueError, match="n_components"):
        model.fit_latent_prior(post[0], n_components=65)
    with pytest.raises(ValueError, match="prior"):
        model.latent_prior_score(post[1], (both["means"], both["logvars"]))
    # samples: reproducible per seed, the mixture's frequencies and means, the decoders' shapes
    s1, s2, s3 = (model.sample_latent_prior(both, 20000, seed=s) for s in (5, 5, 6))
    assert isinstance(s1, np.ndarray) and s1.shape == (20000, nz) and s1.dtype == np.float32
    assert np.array_equal(s1, s2) and not np.array_equal(s1, s3)
    tight = {"weights": both["weights"], "means": (10.0 * np.arange(K)[:, None] * np.ones((1, nz))).astype(np.float32),
             "logvars": np.full((K, nz), -2.0, np.float32)}
    z = model.sample_latent_prior(tight, 20000, seed=1).astype(np.float64)
    comp = np.rint(z[:, 0] / 10.0).astype(int)                    # 10 apart, std 0.37: the component of a draw is plain
    w = tight["weights"].astype(np.float64) / tight["weights"].astype(np.float64).sum()
    for k in range(K):
        n_k = int((comp == k).sum())
        assert abs(n_k - 20000 * w[k]) <= 5.0 * np.sqrt(20000 * w[k] * (1 - w[k])) + 1e-9, (k, n_k, w[k])
        if n_k:
            assert np.abs(z[comp == k].mean(axis=0) - 10.0 * k).max() <= 5.0 * np.exp(-1.0) / np.sqrt(n_k), k
    ts = model.sample_latent_prior({k: torch.from_numpy(v).to(model.device) for k, v in tight.items()}, 7, seed=1)
    assert torch.is_tensor(ts) and ts.shape == (7, nz) and model.sample_latent_prior(tight, 0).shape == (0, nz)
    outs = model.generate(model.sample_latent_prior(both, 5))
    assert [o.shape for o in outs] == [(5, w_) for w_ in WIDTHS] and all(np.isfinite(o).all() for o in outs)
    # inside averaged(): given latents, the switch changes nothing
    with model.averaged():
        assert _same_fit(model.fit_latent_prior(post, n_components=K, n_iters=5), both)
        inner = model.latent_prior_score(post[1], both)
        avg_post = model.posterior(X)
        model.fit_latent_prior(avg_post, n_components=K, n_iters=2)
    assert np.array_equal(_bits(inner["log_density"]), _bits(sc["log_density"]))
    assert not np.array_equal(_bits(avg_post[0][0]), _bits(post[0][0]))


# ------------------------------------------------------------------------------------------------ 9. no side effects
def test_prior_calls_have_no_side_effects_on_training(V):
    nz = 20
    rng = np.random.default_rng(21)
    Xt = synth_batch(rng, 2 * B, WIDTHS, [True, False])
    et = rng.standard_normal((2 * B, nz)).astype(np.float32)
    mu, lv, _ = P.clusters(rng, 1100, nz, 4, 3.0)
    state = lambda m: m.get_opt_state() + (m.get_params(), m.cost_history(1))
    runs = []
    for with_calls in (False, True):
        model = _model(V, nz, fresh=True)
        model.partial_fit([x[:B] for x in Xt], et[:B])
        before = state(model)
        if with_calls:
            prior = model.fit_latent_prior((mu, lv), n_components=5, n_iters=4)
            model.latent_prior_score((mu, lv), prior, responsibilities=True)
            model.generate(model.sample_latent_prior(prior, 5))
            model.synchronize()
            for x, y in zip(before, state(model)):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        cost = model.partial_fit([x[B:] for x in Xt], et[B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append((np.float32(cost), model.get_grads()) + state(model))
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x), np.asarray(y))
