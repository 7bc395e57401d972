"""The definition of ``impute`` (tests/impute_reference.py) checked without a GPU: the fusion rule against its naive form, its
range, the stationarity of sum_m KL(q || q_m) at the fused Gaussian, the select and prior cases, the float32 Welford update
against two fp64 passes on the GPU tests' own inputs, and the Python argument checks."""
import numpy as np
import pytest

import impute_reference as R

U32 = 2.0 ** -24


def _posteriors(rng, M, N, nz, spread=1.0):
    return rng.standard_normal((M, N, nz)), spread * rng.standard_normal((M, N, nz))


def test_shifted_fusion_equals_naive_form():
    rng = np.random.default_rng(0)
    mu, lv = _posteriors(rng, 3, 64, 20, 2.0)
    p = R.pattern_rows(64, 3)
    some = p.any(1)
    a, b = R.fuse(mu, lv, p)
    na, nb = R.fuse_naive(mu, lv, p)
    many = p.sum(1) > 1
    assert np.abs(a[many] - na[many]).max() <= 1e-13 * np.abs(na[many]).max()
    assert np.abs(b[many] - nb[many]).max() <= 1e-13 * max(1.0, np.abs(nb[many]).max())
    assert np.allclose(a[some], na[some], rtol=1e-12, atol=1e-13) and np.allclose(b[some], nb[some], rtol=1e-12, atol=1e-13)


def test_fusion_stays_finite_where_the_naive_float32_form_does_not():
    rng = np.random.default_rng(1)
    N, nz = 8, 7
    mu = rng.standard_normal((2, N, nz)).astype(np.float32)
    p = np.ones((N, 2), bool)
    for lv0, lv1 in ((80.0, 80.0), (-80.0, -80.0), (80.0, -80.0), (-80.0, 79.0)):
        lv = np.stack([np.full((N, nz), lv0, np.float32), np.full((N, nz), lv1, np.float32)])
        a, b = R.fuse(mu, lv, p)
        assert a.dtype == np.float32 and np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (lv0, lv1)
        a64, b64 = R.fuse(mu.astype(np.float64), lv.astype(np.float64), p)
        assert np.abs(a - a64).max() <= 1e-5 * max(1.0, np.abs(a64).max()) and np.abs(b - b64).max() <= 1e-5 * np.abs(b64).max()
    with np.errstate(all="ignore"):
        na, nb = R.fuse_naive(mu, np.full((2, N, nz), 80.0, np.float32), p)            # exp(-80) underflows float32's normal range
        na2, nb2 = R.fuse_naive(mu, np.full((2, N, nz), -100.0, np.float32), p)        # exp(100) overflows
    assert not (np.all(np.isfinite(na2)) and np.all(np.isfinite(nb2)))
    a, b = R.fuse(mu, np.full((2, N, nz), -100.0, np.float32), p)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))


def test_fused_gaussian_is_a_stationary_point_and_a_minimum():
    rng = np.random.default_rng(2)
    for M in (2, 3):
        mu, lv = _posteriors(rng, M, 16, 12, 0.7)
        p = np.ones((16, M), bool)
        a, b = R.fuse(mu, lv, p)
        for n in range(16):
            g_mu, g_s = R.kl_sum_grad(a[n], b[n], mu[:, n], lv[:, n])
            assert np.abs(g_mu).max() <= 1e-12 and np.abs(g_s).max() <= 1e-12, (M, n, np.abs(g_mu).max(), np.abs(g_s).max())
            base = R.kl_sum(a[n], b[n], mu[:, n], lv[:, n])
            for scale in (1e-3, 1e-1, 1.0):
                for _ in range(8):
                    d_mu, d_s = scale * rng.standard_normal(12), scale * rng.standard_normal(12)
                    assert R.kl_sum(a[n] + d_mu, b[n] + d_s, mu[:, n], lv[:, n]) > base


def test_identical_posteriors_fuse_to_themselves():
    rng = np.random.default_rng(3)
    mu1, lv1 = _posteriors(rng, 1, 10, 20)
    for M in (2, 3, 4):
        a, b = R.fuse(np.repeat(mu1, M, 0), np.repeat(lv1, M, 0), np.ones((10, M), bool))
        assert np.abs(a - mu1[0]).max() <= 1e-15 * np.abs(mu1).max() + 1e-16 and np.abs(b - lv1[0]).max() <= 1e-15 * max(1, np.abs(lv1).max())


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_modality_is_a_select_and_none_is_the_prior(dt):
    rng = np.random.default_rng(4)
    mu, lv = (a.astype(dt) for a in _posteriors(rng, 3, 24, 7, 3.0))
    lv[1, 3, 2] = 0.0
    p = R.pattern_rows(24, 3)
    dirty_mu, dirty_lv = mu.copy(), lv.copy()
    for m in range(3):
        dirty_mu[m][~p[:, m]] = np.nan
        dirty_lv[m][~p[:, m]] = np.inf
    a, b = R.fuse(dirty_mu, dirty_lv, p)                                               # absent posteriors are never used
    a2, b2 = R.fuse(mu, lv, p)
    assert np.array_equal(a.view(np.uint8), a2.view(np.uint8)) and np.array_equal(b.view(np.uint8), b2.view(np.uint8))
    for m in range(3):
        only = p[:, m] & (p.sum(1) == 1)
        assert only.any()
        assert np.array_equal(a[only].view(np.uint8), mu[m][only].view(np.uint8))
        assert np.array_equal(b[only].view(np.uint8), lv[m][only].view(np.uint8))
    none = ~p.any(1)
    assert none.any() and not a[none].view(np.uint8).any() and not b[none].view(np.uint8).any()      # +0.0 exactly


def test_welford_on_equal_values_is_exact_and_one_sample_has_no_variance():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 1, 50)).astype(np.float32)
    m1, v1 = R.welford32(x)
    assert np.array_equal(m1, x[:, 0]) and not v1.view(np.uint32).any()
    m3, v3 = R.welford32(np.repeat(x, 3, 1))
    assert np.array_equal(m3, x[:, 0]) and not v3.view(np.uint32).any()


# (n_z, three modalities, N, K): the cases of tests/test_gpu_impute.py::test_sampled_mean_and_variance
SAMPLED = [(20, True, 19, 5), (7, False, 15, 16), (64, False, 1, 40), (20, False, 19, 40), (7, True, 15, 5), (20, False, 2, 300)]


@pytest.mark.parametrize("nz,three,N,K", SAMPLED)
def test_float32_welford_equals_two_fp64_passes_on_the_gpu_tests_inputs(nz, three, N, K):
    """The decoded samples of the fp64 definition, rounded to float32 as the kernels see them: the sequential float32 update
    against two fp64 passes.  Bounds from the update's roundings, X = max |x|: every step rounds delta, the quotient and the sum
    (<= 4 u X on the mean, K steps), and the M2 addend delta * (x - mean) <= (2X)^2 with three roundings plus the carried mean
    error (<= 4 K u X) in both factors: |var error| <= (16 + 16 K) u X^2."""
    archs, X, p, eps = R.case(nz, three, N, K, seed=100 + K)
    ref = R.oracle_for(archs, three, "relu", 16, R.init_flat(archs, 5))
    r = R.ref_impute(ref, X, p, K, eps)
    for d, x in enumerate(r["samples"]):
        x32 = x.astype(np.float32)
        m64, v64 = R.two_pass(x32)
        m32, v32 = R.welford32(x32)
        Xm = np.abs(x32).max()
        em, ev = np.abs(m32 - m64).max(), np.abs(v32 - v64).max()
        print("nz=%d K=%d modality %d: mean err %.3e (bound %.3e), var err %.3e (bound %.3e)"
              % (nz, K, d, em, 4 * K * U32 * Xm, ev, (16 + 16 * K) * U32 * Xm * Xm))
        assert em <= 4 * K * U32 * Xm and ev <= (16 + 16 * K) * U32 * Xm * Xm
        assert np.allclose(r["mean"][d], m64, rtol=0, atol=1e-6 * Xm) and np.all(v32 >= 0)


def test_reference_routes_agree():
    """n_samples = 0 decodes mu; eps = 0 samples give the same mean and no variance; None and an all-absent column agree."""
    archs, X, p, _ = R.case(20, True, 11, 0, seed=3)
    ref = R.oracle_for(archs, True, "relu", 16, R.init_flat(archs, 5))
    r0 = R.ref_impute(ref, X, p, 0)
    r3 = R.ref_impute(ref, X, p, 3, np.zeros((11, 3, 20)))
    for d in range(3):
        assert np.allclose(r3["mean"][d], r0["mean"][d], rtol=1e-14, atol=1e-15) and np.abs(r3["var"][d]).max() <= 1e-28
    p1 = p.copy()
    p1[:, 2] = False
    a, b = R.ref_impute(ref, X, p1, 0), R.ref_impute(ref, [X[0], X[1], None], p, 0)
    assert np.array_equal(a["mu"], b["mu"]) and all(np.array_equal(x, y) for x, y in zip(a["mean"], b["mean"]))
    prior = ~p.any(1)
    assert prior.any() and not np.any(r0["mu"][prior]) and not np.any(r0["logvar"][prior])


def test_python_argument_checks_need_no_device():
    from vae_assoc_amd.vae_assoc import impute_args
    widths, nz = [784, 147], 20
    rng = np.random.default_rng(0)
    X = [rng.random((9, 784)).astype(np.float32), rng.standard_normal((9, 147)).astype(np.float32)]
    args = lambda *a, **k: impute_args(*a, widths=widths, n_z=nz, device="cpu", **k)
    ts, rows, was_np, ptrs, lds, p, K, e = args(X, None, 0, None)
    assert rows == 9 and was_np and p is None and K == 0 and e is None
    ts, rows, was_np, ptrs, lds, p, K, e = args([None, X[1]], None, 4, np.zeros((9, 4, 20)))
    assert rows == 9 and ts[0] is None and ptrs[0] is None and lds[0] == 0 and tuple(e.shape) == (9, 4, 20)
    ts, rows, was_np, ptrs, lds, p, K, e = args([None, None], np.ones((5, 2)), 2, None)
    assert rows == 5 and was_np and p.dtype.is_floating_point is False and tuple(p.shape) == (5, 2)
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="n_samples"):
            args(X, None, bad, None)
    with pytest.raises(ValueError):
        args([None, None], None, 0, None)                                              # no row count
    with pytest.raises(ValueError):
        args([X[0]], None, 0, None)                                                    # one modality short
    with pytest.raises(ValueError):
        args([X[0], X[1][:8]], None, 0, None)                                          # row counts disagree
    with pytest.raises(ValueError):
        args([X[0], X[1][:, :100]], None, 0, None)                                     # wrong width
    with pytest.raises(ValueError):
        args(X, np.ones((9, 3)), 0, None)                                              # presence width != M
    with pytest.raises(ValueError):
        args(X, np.ones((8, 2)), 0, None)                                              # presence rows != X rows
    with pytest.raises(ValueError):
        args(X, None, 4, np.zeros((9, 20)))                                            # eps rank
    with pytest.raises(ValueError):
        args(X, None, 4, np.zeros((9, 3, 20)))                                         # eps K
    with pytest.raises(ValueError):
        args(X, None, 0, np.zeros((9, 1, 20)))                                         # eps without samples
