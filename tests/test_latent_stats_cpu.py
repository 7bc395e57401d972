"""Posterior diagnostics checked without a GPU: the float64 definition (tests/latent_stats_reference.py) against np.var / np.cov on
complete data and against a brute-force loop on masked data, what the float32 restatement and a float32 raw-moment pass are
worth on the tests' input families, avae_latent_stats_plan (host-only), and the Python argument checks."""
import ctypes as C

import numpy as np
import pytest

import latent_stats_reference as R


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def test_definition_equals_numpy_on_complete_data():
    rng = np.random.default_rng(0)
    for nz in (7, 20):
        post = R.family(rng, "A", 300, nz, n_mod=3)
        st = R.stats64(post)
        assert (st["count"] == 300).all()
        for s in range(3):
            x = post[s][0].astype(np.float64)
            assert np.allclose(st["cov"][s], np.cov(x.T, bias=True), rtol=1e-12, atol=1e-15)
            assert np.allclose(st["post_var"][s], np.exp(post[s][1].astype(np.float64)).mean(0), rtol=1e-13)
            for d in range(3):
                y = post[d][0].astype(np.float64)
                assert np.allclose(st["mean"][s, d], x.mean(0), rtol=1e-13, atol=1e-16)
                assert np.allclose(st["var"][s, d], np.var(x, axis=0), rtol=1e-12)
                assert np.allclose(st["xcov"][s, d], ((x - x.mean(0)) * (y - y.mean(0))).mean(0), rtol=1e-12, atol=1e-15)
            assert np.array_equal(st["xcov"][s, s], st["var"][s, s]) and not st["assoc"][s, s].any()
            assert np.allclose(np.diagonal(st["cov"][s]), st["var"][s, s], rtol=1e-12)
        assert np.array_equal(st["assoc"][0, 1], st["assoc"][1, 0]) and np.all(st["assoc"] >= 0) and np.all(st["kl"] >= 0)


def test_definition_equals_a_brute_force_loop_on_masked_data():
    rng = np.random.default_rng(1)
    rows, nz = 23, 5
    post = R.family(rng, "B", rows, nz, n_mod=4)
    post[3] = None
    present = rng.random((rows, 4)) < 0.6
    present[:, 2] = False
    present[4, 2] = True                                             # one row of modality 2 ...
    present[4, 1] = False                                            # ... which modality 1 lacks: the pair (1, 2) is empty
    for m in range(3):                                               # absent entries are never read
        post[m][0][~present[:, m]] = np.nan
        post[m][1][~present[:, m]] = np.nan
    a, b = R.stats64(post, present), R.brute64(post, present)
    assert np.array_equal(a["count"], b["count"])
    assert a["count"][2, 2] == 1 and a["count"][1, 2] == 0 and not a["count"][3].any() and not a["count"][:, 3].any()
    for k in R.NAMES[1:]:
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        assert np.allclose(a[k], b[k], rtol=1e-9, atol=1e-12, equal_nan=True), k
    assert np.isnan(a["mean"][1, 2]).all() and np.isnan(a["cov"][3]).all() and np.isnan(a["kl"][3]).all()
    assert not a["var"][2, 2].any() and not a["cov"][2].any() and np.array_equal(a["mean"][2, 2], post[2][0][4].astype(np.float64))
    assert all(v == 0.0 for v in R.errors(a, a).values())


@pytest.mark.parametrize("nz", R.NZS)
def test_float32_restatement_is_sound_and_a_raw_moment_pass_is_not(nz):
    """What the GPU tests' bound (4 x the restatement's worst error, tests/test_gpu_latent_stats.py) is worth.  The restatement's
    variance is within 2.5e-3 of the true one, relative, on every case of 65 rows and more (measured worst: 2.1e-3, family B, 4099
    rows, n_z = 64).  On two rows of families B and C it can be off by the whole variance: two values a few float32 spacings
    apart have a float32 mean that IS one of them (measured: 1.0 at n_z = 20 and 64).  A raw-moment float32 variance is off by
    0.2 and more in its worst column on every case of families B and C with two rows and more, by more than 1e5 at 4099."""
    raw_worst = 0.0
    for name in R.FAMILIES:
        for rows in R.ROWS:
            post, ref, err = R.case(name, rows, nz)
            assert np.isfinite(list(err.values())).all()
            if rows == 1:
                assert err["var"] == 0.0 and err["cov"] == 0.0 and err["mean"] == 0.0
            if rows >= 65:
                assert err["var"] <= 2.5e-3 and err["cov"] <= 2.5e-3, (name, rows, err)
            if name != "A" and rows >= 2:
                with np.errstate(all="ignore"):
                    raw = max((np.abs(R.raw_var32(post[m][0]) - ref["var"][m, m]) / ref["var"][m, m]).max() for m in range(2))
                assert raw >= 0.2, (name, rows, raw)
                raw_worst = max(raw_worst, raw)
    assert raw_worst > 1e5
    tol, worst = R.bound(nz)
    assert all(tol[k] == 4.0 * worst[k] for k in tol) and all(0 < worst[k] <= 1.0 for k in worst)
    assert max(worst[k] for k in ("mean", "assoc", "post_var", "kl")) < 2e-4


def _config(capi, n_z=20, n_mod=2):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = n_mod
    for m in range(n_mod):
        cfg.mod[m].n_input = 147
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = 72
        cfg.mod[m].binary = 0
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = n_z, 16, 1, 0
    cfg.learning_rate, cfg.assoc_lambda = 1e-3, 1.0
    return cfg


def _plan(capi, rows, n_z=20, n_mod=2):
    rt, ns, sb = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    rc = capi.lib().avae_latent_stats_plan(C.byref(_config(capi, n_z, n_mod)), rows, C.byref(rt), C.byref(ns), C.byref(sb))
    assert rc == 0, capi.lib().avae_last_error(None)
    return rt.value, ns.value, sb.value


SCRATCH_BOUND = 42487808                                             # include/avae.h: 256 slices, 4 modalities, n_z = 64


@pytest.mark.parametrize("rows", [1, 2, 65, 255, 256, 257, 4099, 20000, 65536, 65537, 1048576, 2 ** 31 - 1])
def test_plan_slices_cover_the_rows_exactly(capi, rows):
    rt, ns, sb = _plan(capi, rows)
    assert rt >= 1 and 1 <= ns <= 256
    assert (ns - 1) * rt < rows <= ns * rt                           # every row in exactly one slice, the last slice not empty
    if ns < 2 ** 16:
        sl = R.plan_slices(rows, rt, ns)
        assert sl[0][0] == 0 and sl[-1][1] == rows and all(a < b for a, b in sl) and all(x[1] == y[0] for x, y in zip(sl, sl[1:]))
    # a function of rows alone; the scratch is the layout the header states, within its bound
    for n_z, n_mod in ((7, 1), (20, 2), (64, 4)):
        rt2, ns2, sb2 = _plan(capi, rows, n_z, n_mod)
        assert (rt2, ns2) == (rt, ns)
        assert sb2 == ns * (n_mod * (1 + 5 * n_z + n_z * n_z) + n_mod * (n_mod - 1) // 2 * (1 + 8 * n_z)) * 8 <= SCRATCH_BOUND


def test_plan_edges_and_errors(capi):
    L = capi.lib()
    assert _plan(capi, 0)[1:] == (0, 0)                              # no slice, no scratch -- and only for rows == 0
    assert _plan(capi, 2 ** 31 - 1, 64, 4)[1:] == (256, SCRATCH_BOUND)
    # tests/test_gpu_latent_stats.py relies on these: several slices, the last one ragged
    for rows in (4099, 20000):
        rt, ns, _ = _plan(capi, rows)
        assert ns >= 3 and rows % rt != 0
    assert _plan(capi, 65)[1] == 1
    cfg = _config(capi)
    assert L.avae_latent_stats_plan(C.byref(cfg), -1, None, None, None) != 0 and "rows" in L.avae_last_error(None).decode()
    assert L.avae_latent_stats_plan(None, 1, None, None, None) != 0
    bad = _config(capi)
    bad.n_z = 65
    assert L.avae_latent_stats_plan(C.byref(bad), 1, None, None, None) != 0 and "n_z" in L.avae_last_error(None).decode()
    assert L.avae_latent_stats_plan(C.byref(cfg), 5, None, None, None) == 0                      # every output is optional


def test_python_argument_checks_need_no_device():
    import torch
    from vae_assoc_amd.vae_assoc import latent_stats_args
    nz = 20
    rng = np.random.default_rng(0)
    post = R.family(rng, "A", 9, nz, n_mod=3)
    args = lambda *a: latent_stats_args(*a, n_z=nz, device="cpu")
    mus, lvs, rows, p, was_np = args(post, None)
    assert len(mus) == 3 and rows == 9 and p is None and was_np and mus[0].dtype == torch.float32 and mus[2].is_contiguous()
    flags = rng.random((9, 3)) < 0.5
    mus, lvs, rows, p, was_np = args([post[0], None, tuple(torch.from_numpy(a) for a in post[2])], flags)
    assert mus[1] is None and lvs[1] is None and p.dtype == torch.uint8 and tuple(p.shape) == (9, 3) and was_np
    mus, lvs, rows, p, was_np = args([None, None], torch.ones((4, 2), dtype=torch.bool))
    assert rows == 4 and mus == [None, None] and not was_np
    assert args([(post[0][0][:0], post[0][1][:0])], None)[2] == 0                                 # no row at all is fine
    with pytest.raises(ValueError, match=r"posteriors\[1\].*\[rows, 20\]|posteriors\[1\].*20"):
        args([post[0], (post[1][0][:, :19], post[1][1][:, :19])], None)                          # a wrong n_z
    with pytest.raises(ValueError, match=r"posteriors\[1\]"):
        args([post[0], (post[1][0][:8], post[1][1][:8])], None)                                  # mismatched row counts
    with pytest.raises(ValueError, match=r"posteriors\[0\].*logvar"):
        args([(post[0][0], post[0][1][:8])], None)
    with pytest.raises(ValueError, match="present"):
        args(post, flags[:, :2])                                                                 # a present of the wrong shape
    with pytest.raises(ValueError, match=r"posteriors\[0\]"):
        args(post, flags[:8])                                                                    # ... or of other rows
    with pytest.raises(ValueError, match="logvar is None"):
        args([(post[0][0], None)], None)                                                         # a mu without a logvar
    with pytest.raises(ValueError, match="mu is None"):
        args([(None, post[0][1])], None)
    with pytest.raises(ValueError, match="pair"):
        args([post[0][0]], None)
    with pytest.raises(ValueError, match="1 to 4"):
        args([], None)
    with pytest.raises(ValueError, match="1 to 4"):
        args([post[0]] * 5, None)
    with pytest.raises(ValueError, match="row count"):
        args([None, None], None)
