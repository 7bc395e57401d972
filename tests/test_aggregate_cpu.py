"""The aggregate-posterior log-density checked without a GPU: the definitions of tests/aggregate_reference.py against a brute-force
double loop and against closed forms, the float32 restatement's own error, the ELBO decomposition identity, the Python argument
checks, the two new symbols, and avae_agg_logpdf_plan (host-only): the gallery partition is a function of gallery_rows alone, no
slice is empty, and the scratch stays bounded however many queries there are."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import aggregate_reference as A
from conftest import ROOT


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def test_reference_against_a_brute_force_double_loop():
    rng = np.random.default_rng(0)
    N, G, nz = 3, 4, 2
    g = A.latents(rng, G, nz)
    z = A.queries(rng, g, N)
    for exclude in (None, [1, -1, 4], [0, 3, 2]):
        joint, marginal = A.logpdf64(z, g, exclude)
        for n in range(N):
            rows = [r for r in range(G) if exclude is None or r != exclude[n]]
            dens, dens_j = 0.0, [0.0] * nz
            for r in rows:
                p = 1.0
                for j in range(nz):
                    var = math.exp(float(g[1][r, j]))
                    pj = math.exp(-0.5 * (float(z[n, j]) - float(g[0][r, j])) ** 2 / var) / math.sqrt(2.0 * math.pi * var)
                    dens_j[j] += pj / len(rows)
                    p *= pj
                dens += p / len(rows)
            assert abs(joint[n] - math.log(dens)) <= 1e-12 * (abs(math.log(dens)) + nz), (exclude, n)
            for j in range(nz):
                assert abs(marginal[n, j] - math.log(dens_j[j])) <= 1e-12 * (abs(math.log(dens_j[j])) + 1), (exclude, n, j)


def test_identical_standard_normal_rows_give_the_normal_density():
    rng = np.random.default_rng(1)
    for nz in (7, 20, 64):
        z = (3.0 * rng.standard_normal((19, nz))).astype(np.float32)
        g = (np.zeros((33, nz), np.float32), np.zeros((33, nz), np.float32))
        want = (-0.5 * z.astype(np.float64) ** 2 - A.C)
        for exclude in (None, np.arange(19)):
            joint, marginal = A.logpdf64(z, g, exclude)
            assert np.abs(joint - want.sum(1)).max() <= 1e-12 * np.abs(want.sum(1)).max()
            assert np.abs(joint - marginal.sum(1)).max() <= 1e-12 * np.abs(joint).max()
            assert np.abs(marginal - want).max() <= 1e-12 * (np.abs(want).max() + 1)


def test_edges_of_the_definition():
    rng = np.random.default_rng(2)
    nz = 5
    g = A.latents(rng, 6, nz)
    z = A.queries(rng, g, 4)
    clean = A.logpdf64(z, g)
    for fn in (A.logpdf64, A.logpdf32):
        # an empty mixture is NaN; a single excluded row too
        j, m = fn(z, (g[0][:0], g[1][:0]))
        assert np.isnan(j).all() and np.isnan(m).all() and m.shape == (4, nz)
        j, m = fn(z, (g[0][:1], g[1][:1]), [0, 0, -1, 1])
        assert np.isnan(j[:2]).all() and np.isfinite(j[2:]).all() and np.isnan(m[:2]).all() and np.isfinite(m[2:]).all()
        # a query whose every exponent overflows to -Inf has density 0, not NaN
        far = z.astype(np.float64)
        far[1] = 1e30 if fn is A.logpdf32 else 1e200
        j, m = fn(far, g)
        assert np.isneginf(j[1]) and np.isneginf(m[1]).all() and np.isfinite(j[[0, 2, 3]]).all()
        # lv = +Inf contributes nothing: the density of the other rows times (G - 1) / G
        wide = (g[0], g[1].copy())
        wide[1][2] = np.inf
        j, m = fn(z, wide)
        rest = A.logpdf64(z, (np.delete(g[0], 2, 0), np.delete(g[1], 2, 0)))
        assert np.abs(j - (rest[0] + np.log(5 / 6))).max() < 1e-5 and np.abs(m - (rest[1] + np.log(5 / 6))).max() < 1e-5
        # an excluded row is selected away whatever it holds
        bad = (g[0].copy(), g[1].copy())
        bad[0][3], bad[1][3, 0] = np.nan, np.inf
        j, m = fn(z, bad, [3, 3, 3, 0])
        want = fn(z, g, [3, 3, 3, 0])
        assert np.array_equal(j[:3], want[0][:3]) and np.array_equal(m[:3], want[1][:3]) and np.isnan(j[3]) and np.isnan(m[3]).all()
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()


def test_float32_restatement_is_close_to_the_definition():
    """the figures every GPU bound is a multiple of: N = 19 standard queries, G = 64"""
    for nz in (7, 20, 64):
        rng = np.random.default_rng(100 + nz)
        g = A.latents(rng, 64, nz)
        z = A.queries(rng, g)
        ref, own = A.logpdf64(z, g), A.logpdf32(z, g)
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
        ej, em = A.joint_err(own[0], ref[0], nz).max(), A.marginal_err(own[1], ref[1]).max()
        print("n_z=%d: float32 restatement worst error joint %.2e marginal %.2e" % (nz, ej, em))
        assert ej < 2e-6 and em < 2e-6, (nz, ej, em)


def test_decomposition_identity():
    rng = np.random.default_rng(3)
    N, nz, S = 23, 6, 3
    posts = [A.latents(rng, N, nz), None, A.latents(rng, N, nz)]
    eps = rng.standard_normal((S, N, nz))
    for loo in (False, True):
        r = A.decomposition64(posts, eps, leave_one_out=loo)
        for m in (0, 2):
            terms = [r["mi"][m], r["tc"][m]] + list(r["dimwise_kl"][m])
            assert abs(r["kl"][m] - sum(terms)) <= 1e-10 * sum(abs(t) for t in terms), (loo, m)
            assert abs(r["marginal_kl"][m] - (r["tc"][m] + r["dimwise_kl"][m].sum())) <= 1e-12 * abs(r["marginal_kl"][m])
            assert r["cross"][m, m] == 0.0 and np.isfinite(r["cross"][m, 2 - m])
        assert np.isnan(r["kl"][1]) and np.isnan(r["cross"][1]).all() and np.isnan(r["cross"][:, 1]).all()
        assert r["log_n"] == np.log(N)
        if not loo:
            assert np.all(r["mi"][[0, 2]] <= r["log_n"] + 1e-12)                  # the own posterior is in the mixture: mi <= log N
    # kl is the closed-form KL to the prior in expectation: the sample mean of many draws is close to it
    eps = rng.standard_normal((400, N, nz))
    r = A.decomposition64(posts[:1], eps)
    mu, lv = (a.astype(np.float64) for a in posts[0])
    closed = 0.5 * (mu ** 2 + np.exp(lv) - lv - 1.0).sum(1).mean()
    assert abs(r["kl"][0] - closed) < 0.02 * closed


def test_python_argument_checks_need_no_device():
    import torch
    from vae_assoc_amd.vae_assoc import agg_args
    nz = 20
    rng = np.random.default_rng(0)
    g = A.latents(rng, 31, nz)
    z = A.queries(rng, g, 9)
    args = lambda *a, **kw: agg_args(*a, n_z=nz, device="cpu", **kw)
    zt, gm, gl, ex, marg, was_np = args(z, g, None, True)
    assert tuple(zt.shape) == (9, nz) and tuple(gl.shape) == (31, nz) and ex is None and marg is True and was_np
    assert zt.dtype == torch.float32 and zt.is_contiguous()
    zt, gm, gl, ex, marg, was_np = args(torch.from_numpy(z), list(g), np.arange(9), 0)
    assert ex.dtype == torch.int32 and ex.tolist() == list(range(9)) and marg is False and not was_np
    ex = args(z, g, torch.tensor([-5, 2 ** 40, 3, 0, 0, 0, 0, 0, 30]), True)[3]
    assert ex.tolist() == [-1, 2 ** 31 - 1, 3, 0, 0, 0, 0, 0, 30]               # outside the gallery: excludes nothing
    zt, gm, gl, ex, _, _ = args(z[:0], (g[0][:0], g[1][:0]), np.zeros(0, np.int64), True)
    assert zt.shape[0] == 0 and gm.shape[0] == 0 and ex.shape[0] == 0
    with pytest.raises(ValueError, match="z is None"):
        args(None, g, None, True)
    with pytest.raises(ValueError, match="pair"):
        args(z, g[0], None, True)
    with pytest.raises(ValueError, match="pair"):
        args(z, (g[0], g[1], g[1]), None, True)
    with pytest.raises(ValueError, match="gallery: logvar is None"):
        args(z, (g[0], None), None, True)
    with pytest.raises(ValueError, match="gallery: mu is None"):
        args(z, (None, g[1]), None, True)
    with pytest.raises(ValueError, match=r"expected a \[rows, 20\]"):
        args(z[:, :19], g, None, True)                                           # wrong width
    with pytest.raises(ValueError, match="gallery"):
        args(z, (g[0][:, :7], g[1][:, :7]), None, True)
    with pytest.raises(ValueError, match="gallery"):
        args(z, (g[0], g[1][:30]), None, True)                                   # logvar rows != mu rows
    with pytest.raises(ValueError, match="expected"):
        args(z[0], g, None, True)                                                # one row must still be [1, n_z]
    with pytest.raises(ValueError, match="integers"):
        args(z, g, np.arange(9, dtype=np.float32), True)
    with pytest.raises(ValueError, match="integers"):
        args(z, g, torch.zeros(9, dtype=torch.bool), True)
    with pytest.raises(ValueError, match=r"exclude must be \[9\]"):
        args(z, g, np.arange(8), True)
    with pytest.raises(ValueError, match=r"exclude must be \[9\]"):
        args(z, g, np.zeros((9, 1), np.int32), True)


def test_header_declares_and_library_exports_both_symbols(capi):
    txt = open(os.path.join(ROOT, "include", "avae.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = capi.lib()
    for name in ("avae_agg_logpdf", "avae_agg_logpdf_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in capi.SYMBOLS


def _config(capi, n_z=20):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = 2
    for m, (n_in, h) in enumerate(((784, 96), (147, 72))):
        cfg.mod[m].n_input = n_in
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = h
        cfg.mod[m].binary = 1 - m
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = n_z, 16, 1, 0
    cfg.learning_rate, cfg.assoc_lambda = 1e-3, 1.0
    return cfg


def _plan(capi, rows, G, n_z=20):
    """-> (query_tile, chunk_rows, slice_rows, n_slices, scratch_bytes)"""
    qt, ch, sr, ns, sb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    rc = capi.lib().avae_agg_logpdf_plan(C.byref(_config(capi, n_z)), rows, G, C.byref(qt), C.byref(ch), C.byref(sr), C.byref(ns),
                                         C.byref(sb))
    assert rc == 0, capi.lib().avae_last_error(None)
    return qt.value, ch.value, sr.value, ns.value, sb.value


GALLERIES = [1, 63, 64, 65, 1024, 1025, 2100, 4099, 65535, 65536, 65537, 70000, 10 ** 6, 2 ** 31 - 1]


@pytest.mark.parametrize("G", GALLERIES)
def test_plan_slices_cover_the_gallery_and_do_not_depend_on_rows(capi, G):
    seen = set()
    for rows in (0, 1, 19, 64, 65, 2048, 2049, 20000, 2 ** 31 - 1):
        for n_z in (7, 64):
            qt, ch, sr, ns, sb = _plan(capi, rows, G, n_z)
            assert qt == 64 and ch == min(rows, 2048)
            assert sr >= 1024 and sr % 64 == 0 and 1 <= ns <= 64
            assert (ns - 1) * sr < G <= ns * sr                                  # the slices cover the gallery, the last is not empty
            assert sb == ch * ns * (1 + n_z) * 8 and sb <= 68157440
            seen.add((sr, ns))
    assert len(seen) == 1                                                        # a function of gallery_rows alone


def test_plan_figures_the_gpu_tests_rely_on(capi):
    assert _plan(capi, 7, 0)[3:] == (0, 0)                                       # an empty gallery: no slice, no scratch
    assert _plan(capi, 0, 100)[4] == 0
    assert _plan(capi, 130, 1025)[2:4] == (1024, 2)                              # a second slice of one row
    assert _plan(capi, 130, 2100)[2:4] == (1024, 3)
    assert _plan(capi, 3, 65537)[2:4] == (1088, 61)                              # several slices of more than 1024 rows
    assert _plan(capi, 3, 65536)[2:4] == (1024, 64)
    assert _plan(capi, 2 ** 31 - 1, 2 ** 31 - 1, 64)[4] == 68157440
    assert _plan(capi, 2049, 70, 7)[1] == 2048


def test_plan_errors(capi):
    L = capi.lib()
    cfg = _config(capi)
    out = C.c_int32(0)
    for rows, G, needle in ((-1, 1, "rows"), (1, -1, "gallery_rows"), (-2 ** 31, 5, "rows")):
        assert L.avae_agg_logpdf_plan(C.byref(cfg), rows, G, C.byref(out), None, None, None, None) != 0
        assert needle in L.avae_last_error(None).decode(), (rows, G)
    assert L.avae_agg_logpdf_plan(None, 1, 1, None, None, None, None, None) != 0
    bad = _config(capi)
    bad.n_z = 65
    assert L.avae_agg_logpdf_plan(C.byref(bad), 1, 1, None, None, None, None, None) != 0 and "n_z" in L.avae_last_error(None).decode()
    assert L.avae_agg_logpdf_plan(C.byref(cfg), 5, 7, None, None, None, None, None) == 0          # every output is optional
