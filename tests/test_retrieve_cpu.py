"""Cross-modal retrieval checked without a GPU: the definition of the distance (tests/retrieve_reference.py) against the
reference's two-KL formula, the exact zero of identical rows, the total order of a result, the Python argument checks, the two
new symbols, and avae_latent_topk_plan (host-only): its tiles cover rows x gallery_rows exactly, few queries split the gallery, and
the scratch stays bounded however many queries there are."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retrieve_reference as R
from conftest import ROOT


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def test_definition_equals_the_two_kl_formula():
    rng = np.random.default_rng(0)
    for nz in (7, 20, 64):
        q, g = R.latents(rng, 19, nz), R.latents(rng, 33, nz)
        a, b = R.dist64(q, g, "symkl"), R.two_kl64(q, g)
        # the two-KL form cancels "- n_z" against its other addends: its own rounding error is relative to value + n_z
        assert np.abs(a - b).max() <= 1e-12 * (np.abs(b).max() + nz), nz
        assert np.all(np.abs(a - b) <= 1e-12 * (b + nz))
        assert np.all(a >= 0)


def test_identical_rows_are_exactly_zero_and_every_addend_is_non_negative():
    rng = np.random.default_rng(1)
    q = R.latents(rng, 12, 20)
    for metric in R.METRICS:
        for fn in (R.dist64, R.dist32):
            D = fn(q, q, metric)
            assert not np.diag(D).copy().view(np.uint8).any(), (metric, fn.__name__)          # +0.0, not -0.0, not 1e-17
            assert np.all(D >= 0)
    # where the two-KL form in float32 cancels, the definition does not: nearest neighbours keep their relative accuracy
    near = (q[0] + np.float32(1e-3), q[1])
    a32, a64 = R.dist32(q, near, "symkl"), R.dist64(q, near, "symkl")
    assert np.abs(np.diag(a32) - np.diag(a64)).max() <= 1e-5 * np.diag(a64).max()


def test_float32_restatement_is_close_to_the_definition():
    rng = np.random.default_rng(2)
    for nz in (7, 20, 64):
        q, g = R.latents(rng, 19, nz), R.latents(rng, 64, nz)
        for metric in R.METRICS:
            ref = R.dist64(q, g, metric)
            err = np.abs(R.dist32(q, g, metric) - ref) / (ref + (nz if metric == "symkl" else 0))
            assert err.max() < 2e-6, (nz, metric, err.max())


def test_total_order_puts_nan_last_and_ties_to_the_lower_index():
    d = np.array([3.0, np.nan, 1.0, np.inf, 1.0, 0.0, np.nan, 3.0], np.float32)
    assert R.order(d).tolist() == [5, 2, 4, 0, 7, 3, 1, 6]
    index, dist = R.topk(d[None], 10)
    assert index[0].tolist() == [5, 2, 4, 0, 7, 3, 1, 6, -1, -1] and np.isinf(dist[0, 8:]).all() and np.isnan(dist[0, 6:8]).all()
    D = np.array([[0.0, 2.0, 1.0], [5.0, 4.0, 3.0], [1.0, 9.0, 1.0]])
    assert R.recall(D, (1, 2, 3)).tolist() == [1 / 3, 1.0, 1.0]                            # row 2 ties with row 0: the lower index is first


def test_python_argument_checks_need_no_device():
    import torch
    from vae_assoc_amd.vae_assoc import topk_args
    nz = 20
    rng = np.random.default_rng(0)
    q, g = R.latents(rng, 9, nz), R.latents(rng, 31, nz)
    args = lambda *a, **kw: topk_args(*a, n_z=nz, device="cpu", **kw)
    qm, ql, gm, gl, k, mid, was_np = args(q, g, 5, "symkl")
    assert tuple(qm.shape) == (9, nz) and tuple(gl.shape) == (31, nz) and k == 5 and mid == 0 and was_np
    assert qm.dtype == torch.float32 and qm.is_contiguous()
    qm, ql, gm, gl, k, mid, was_np = args((torch.from_numpy(q[0]), None), (g[0], None), np.int64(64), "L2")
    assert ql is None and gl is None and k == 64 and mid == 1 and not was_np
    qm, ql, gm, gl, k, mid, was_np = args(q, g, 1, "l2")                                # given log-variances are not marshalled
    assert ql is None and gl is None
    qm, ql, gm, gl, k, mid, was_np = args((q[0][:0], q[1][:0]), (g[0][:0], g[1][:0]), 3, "symkl")
    assert qm.shape[0] == 0 and gm.shape[0] == 0
    for bad in (0, 65, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="k must"):
            args(q, g, bad, "symkl")
    for bad in ("cosine", None, 0, b"l2"):
        with pytest.raises(ValueError, match="metric"):
            args(q, g, 1, bad)
    with pytest.raises(ValueError, match="query: logvar is None"):
        args((q[0], None), g, 1, "symkl")
    with pytest.raises(ValueError, match="gallery: logvar is None"):
        args(q, (g[0], None), 1, "symkl")
    with pytest.raises(ValueError, match="gallery: mu is None"):
        args(q, (None, g[1]), 1, "l2")
    with pytest.raises(ValueError, match="pair"):
        args(q[0], g, 1, "l2")
    with pytest.raises(ValueError, match="pair"):
        args(q, (g[0], g[1], g[1]), 1, "l2")
    with pytest.raises(ValueError, match="query"):
        args((q[0][:, :19], q[1][:, :19]), g, 1, "symkl")                                # wrong width
    with pytest.raises(ValueError, match="gallery"):
        args(q, (g[0], g[1][:30]), 1, "symkl")                                           # logvar rows != mu rows
    with pytest.raises(ValueError, match="gallery"):
        args(q, (g[0], g[1][:, :7]), 1, "symkl")
    with pytest.raises(ValueError, match="query"):
        args((q[0][0], q[1][0]), g, 1, "symkl")                                          # one row must still be [1, n_z]


def test_header_declares_and_library_exports_both_symbols(capi):
    txt = open(os.path.join(ROOT, "include", "avae.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = capi.lib()
    for name in ("avae_latent_topk", "avae_latent_topk_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    for name, value in (("AVAE_METRIC_SYMKL", capi.METRIC_SYMKL), ("AVAE_METRIC_L2", capi.METRIC_L2), ("AVAE_TOPK_MAX", capi.TOPK_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name


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


def _plan(capi, rows, G, k, n_z=20):
    qt, gt, ns, sb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    rc = capi.lib().avae_latent_topk_plan(C.byref(_config(capi, n_z)), rows, G, k, C.byref(qt), C.byref(gt), C.byref(ns), C.byref(sb))
    assert rc == 0, capi.lib().avae_last_error(None)
    return qt.value, gt.value, ns.value, sb.value


PLAN_SHAPES = [(1, 65536), (4096, 65536), (19, 4099), (1, 1), (1, 64), (1, 65), (70, 1000), (15, 4099), (300, 1000), (64, 257),
               (65, 256), (16384, 70000), (100000, 65536), (1000000, 33), (5, 2 ** 31 - 1), (2 ** 31 - 1, 1)]


@pytest.mark.parametrize("rows,G", PLAN_SHAPES)
def test_plan_tiles_cover_the_problem_exactly(capi, rows, G):
    for n_z in (7, 64):
        for k in (1, 10, 64):
            qt, gt, ns, sb = _plan(capi, rows, G, k, n_z)
            assert qt >= 1 and gt >= 1 and ns >= 1
            chunk = min(rows, 16384)
            assert sb == chunk * ns * k * 8 and sb <= 40 << 20
            q, g = R.plan_cover(chunk, G, qt, gt, ns)
            # query tiles: consecutive, none empty, the chunk exactly
            assert q[0][0] == 0 and q[-1][1] == chunk and all(a < b for a, b in q) and all(x[1] == y[0] for x, y in zip(q, q[1:]))
            # gallery splits: consecutive, none empty, whole tiles, the gallery exactly
            assert len(g) == ns and g[0][0] == 0 and g[-1][1] == G
            assert all(a < b for a, b in g) and all(x[1] == y[0] for x, y in zip(g, g[1:])) and all(a % gt == 0 for a, _ in g)
            # the launch is neither tiny next to the device nor unbounded: at most 1024 + 256 workgroups per chunk
            assert len(q) * ns <= 1280


def test_plan_splits_the_gallery_for_few_queries_and_bounds_the_scratch(capi):
    qt, gt, ns, sb = _plan(capi, 1, 65536, 10)
    assert ns > 1 and ns >= 256                      # one query against a large gallery: at least one workgroup per CU
    assert _plan(capi, 4096, 65536, 10)[2] * (4096 // qt) >= 512
    assert _plan(capi, 1, 1, 1)[2] == 1
    assert _plan(capi, 7, 0, 3)[2:] == (0, 0)        # an empty gallery: no split, no scratch (the merge launch alone pads)
    assert _plan(capi, 0, 100, 3)[3] == 0
    # tests/test_gpu_retrieve.py relies on these: several tiles per split AND several splits
    for rows, G in ((1, 1000), (15, 1000), (70, 1000), (1, 4099), (15, 4099), (70, 4099), (300, 1000)):
        qt, gt, ns, _ = _plan(capi, rows, G, 5)
        assert ns >= 2 and -(-G // gt) >= 2 * ns, (rows, G, ns)
    assert -(-70 // _plan(capi, 70, 1000, 5)[0]) == 2 and -(-300 // qt) >= 2      # ... and several query tiles
    # the scratch does not grow with the number of queries
    sizes = [_plan(capi, rows, 65536, 64)[3] for rows in (1, 64, 4096, 16384, 16385, 10 ** 6, 2 ** 31 - 1)]
    assert max(sizes) <= 40 << 20 and sizes[-1] == sizes[-2] == sizes[-3] == sizes[-4]
    # a function of (rows, gallery_rows, k) alone
    assert _plan(capi, 19, 4099, 5, n_z=7) == _plan(capi, 19, 4099, 5, n_z=64)


def test_plan_errors(capi):
    L = capi.lib()
    cfg = _config(capi)
    out = C.c_int32(0)
    for rows, G, k, needle in ((1, 1, 0, "k = 0"), (1, 1, 65, "k = 65"), (1, 1, -3, "k = -3"), (-1, 1, 1, "rows"), (1, -1, 1, "gallery_rows")):
        assert L.avae_latent_topk_plan(C.byref(cfg), rows, G, k, C.byref(out), None, None, None) != 0
        assert needle in L.avae_last_error(None).decode(), (rows, G, k)
    assert L.avae_latent_topk_plan(None, 1, 1, 1, None, None, None, None) != 0
    bad = _config(capi)
    bad.n_z = 65
    assert L.avae_latent_topk_plan(C.byref(bad), 1, 1, 1, None, None, None, None) != 0 and "n_z" in L.avae_last_error(None).decode()
    assert L.avae_latent_topk_plan(C.byref(cfg), 5, 7, 64, None, None, None, None) == 0          # every output is optional
