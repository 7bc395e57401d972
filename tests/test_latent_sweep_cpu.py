"""tests/test_gpu_latent_sweep.py kept honest without a device: every case of tests/latent_sweep_cases.py has a finite float64
reference and a float32 restatement whose own pooled error is not zero (4 x 0 would demand bit equality with float64), the
lattice inputs of the many-splits cases make the float32 chain equal the integer result, and the split counts those cases are
named after come out of the library's plan call."""
import numpy as np
import pytest

import aggregate_reference as A
import latent_stats_reference as S
import latent_sweep_cases as W
import retrieve_reference as R
from test_retrieve_cpu import _plan


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


# ------------------------------------------------------------------------------------------------ A. the n_z sweep
def test_the_sweep_covers_every_width_class_exact_one_past_and_most_idle():
    cls = lambda nz: 8 if nz <= 8 else 16 if nz <= 16 else 32 if nz <= 32 else 64
    for nzs in (W.NZ_NEW, W.PRIOR_NZ):
        assert all(1 <= nz <= 64 for nz in nzs) and not set(nzs) & {7, 20, 64}           # what the four kernels' own files run
        assert {cls(nz) for nz in nzs} == {8, 16, 32, 64}
        assert {8, 16, 32} <= set(nzs) and {9, 17, 33} <= set(nzs)                       # no idle column; the most idle columns
    assert {1, 2, 3} <= set(W.NZ_NEW) and 63 in W.NZ_NEW
    for JW in (8, 16, 32, 64):                                      # one past phase 2's stride KG = 256 / JW in every class
        assert 256 // JW + 1 in [K for nz, K in W.PRIOR_PAIRS if cls(nz) == JW], JW
    assert {1, 16, 17, 64} <= {K for _, K in W.PRIOR_PAIRS}         # ... and phase 1's round of 16: exactly, one past, all four
    assert set(W.TOPK_SELECT_NZ) <= set(W.NZ_NEW) and set(W.STATS_MASKED_NZ) <= set(W.NZ_NEW)
    assert set(W.AGG_BIG_NZ) <= set(W.NZ_NEW) and set(W.AGG_EXCLUDE_NZ) <= set(W.NZ_NEW)


@pytest.mark.parametrize("nz", W.NZ_NEW)
def test_topk_references_are_finite_and_the_restatement_errs(nz):
    for metric in R.METRICS:
        q, g, ref, own = W.topk_case(nz, metric)
        assert q[0].shape == (19, nz) and g[0].shape == (64, nz) and np.isfinite(ref).all() and (ref > 0).all()
        assert 0.0 < own < 2e-6, (metric, own)


@pytest.mark.parametrize("nz", W.NZ_NEW)
def test_stats_references_are_finite_and_the_restatement_errs(nz):
    tol, own = W.stats_bound(nz)
    for name in S.FAMILIES:
        for rows in W.STATS_ROWS:
            ref = S.case(name, rows, nz)[1]
            assert (ref["count"] == rows).all() and all(np.isfinite(ref[k]).all() for k in S.NAMES[1:]), (name, rows)
    assert all(0.0 < own[k] < np.inf for k in own), own
    assert tol == {k: 4.0 * own[k] for k in own}
    loose, _ = S.bound(nz)                                          # pooled over fewer rows: never looser than the reference module's
    assert all(tol[k] <= loose[k] for k in tol)


@pytest.mark.parametrize("nz", W.STATS_MASKED_NZ)
def test_masked_stats_reference_has_the_sets_the_test_looks_at(nz):
    post, present = W.stats_masked_case(nz=nz)
    ref = S.stats64(post[:3] + [None], present)
    assert ref["count"][2, 2] == 1 and ref["count"][1, 2] == 0 and ref["count"][0, 2] == 1 and not ref["count"][3].any()
    full = ref["count"] > 0
    for k in S.TABLES:
        assert np.array_equal(np.isfinite(ref[k]).all(-1), full), k


@pytest.mark.parametrize("nz", W.NZ_NEW)
def test_density_references_are_finite_and_the_restatement_errs(nz):
    z, g, refs, own = W.agg_small_case(nz)
    assert sorted(refs) == sorted(W.AGG_SMALL) and all(np.isfinite(r[0]).all() and np.isfinite(r[1]).all() for r in refs.values())
    assert 0.0 < own[0] < 1e-5 and 0.0 < own[1] < 1e-5, own


@pytest.mark.parametrize("nz", W.AGG_BIG_NZ)
def test_density_references_of_the_three_slice_case(nz, capi):
    import ctypes as C
    from test_retrieve_cpu import _config
    z, g, ref, own = W.agg_big_case(nz)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and 0.0 < own[0] < 1e-5 and 0.0 < own[1] < 1e-5, own
    v = [C.c_int32(-1) for _ in range(4)]
    assert capi.lib().avae_agg_logpdf_plan(C.byref(_config(capi, nz)), *W.AGG_BIG, *[C.byref(x) for x in v], None) == 0
    query_tile, _, slice_rows, n_slices = (x.value for x in v)
    assert (query_tile, slice_rows, n_slices) == (64, 1024, 3) and (W.AGG_BIG[1] - 2 * slice_rows) % 64 == 52
    if nz in W.AGG_EXCLUDE_NZ:
        z, g, ex, ref, own = W.agg_exclude_case(nz)
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and 0.0 < own[0] < 1e-5 and 0.0 < own[1] < 1e-5, own
        plain = A.logpdf64(z, g)
        inside = (ex >= 0) & (ex < g[0].shape[0])
        assert inside.sum() == len(ex) - 4 and (ref[0][inside] != plain[0][inside]).all()
        assert np.array_equal(ref[0][~inside], plain[0][~inside])


@pytest.mark.parametrize("nz", W.PRIOR_NZ)
def test_prior_references_are_finite_and_the_restatement_errs(nz):
    cases, own, own_sc = W.prior_case(nz)
    Ks = [K for z, K in W.PRIOR_PAIRS if z == nz]
    assert len(cases) == len(Ks) * len(W.PRIOR_N) * 2
    for K, N, mu, logvar, init, ref, bound, ll64, r64 in cases:
        assert np.isfinite(bound) and all(np.isfinite(ref[k]).all() for k in W.PRIOR_KEYS), (K, N)
        assert ref["means"].shape == (K, nz) and np.isfinite(ll64).all() and np.isfinite(r64).all()
        assert np.abs(r64.sum(1) - 1.0).max() < 1e-12
    assert all(0.0 < o < 0.05 for o in own), own                   # (1, 1) alone would give a weight error of exactly 0
    assert own_sc[1] > 0.0 and (own_sc[0] > 0.0 or Ks == [1]), own_sc


# ------------------------------------------------------------------------------------------------ B. more than 64 splits
@pytest.mark.parametrize("rows,G,nz,splits", W.LATTICE)
def test_lattice_chain_in_float32_is_the_integer_result(rows, G, nz, splits):
    q, g = W.lattice_case(rows, G, nz)
    n = min(rows, 8)                                                # (the first query tile's share is enough for the arithmetic)
    q = (q[0][:n], q[1][:n])
    qi, gi = q[0].astype(np.int64), g[0].astype(np.int64)
    D = ((qi[:, None, :] - gi[None]) ** 2).sum(-1)
    assert D.max() <= nz * 256 < 2 ** 23
    for metric in R.METRICS:
        d32 = R.dist32(q, g, metric)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.int64), D) and np.array_equal(d32, D.astype(np.float32)), metric
    index, dist = W.lattice_table(q, g, 64)
    want_i, want_d = R.topk(D.astype(np.float32), 64)
    assert np.array_equal(index, want_i) and np.array_equal(dist, want_d)
    # many ties, spread over many splits: the merge has to order equal keys of different lanes and heads by index
    per = -(-(-(-G // 64)) // splits) * 64
    assert len(np.unique(dist[0])) < 64 and len(np.unique(index[0] // per)) > 16
    if G == 65536:
        assert index[0, :4].tolist() == list(W.LATTICE_PLANTED) and not dist[0, :4].any() and dist[0, 4] > 0
        assert [r // per for r in W.LATTICE_PLANTED] == [64, 128, 192, 255]                 # heads r = 1, 2, 3 only


def test_plan_figures_of_the_many_splits_cases(capi):
    for rows, G, nz, splits in W.LATTICE:
        for k in W.TOPK_KS:
            qt, gt, ns, _ = _plan(capi, rows, G, k, nz)
            assert (qt, gt, ns) == (64, 64, splits), (rows, G, k)
    tiles = lambda G: -(-G // 64)
    assert tiles(16385) == 64 * 4 + 1 and tiles(65536) == 256 * 4 and -(-tiles(65537) // 205) == 5 and tiles(65537) - 204 * 5 == 5
    G, nz, calls = W.FLOAT_SPLITS
    for rows, splits in calls:
        assert _plan(capi, rows, G, 64, nz)[2] == splits
    # ... and the sweep's selection check runs several splits of several tiles, two query tiles
    qt, gt, ns, _ = _plan(capi, 70, W.TOPK_SELECT_G, 5, 9)
    assert ns == 4 and tiles(W.TOPK_SELECT_G) == 16 and -(-70 // qt) == 2
