"""latent_topk, latent_stats, aggregate_log_density and fit_latent_prior / latent_prior_score on a real MI355X at the latent
widths, component counts and split counts their own test files (n_z in {7, 20, 64}) never run; the inputs are
tests/latent_sweep_cases.py's, which tests/test_latent_sweep_cpu.py checks without a device.

A. one test per kernel family over n_z in NZ_NEW = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63): every width class of the thread maps
   (8, 16, 32, 64) at its exact, one-past and most idle width, Gram blocks and unrolled loops shorter than 4, waves without a
   marginal column, the merge's 64 columns exactly; the mixture kernels at (n_z, K) pairs one past a stride of either phase.
   Arithmetic against the float64 definition within 4x the float32 restatement's own worst error on the same inputs, pooled per
   n_z over the test's case list; selection, repetition and call independence bit for bit.
B. latent_topk with 65, 205 and 256 splits (the merge keeps up to four list heads per lane; the kernels' own files stop at 17
   splits): integer lattice latents, whose distances are exact in float32, against a table computed in integer arithmetic, bit
   for bit, and random latents against the same query in a call with 13 splits.

The model is only a handle with the right n_z: one small dense modality, batch_size = 16, fp32, released before the next n_z."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_prior_reference as P
import latent_stats_reference as S
import latent_sweep_cases as W
import retrieve_reference as R
import test_gpu_aggregate as TA
import test_gpu_latent_prior as TP
import test_gpu_latent_stats as TS
import test_gpu_retrieve as TR
from conftest import make_arch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


@pytest.fixture(scope="module")
def model(V, request):
    """a handle with n_z = request.param; its scratch allocations (about 100 MB for these entry points) go before the next one's come"""
    m = V.AssocVariationalAutoEncoder([make_arch("solo", 25, 9, 7, request.param)], binary=True, transfer_fct="relu", batch_size=16,
                                      compute_dtype="fp32", device=0, seed=3)
    yield m
    m.synchronize()
    m.__del__()


def over(nzs):
    return pytest.mark.parametrize("model", nzs, indirect=True, ids=["nz%d" % nz for nz in nzs])


def _dev(model, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(model.device) for a in arrays)


# ------------------------------------------------------------------------------------------------ A1. latent_topk
@over(W.NZ_NEW)
def test_topk_every_distance_against_the_float64_definition(model):
    """tests/test_gpu_retrieve.py's test 1 at the new widths: every distance of k = G calls, the index rows permutations, the
    distances ascending.  Measured on the MI355X, 2026-10-19, kernel worst / restatement worst: symkl from 2.2e-7 / 2.9e-7 (n_z = 1)
    to 5.7e-7 / 4.7e-7 (n_z = 63), the largest ratio 1.6 (4.3e-7 / 2.7e-7 at n_z = 16); l2 from 1.6e-7 / 1.6e-7 to 4.8e-7 / 4.8e-7, the
    largest ratio 1.1 (n_z = 33)."""
    nz = model.n_z
    for metric in R.METRICS:
        q, g, ref, own = W.topk_case(nz, metric)
        worst = 0.0
        for N, G in W.TOPK_NG:
            r = model.latent_topk((q[0][:N], q[1][:N]), (g[0][:G], g[1][:G]), k=G, metric=metric)
            assert r["index"].shape == (N, G) and r["index"].dtype == np.int32 and r["distance"].dtype == np.float32
            assert np.array_equal(np.sort(r["index"], 1), np.tile(np.arange(G, dtype=np.int32), (N, 1)))
            D = np.empty((N, G), np.float32)
            np.put_along_axis(D, r["index"].astype(np.int64), r["distance"], 1)
            worst = max(worst, W.rel_err(D, ref[:N, :G], nz, metric).max())
            assert np.all(np.diff(r["distance"], axis=1) >= 0)
        print("n_z=%d %s: float32 restatement worst rel err %.3e, kernel worst %.3e (bound 4x)" % (nz, metric, own, worst))
        assert worst <= 4.0 * own, (metric, worst, own)


@over(W.TOPK_SELECT_NZ)
@pytest.mark.parametrize("metric", R.METRICS)
def test_topk_selection_is_the_total_order_of_the_kernels_own_distances(model, metric):
    """tests/test_gpu_retrieve.py's test 2 (its gallery with duplicates, NaN means and infinite log-variances, its matrix of the
    kernel's own distances from chunk calls) at G = 1000: 16 gallery tiles in 4 splits, N = 70 two query tiles.  A staging error
    that moves a value to the wrong (row, dimension) only at some tile offsets shows as a difference between the chunk calls
    (chunks of 64, 1, 37, 63, 5 rows: every tile starts elsewhere) and the whole call."""
    nz, G = model.n_z, W.TOPK_SELECT_G
    q, g, D = TR._own_matrix(model, nz, G, metric)
    assert np.isnan(D[:, 5]).all() and np.isnan(D[:, 130]).all() and np.isnan(D[:, G - 3]).all()
    assert np.isnan(D[:, G // 3]).all() == (metric == "symkl")
    assert not TR._bits(D[0, [7, 300, G - 2]]).any() and not TR._bits(D[1, 64]).any()
    assert np.array_equal(TR._bits(D[:, 3]), TR._bits(D[:, 2])) and np.array_equal(TR._bits(D[:, 10]), TR._bits(D[:, 700]))
    for N in (1, 15, TR.N_MAX):
        for k in W.TOPK_KS:
            got = model.latent_topk((q[0][:N], q[1][:N]), g, k=k, metric=metric)
            want_i, want_d = R.topk(D[:N], k)
            assert np.array_equal(got["index"], want_i), (N, k, np.argwhere(got["index"] != want_i)[:4].tolist())
            assert np.array_equal(TR._bits(got["distance"]), TR._bits(want_d)), (N, k)
    top = model.latent_topk((q[0][:2], q[1][:2]), g, k=5, metric=metric)["index"]
    assert top[0, :3].tolist() == [7, 300, G - 2] and top[1, 0] == 64


# ------------------------------------------------------------------------------------------------ A2. latent_stats
@over(W.NZ_NEW)
def test_stats_every_statistic_against_the_float64_definition(model):
    """tests/test_gpu_latent_stats.py's test 1 with the bound pooled over rows in {1, 2, 65, 4099}: families A, B, C, M = 2, every
    statistic including cov; the diagonal of xcov is var bit for bit; a second call gives the same bits.  Measured on the MI355X,
    2026-10-19, kernel worst over the twelve widths (the restatement's own worst in brackets): mean 3.0e-16 (1.1e-6 to 2.6e-6),
    var and xcov 8.7e-13 (6.4e-4 to 1.1e-1), assoc 1.6e-7 (7.9e-7 to 3.0e-6), post_var 6.9e-8 (1.8e-6 to 3.1e-6), kl 4.2e-8
    (3.0e-5 to 3.2e-5), cov 2.4e-7 (6.4e-4 to 1.1e-1)."""
    nz = model.n_z
    tol, own = W.stats_bound(nz)
    worst = {k: 0.0 for k in tol}
    for name in S.FAMILIES:
        for rows in W.STATS_ROWS:
            post, ref, _ = S.case(name, rows, nz)
            got = model.latent_stats(post)
            assert got["mean"].shape == (2, 2, nz) and got["kl"].shape == (2, nz) and got["cov"].shape == (2, nz, nz)
            assert (got["count"] == rows).all()
            for k, e in S.errors(got, ref).items():
                worst[k] = max(worst[k], e)
            assert not TS._bits(got["assoc"][[0, 1], [0, 1]]).any()
            assert np.array_equal(TS._bits(got["xcov"][[0, 1], [0, 1]]), TS._bits(got["var"][[0, 1], [0, 1]]))
            assert np.array_equal(got["cov"], np.swapaxes(got["cov"], 1, 2))
            assert TS._same(model.latent_stats(post), got), (name, rows)
            if rows == 1:
                for k in ("var", "xcov", "cov"):
                    assert not TS._bits(got[k]).any(), k
                for s in range(2):
                    for d in range(2):
                        assert np.array_equal(got["mean"][s, d], post[s][0][0].astype(np.float64))
    for k in tol:
        print("n_z=%d %-8s float32 restatement worst %.3e, bound %.3e, kernel worst %.3e" % (nz, k, own[k], tol[k], worst[k]))
    assert TS._within(worst, tol), worst


@over(W.STATS_MASKED_NZ)
def test_stats_masks_against_the_float64_definition(model):
    """tests/test_gpu_latent_stats.py's masked case (M = 4: two modalities on random rows, one on a single row, one NULL; NaN in
    every absent entry) at n_z = 3 (one partial Gram block), 9 and 33, at the bound of the test above.  Measured on the MI355X,
    2026-10-19, kernel worst at n_z = 3 / 9 / 33: var 2.9e-15 / 2.9e-15 / 5.3e-15, assoc 4.4e-8 / 4.0e-8 / 1.2e-7, post_var 4.6e-8 /
    4.7e-8 / 7.2e-8, kl 2.2e-8 / 4.4e-9 / 2.5e-8, cov 6.8e-9 / 9.0e-9 / 1.6e-8."""
    nz = model.n_z
    post, present = W.stats_masked_case(nz=nz)
    null3 = post[:3] + [None]
    ref = S.stats64(null3, present)
    got = model.latent_stats(null3, present)
    assert np.array_equal(got["count"], ref["count"])
    assert got["count"][2, 2] == 1 and got["count"][1, 2] == 0 and got["count"][0, 2] == 1 and not got["count"][3].any()
    err = S.errors(got, ref)
    tol, _ = W.stats_bound(nz)
    print("n_z=%d masked: kernel worst" % nz, {k: "%.3e" % v for k, v in err.items()}, "bound", {k: "%.3e" % v for k, v in tol.items()})
    assert TS._within(err, tol), err
    for k in S.TABLES:
        assert np.isnan(got[k][1, 2]).all() and np.isnan(got[k][2, 1]).all() and np.isnan(got[k][3]).all() and np.isnan(got[k][:, 3]).all()
    assert np.isnan(got["post_var"][3]).all() and np.isnan(got["kl"][3]).all() and np.isnan(got["cov"][3]).all()
    assert not TS._bits(got["var"][2, 2]).any() and not TS._bits(got["cov"][2]).any() and not TS._bits(got["xcov"][0, 2]).any()
    assert np.array_equal(got["mean"][2, 0], post[2][0][1234].astype(np.float64))
    assert np.array_equal(got["mean"][0, 2], post[0][0][1234].astype(np.float64))
    assert np.array_equal(TS._bits(got["xcov"][[0, 1, 2], [0, 1, 2]]), TS._bits(got["var"][[0, 1, 2], [0, 1, 2]]))
    filled = [(np.where(np.isnan(mu), np.float32(7.0), mu), np.where(np.isnan(lv), np.float32(-1.0), lv)) for mu, lv in post[:3]] + [None]
    assert TS._same(model.latent_stats(filled, present), got)
    assert TS._same(model.latent_stats(null3, present), got)


# ------------------------------------------------------------------------------------------------ A3. aggregate_log_density
@over(W.NZ_NEW)
def test_density_against_the_float64_definition(model):
    """tests/test_gpu_aggregate.py's test 1 (N in {1, 19} x G in {1, 5, 64}, joint and marginals) at the new widths.  Measured on
    the MI355X, 2026-10-19, kernel worst / restatement worst: joint from 8.7e-8 / 9.6e-8 (n_z = 1) to 3.0e-7 / 3.0e-7 (n_z = 33),
    marginals from 8.7e-8 / 9.6e-8 to 2.3e-7 / 2.7e-7 (n_z = 32); the kernel's is never above the restatement's."""
    nz = model.n_z
    z, g, refs, own = W.agg_small_case(nz)
    worst = [0.0, 0.0]
    for N, G in W.AGG_SMALL:
        r = model.aggregate_log_density(z[:N], (g[0][:G], g[1][:G]))
        assert r["joint"].shape == (N,) and r["joint"].dtype == np.float32
        assert r["marginal"].shape == (N, nz) and r["marginal"].dtype == np.float32
        ej, em = TA._errs(r, refs[N, G], nz)
        worst = [max(worst[0], ej), max(worst[1], em)]
    print("n_z=%d: float32 restatement worst error joint %.3e marginal %.3e; kernel worst joint %.3e marginal %.3e (bound 4x)"
          % (nz, own[0], own[1], worst[0], worst[1]))
    assert worst[0] <= 4.0 * own[0] and worst[1] <= 4.0 * own[1]


@over(W.AGG_BIG_NZ)
def test_density_three_slices_a_ragged_tail_and_call_independence(model):
    """(N, G) = (130, 2100): three query tiles (the last of 2 rows), three slices, the last tile of 52 rows; query 0 alone gives
    the bits of row 0 of the whole call, and so does the whole call again.  Measured on the MI355X, 2026-10-19, kernel /
    restatement at n_z = 1, 9, 33, 63: joint 5.8e-8 / 9.9e-7, 9.9e-8 / 1.2e-7, 2.0e-7 / 2.3e-7, 3.9e-7 / 3.3e-7; marginals 3.4e-7 /
    9.9e-7, 4.3e-7 / 1.0e-6, 4.9e-7 / 1.1e-6, 4.4e-7 / 1.2e-6."""
    nz = model.n_z
    N, G = W.AGG_BIG
    assert TA._plan(model, N, G)[2:] == (1024, 3)
    z, g, ref, own = W.agg_big_case(nz)
    zd, gm, gl = _dev(model, z, g[0], g[1])
    big = model.aggregate_log_density(zd, (gm, gl))
    ej, em = TA._errs({k: v.cpu().numpy() for k, v in big.items()}, ref, nz)
    print("n_z=%d N=%d G=%d: restatement joint %.3e marginal %.3e; kernel joint %.3e marginal %.3e" % (nz, N, G, own[0], own[1], ej, em))
    assert ej <= 4.0 * own[0] and em <= 4.0 * own[1]
    for i in (0, 63, 64, 129):
        one = model.aggregate_log_density(zd[i:i + 1], (gm, gl))
        assert TA._same(one, {k: v[i:i + 1] for k, v in big.items()}), i
    assert TA._same(model.aggregate_log_density(zd, (gm, gl)), big)
    only_j = model.aggregate_log_density(zd, (gm, gl), marginals=False)
    assert only_j["marginal"] is None and np.array_equal(TA._bits(only_j["joint"]), TA._bits(big["joint"]))


@over(W.AGG_EXCLUDE_NZ)
def test_density_leave_one_out(model):
    """tests/test_gpu_aggregate.py's exclusion case (N = 70, G = 133, excluded rows on block and tile borders, four entries that
    name no row) at n_z = 9 and 63.  Measured on the MI355X, 2026-10-19, kernel / restatement: n_z = 9 joint 1.7e-7 / 1.7e-7,
    marginals 2.4e-7 / 2.4e-7; n_z = 63 joint 2.5e-7 / 2.9e-7, marginals 2.6e-7 / 2.7e-7."""
    nz = model.n_z
    z, g, ex, ref, own = W.agg_exclude_case(nz)
    got = model.aggregate_log_density(z, g, exclude=ex)
    ej, em = TA._errs(got, ref, nz)
    print("n_z=%d exclusion: restatement joint %.3e marginal %.3e; kernel joint %.3e marginal %.3e" % (nz, own[0], own[1], ej, em))
    assert ej <= 4.0 * own[0] and em <= 4.0 * own[1]
    plain = model.aggregate_log_density(z, g)
    assert TA._same({k: v[6:10] for k, v in got.items()}, {k: v[6:10] for k, v in plain.items()})
    assert not np.array_equal(TA._bits(got["joint"][:6]), TA._bits(plain["joint"][:6]))
    one = model.aggregate_log_density(z[:1], g, exclude=ex[:1])
    assert TA._same(one, {k: v[:1] for k, v in got.items()})


# ------------------------------------------------------------------------------------------------ A4. the mixture prior
@over(W.PRIOR_NZ)
def test_prior_one_iteration_and_the_score_against_the_float64_definition(model):
    """tests/test_gpu_latent_prior.py's test 1 at the (n_z, K) pairs of PRIOR_PAIRS, N in {1, 19, 64, 65, 300}, with and without
    logvar: one iteration against step64, then latent_prior_score of the same start against estep64; component is the argmax of
    the kernel's own responsibilities (lowest index on ties) and every row of them sums to 1 within their tolerance.

    Measured on the MI355X, 2026-10-19, kernel worst / restatement worst (weights, means, logvars, bound; resp, ll), at the ends of
    the range: n_z = 1, K in {1, 64}: 1.7e-8 / 2.2e-8, 1.6e-7 / 3.2e-7, 1.9e-7 / 9.0e-7, 3.5e-7 / 4.0e-7; 3.7e-8 / 4.4e-8, 3.5e-7 /
    1.5e-7; n_z = 63, K = 63: 6.7e-7 / 6.7e-7, 2.5e-5 / 2.5e-5, 3.7e-5 / 1.1e-3, 1.2e-7 / 1.8e-7; 1.3e-5 / 1.3e-5, 2.9e-7 / 2.9e-7.  The
    largest ratios: ll 2.3 (n_z = 1), means 1.18 and logvars 1.18 (n_z = 16), resp 1.21 (n_z = 2).  |sum_k r - 1| is 6.2e-8 to 8.9e-8.

    Two things this test found in k_gmm_estep, both fixed there.  The normaliser of the responsibilities was an fp32 running
    sum: |sum_k r - 1| was 3.0e-7 at n_z = 1, K = 64, N = 1, above 4 x 4.4e-8 (it is added in fp64 now).  The sums behind the
    M-step were fp32 over a tile: at n_z = 2, K = 3, N = 1 with logvar the log-variance error was 3.19e-6 against 4 x 7.24e-7 --
    with one row the variance is S2 / R - (S1 / R)^2 = (d^2 + v) - d^2, and the fp32 roundings of r (d^2 + v) and r d were amplified
    by d^2 / v.  With d and the products in fp64 it is 8.2e-8 there, and at n_z = 12, K = 64 2.0e-6 where the restatement has 9.4e-3."""
    nz = model.n_z
    cases, own, own_sc = W.prior_case(nz)
    worst, worst_sc, worst_sum = [0.0] * 4, [0.0, 0.0], 0.0
    for K, N, mu, logvar, init, ref, bound, ll64, r64 in cases:
        got = model.fit_latent_prior((mu, logvar), n_components=K, n_iters=1, init=init)
        assert got["weights"].shape == (K,) and got["means"].shape == (K, nz) and got["logvars"].shape == (K, nz)
        assert got["n_used"] == N and np.isfinite(got["bound"]).all() and got["bound"].shape == (2,)
        errs = TP._step_errs(got, ref, bound, nz)
        assert all(e <= 4.0 * o for e, o in zip(errs, own)), (K, N, logvar is None, errs, own)
        worst = [max(w, e) for w, e in zip(worst, errs)]
        sc = model.latent_prior_score(mu if logvar is None else (mu, logvar), init, responsibilities=True)
        assert sc["log_density"].shape == (N,) and sc["component"].dtype == np.int32 and sc["responsibilities"].shape == (N, K)
        e_sc = (float(P.abs_err(sc["responsibilities"], r64).max()), float(P.ll_err(sc["log_density"], ll64, nz).max()))
        assert e_sc[0] <= 4.0 * own_sc[0] and e_sc[1] <= 4.0 * own_sc[1], (K, N, logvar is None, e_sc, own_sc)
        worst_sc = [max(w, e) for w, e in zip(worst_sc, e_sc)]
        assert np.array_equal(sc["component"], sc["responsibilities"].argmax(axis=1)), (K, N)
        e_sum = float(np.abs(sc["responsibilities"].astype(np.float64).sum(axis=1) - 1.0).max())
        assert e_sum <= 4.0 * own_sc[0], (K, N, e_sum, own_sc[0])
        worst_sum = max(worst_sum, e_sum)
        # the bound of the incoming parameters is the mean of the scores: the same fp32 numbers summed in fp64 in another order
        ll = sc["log_density"].astype(np.float64)
        assert abs(ll.mean() - got["bound"][0]) <= N * 2.0 ** -52 * np.abs(ll).max(), (K, N)
    print("n_z=%d K=%s: float32 restatement worst weights %.3e means %.3e logvars %.3e bound %.3e resp %.3e ll %.3e; kernel worst "
          "weights %.3e means %.3e logvars %.3e bound %.3e resp %.3e ll %.3e, |sum r - 1| %.3e (bound 4x)"
          % ((nz, sorted({c[0] for c in cases})) + tuple(own) + tuple(own_sc) + tuple(worst) + tuple(worst_sc) + (worst_sum,)))


# ------------------------------------------------------------------------------------------------ B. more than 64 splits
def _topk_plan(model, rows, G, k):
    """-> (query_tile, gallery_tile, n_splits)"""
    v = [C.c_int32(-1) for _ in range(3)]
    assert model._L.avae_latent_topk_plan(C.byref(model._cfg), rows, G, k, *[C.byref(x) for x in v], None) == 0
    return tuple(x.value for x in v)


@pytest.mark.parametrize("model,rows,G,splits", [(nz, rows, G, splits) for rows, G, nz, splits in W.LATTICE], indirect=["model"],
                         ids=["nz%d-%dx%d-%dsplits" % (nz, rows, G, splits) for rows, G, nz, splits in W.LATTICE])
def test_topk_merge_of_more_than_64_splits_is_exact_on_lattice_latents(model, rows, G, splits):
    """k_latent_topk_merge keeps the heads of the splits lane, lane + 64, lane + 128, lane + 192 per lane; with at most 17 splits
    (tests/test_gpu_retrieve.py) only the first is ever live.  Integer latents with lv = 0 make every distance exact in float32
    and, under symkl, the same number (t = 0, iv = 1, times 0.5), so index and distance must equal the integer table bit for
    bit, for both metrics; the lattice has many ties, which the merge has to break by index across lanes and heads.  In the
    65536-row case the four copies of query 0 sit in splits 64, 128, 192 and 255: heads r = 1, 2, 3 only."""
    nz = model.n_z
    for k in W.TOPK_KS:
        assert _topk_plan(model, rows, G, k) == (64, 64, splits), k
    q, g = W.lattice_case(rows, G, nz)
    want_i, want_d = W.lattice_table(q, g, 64)
    qd, gd = _dev(model, *q), _dev(model, *g)
    for metric in R.METRICS:
        for k in W.TOPK_KS:
            got = {key: v.cpu().numpy() for key, v in model.latent_topk(qd, gd, k=k, metric=metric).items()}
            assert np.array_equal(got["index"], want_i[:, :k]), (metric, k, np.argwhere(got["index"] != want_i[:, :k])[:4].tolist())
            assert np.array_equal(TR._bits(got["distance"]), TR._bits(want_d[:, :k])), (metric, k)
            if G == 65536:
                n = min(k, 4)
                assert got["index"][0, :n].tolist() == list(W.LATTICE_PLANTED[:n]) and not TR._bits(got["distance"][0, :n]).any()


@over((W.FLOAT_SPLITS[1],))
@pytest.mark.parametrize("metric", R.METRICS)
def test_topk_of_256_splits_equals_the_same_query_under_13_splits(model, metric):
    """Random float latents, G = 65536, k = 64: one query alone (256 splits of 4 tiles) against the same query as row 0 of a
    5000-query call (13 splits of 79 tiles); the value of a pair does not depend on the split, so the lists are the same bits."""
    G, nz, calls = W.FLOAT_SPLITS
    for rows, splits in calls:
        assert _topk_plan(model, rows, G, 64)[2] == splits
    rng = np.random.default_rng(65536 + nz)
    q, g = R.latents(rng, calls[1][0], nz), R.latents(rng, G, nz)
    qd, gd = _dev(model, *q), _dev(model, *g)
    cut = lambda r: {k: v[:1].cpu().numpy() for k, v in r.items()}
    one = cut(model.latent_topk((qd[0][:1], qd[1][:1]), gd, k=64, metric=metric))
    many = cut(model.latent_topk(qd, gd, k=64, metric=metric))
    assert TR._same(one, many)
    assert len(set(one["index"][0].tolist())) == 64 and np.all(np.diff(one["distance"][0]) >= 0)
    # ... and they are distances: against float64 at the bound of tests/test_gpu_retrieve.py's test 1 at this n_z
    ref = R.dist64((q[0][:1], q[1][:1]), g, metric)[0, one["index"][0]]
    assert W.rel_err(one["distance"][0], ref, nz, metric).max() <= 4.0 * W.topk_case(nz, metric)[3]
