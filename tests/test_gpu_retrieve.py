"""latent_topk / avae_latent_topk on a real MI355X (include/avae.h) against tests/retrieve_reference.py.

1. arithmetic: every distance of small galleries (k = G) against the float64 definition, within 4x the float32 restatement's own
   worst error on the same inputs;
2. selection, exactly: index and distance of a call over several gallery tiles, splits and query tiles equal the documented
   total order of the kernel's OWN distance matrix, bit for bit.  That matrix is put together from calls on gallery chunks of at
   most 64 rows with k = the chunk size: the value of a pair is a pure function of the two rows' bits, so the chunk calls give the
   bits the big call compares.  (Indices against float64 would fail on honest near-ties.)  The gallery holds bitwise duplicates
   (ties go to the lower index), rows with mu = NaN and rows with lv = +Inf (NaN distances: they rank last);
3. split independence and determinism; 4. edges and errors of the C ABI; 5. the Python surface; 6. no side effects on training.

batch_size = 16, small MLPs, n_z in {7, 20, 64}; latents mu ~ N(0, 1), lv ~ U(-6, 1), seeded."""
import numpy as np
import pytest
import torch

import retrieve_reference as R
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
    """one fp32 relu model per n_z, shared by the tests that only look latents up"""
    if fresh or nz not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, nz), make_arch("joint", 147, 72, 40, nz)]
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          learning_rate=1e-3, batch_size=B, compute_dtype="fp32", device=0, seed=3, **kw)
        if fresh:
            return m
        _MODELS[nz] = m
    return _MODELS[nz]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    return (np.array_equal(np.asarray(a["index"]), np.asarray(b["index"]))
            and np.array_equal(_bits(a["distance"]), _bits(b["distance"])))


def _rel_err(got, ref, nz, metric):
    return np.abs(got.astype(np.float64) - ref) / (ref + (nz if metric == "symkl" else 0.0))


# ------------------------------------------------------------------------------------------------ 1. arithmetic
_CASES = {}


def _arith_case(nz, metric):
    """Test 1's inputs and its tolerance: 19 queries, 64 gallery rows, the float64 definition on them, and the worst error of the
    float32 restatement over these 19 x 64 pairs (denominator ref + n_z for symkl -- the two-KL form's scale, what the assoc
    column of score_samples is accurate to -- and ref for l2)."""
    if (nz, metric) not in _CASES:
        rng = np.random.default_rng(100 + nz)
        q, g = R.latents(rng, 19, nz), R.latents(rng, 64, nz)
        ref = R.dist64(q, g, metric)
        _CASES[nz, metric] = (q, g, ref, float(_rel_err(R.dist32(q, g, metric), ref, nz, metric).max()))
    return _CASES[nz, metric]


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("nz", [7, 20, 64])
def test_every_distance_against_the_float64_definition(V, nz, metric):
    """The bound is 4x the worst error of the float32 restatement over THESE inputs (the 19 x 64 pairs every case below is cut
    from): the kernel runs the restatement's operations with the device's expf and with each addend joined by a fused
    multiply-add, both within a small multiple of the restatement's own roundings."""
    model = _model(V, nz)
    q, g, ref, own = _arith_case(nz, metric)
    tol = 4.0 * own
    worst = 0.0
    for N in (1, 19):
        for G in (1, 5, 64):
            r = model.latent_topk((q[0][:N], q[1][:N]), (g[0][:G], g[1][:G]), k=G, metric=metric)
            assert r["index"].shape == (N, G) and r["index"].dtype == np.int32 and r["distance"].dtype == np.float32
            assert np.array_equal(np.sort(r["index"], 1), np.tile(np.arange(G, dtype=np.int32), (N, 1)))
            D = np.empty((N, G), np.float32)
            np.put_along_axis(D, r["index"].astype(np.int64), r["distance"], 1)
            worst = max(worst, _rel_err(D, ref[:N, :G], nz, metric).max())
            assert np.all(np.diff(r["distance"], axis=1) >= 0)
    print("n_z=%d %s: float32 restatement worst rel err %.3e, bound %.3e, kernel worst %.3e" % (nz, metric, own, tol, worst))
    assert worst <= tol


# ------------------------------------------------------------------------------------------------ 2. selection, exactly
N_MAX = 70


def _gallery(nz, G, seed):
    """Random gallery with bitwise duplicates (within a tile, across tiles, across splits; one of them of query 0), NaN means
    and infinite log-variances.  Queries: N_MAX random rows, query 1 a copy of a gallery row (distance exactly 0)."""
    rng = np.random.default_rng(seed)
    gm, gl = R.latents(rng, G, nz)
    qm, ql = R.latents(rng, N_MAX, nz)
    for src, dst in ((3, 2), (10, 700), (G - 1, 65), (500, 501), (40, G // 2), (G // 2 + 1, 41)):
        gm[dst], gl[dst] = gm[src], gl[src]
    for dst in (7, 300, G - 2):
        gm[dst], gl[dst] = qm[0], ql[0]                  # three bitwise copies of query 0: a three-way tie at distance 0
    gm[5, 0] = np.nan
    gm[G - 3, nz - 1] = np.nan
    gm[130] = np.nan
    gl[6, 1 % nz] = np.inf
    gl[G // 3] = np.inf
    qm[1], ql[1] = gm[64], gl[64]
    return (qm, ql), (gm, gl)


_D = {}


def _own_matrix(model, nz, G, metric):
    """(queries, gallery, D [N_MAX, G]): the kernel's own distances, from calls on gallery chunks of <= 64 rows with k = chunk
    size (chunks of different sizes, so tile tails of every length are among them)"""
    key = (nz, G, metric)
    if key not in _D:
        q, g = _gallery(nz, G, 7 * nz + G)
        dev = lambda a: torch.from_numpy(a).to(model.device)
        qd, gd = (dev(q[0]), dev(q[1])), (dev(g[0]), dev(g[1]))
        D = torch.empty((N_MAX, G), dtype=torch.float32, device=model.device)
        lo, sizes, i = 0, (64, 1, 37, 63, 5), 0
        while lo < G:
            n = min(sizes[i % len(sizes)], G - lo)
            r = model.latent_topk(qd, (gd[0][lo:lo + n], gd[1][lo:lo + n]), k=n, metric=metric)
            assert int(r["index"].min()) == 0 and int(r["index"].max()) == n - 1
            D[:, lo:lo + n].scatter_(1, r["index"].long(), r["distance"])
            lo, i = lo + n, i + 1
        _D[key] = (q, g, D.cpu().numpy())
    return _D[key]


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("nz,G", [(20, 1000), (20, 4099), (7, 4099), (64, 1000)])
def test_selection_is_the_total_order_of_the_kernels_own_distances(V, nz, G, metric):
    """G = 1000: 16 gallery tiles in 4 splits; G = 4099: 65 tiles (the last of 3 rows) in 17 splits; N = 70: two query tiles, the
    second of 6 rows (tests/test_retrieve_cpu.py pins these plan figures)."""
    model = _model(V, nz)
    q, g, D = _own_matrix(model, nz, G, metric)
    # the matrix itself: NaN where a NaN mean or an infinite log-variance meets the metric, exact zeros at the planted copies
    assert np.isnan(D[:, 5]).all() and np.isnan(D[:, 130]).all() and np.isnan(D[:, G - 3]).all()
    assert np.isnan(D[:, G // 3]).all() == (metric == "symkl")
    assert not _bits(D[0, [7, 300, G - 2]]).any() and not _bits(D[1, 64]).any()
    assert np.array_equal(_bits(D[:, 3]), _bits(D[:, 2])) and np.array_equal(_bits(D[:, 10]), _bits(D[:, 700]))
    for N in (1, 15, N_MAX):
        for k in (1, 5, 64):
            got = model.latent_topk((q[0][:N], q[1][:N]), g, k=k, metric=metric)
            want_i, want_d = R.topk(D[:N], k)
            assert np.array_equal(got["index"], want_i), (N, k, np.argwhere(got["index"] != want_i)[:4].tolist())
            assert np.array_equal(_bits(got["distance"]), _bits(want_d)), (N, k)
    top = model.latent_topk((q[0][:2], q[1][:2]), g, k=5, metric=metric)["index"]
    assert top[0, :3].tolist() == [7, 300, G - 2]                   # equal distances: the lower index first, across splits
    assert top[1, 0] == 64


# ------------------------------------------------------------------------------------------------ 3. split independence
@pytest.mark.parametrize("metric", R.METRICS)
def test_result_does_not_depend_on_rows_splits_stream_or_repetition(V, metric):
    """rows = 1 cuts the gallery of 4099 rows into 17 splits of 4 tiles; 300 queries are five query tiles over the same splits,
    20000 queries go in two chunks of launches, 256 query tiles over four splits of 17 tiles in the first."""
    model = _model(V, 20)
    rng = np.random.default_rng(5)
    q, g = R.latents(rng, 20000, 20), R.latents(rng, 4099, 20)
    dev = lambda a: torch.from_numpy(a).to(model.device)
    qd, gd = (dev(q[0]), dev(q[1])), (dev(g[0]), dev(g[1]))
    cut = lambda r, rows: {k: v[rows].cpu().numpy() for k, v in r.items()}
    big = model.latent_topk(qd, gd, k=64, metric=metric)
    one = model.latent_topk((qd[0][:1], qd[1][:1]), gd, k=64, metric=metric)
    mid = model.latent_topk((qd[0][:300], qd[1][:300]), gd, k=64, metric=metric)
    assert _same(cut(one, slice(0, 1)), cut(big, slice(0, 1))) and _same(cut(one, slice(0, 1)), cut(mid, slice(0, 1)))
    assert _same(cut(mid, slice(0, 300)), cut(big, slice(0, 300)))
    last = model.latent_topk((qd[0][19999:], qd[1][19999:]), gd, k=64, metric=metric)          # a row of the second chunk
    assert _same(cut(last, slice(0, 1)), cut(big, slice(19999, 20000)))
    again = model.latent_topk(qd, gd, k=64, metric=metric)
    assert _same(cut(again, slice(None)), cut(big, slice(None)))
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    with torch.cuda.stream(side):
        other = model.latent_topk((qd[0][:300], qd[1][:300]), gd, k=64, metric=metric)
    side.synchronize()
    assert _same(cut(other, slice(None)), cut(mid, slice(None)))


# ------------------------------------------------------------------------------------------------ 4. edges and errors
def test_edges_and_errors_of_the_c_abi(V):
    model = _model(V, 20)
    L, h, dev = model._L, model._h, model.device
    rng = np.random.default_rng(9)
    q, g = R.latents(rng, 6, 20), R.latents(rng, 40, 20)
    g[0][[3, 17, 30]] = np.nan                                       # three NaN rows: behind every number, in index order
    t = lambda a: torch.from_numpy(a).to(dev)
    qm, ql, gm, gl = t(q[0]), t(q[1]), t(g[0]), t(g[1])

    def call(qm_, ql_, rows, gm_, gl_, G, metric, k, index, dist):
        p = lambda x: None if x is None else x.data_ptr()
        rc = L.avae_latent_topk(h, p(qm_), p(ql_), rows, p(gm_), p(gl_), G, metric, k, p(index), p(dist), None)
        torch.cuda.synchronize()
        return rc

    def outs(rows, k):
        return (torch.full((rows, k), -7, dtype=torch.int32, device=dev), torch.full((rows, k), -7.0, dtype=torch.float32, device=dev))
    # k > G: the tail is -1 / +Inf; NaN distances sit between the numbers and the padding
    idx, dist = outs(6, 64)
    assert call(qm, ql, 6, gm, gl, 40, 0, 64, idx, dist) == 0
    i_np, d_np = idx.cpu().numpy(), dist.cpu().numpy()
    assert (i_np[:, 40:] == -1).all() and np.isposinf(d_np[:, 40:]).all()
    assert (i_np[:, 37:40] == [3, 17, 30]).all() and np.isnan(d_np[:, 37:40]).all() and np.isfinite(d_np[:, :37]).all()
    D = np.full((6, 40), np.nan, np.float32)
    np.put_along_axis(D, i_np[:, :40].astype(np.int64), d_np[:, :40], 1)
    want_i, want_d = R.topk(D, 64)
    assert np.array_equal(i_np, want_i) and np.array_equal(_bits(d_np), _bits(want_d))
    # either output alone
    idx2, dist2 = outs(6, 64)
    assert call(qm, ql, 6, gm, gl, 40, 0, 64, idx2, None) == 0 and call(qm, ql, 6, gm, gl, 40, 0, 64, None, dist2) == 0
    assert torch.equal(idx2, idx) and np.array_equal(_bits(dist2.cpu().numpy()), _bits(d_np))
    assert call(qm, ql, 6, gm, gl, 40, 0, 64, None, None) == 0
    # rows = 0: nothing is written, nothing is read (NULL inputs are fine)
    idx3, dist3 = outs(2, 3)
    assert call(None, None, 0, gm, gl, 40, 0, 3, idx3, dist3) == 0 and call(qm, ql, 0, None, None, 0, 0, 3, idx3, dist3) == 0
    assert (idx3 == -7).all() and (dist3 == -7.0).all()
    # an empty gallery: all -1 / +Inf, no gallery pointer needed
    assert call(qm, ql, 2, None, None, 0, 0, 3, idx3, dist3) == 0
    assert (idx3 == -1).all() and torch.isposinf(dist3).all()
    # l2 never reads a log-variance
    idx4, dist4 = outs(6, 5)
    assert call(qm, None, 6, gm, None, 40, 1, 5, idx4, dist4) == 0
    idx5, dist5 = outs(6, 5)
    junk = torch.full_like(ql, float("nan"))
    assert call(qm, junk, 6, gm, torch.full_like(gl, float("nan")), 40, 1, 5, idx5, dist5) == 0
    assert torch.equal(idx4, idx5) and np.array_equal(_bits(dist4.cpu().numpy()), _bits(dist5.cpu().numpy()))
    want = R.dist64((q[0], None), (g[0], None), "l2")
    assert np.array_equal(idx4.cpu().numpy(), R.topk(want, 5)[0])
    # errors: nonzero, a message that names the argument, outputs untouched
    idx6, dist6 = outs(6, 5)
    for args, needle in (((qm, ql, 6, gm, gl, 40, 0, 0, idx6, dist6), "k = 0"),
                         ((qm, ql, 6, gm, gl, 40, 0, 65, idx6, dist6), "k = 65"),
                         ((qm, ql, 6, gm, gl, 40, 2, 5, idx6, dist6), "metric"),
                         ((qm, ql, 6, gm, gl, 40, -1, 5, idx6, dist6), "metric"),
                         ((None, ql, 6, gm, gl, 40, 0, 5, idx6, dist6), "q_mu_dev"),
                         ((qm, ql, 6, None, gl, 40, 1, 5, idx6, dist6), "g_mu_dev"),
                         ((qm, None, 6, gm, gl, 40, 0, 5, idx6, dist6), "q_logvar_dev"),
                         ((qm, ql, 6, gm, None, 40, 0, 5, idx6, dist6), "g_logvar_dev"),
                         ((qm, ql, -1, gm, gl, 40, 0, 5, idx6, dist6), "rows"),
                         ((qm, ql, 6, gm, gl, -1, 0, 5, idx6, dist6), "gallery_rows")):
        assert call(*args) != 0, needle
        assert needle in L.avae_last_error(h).decode(), needle
    assert (idx6 == -7).all() and (dist6 == -7.0).all()
    # ... and the handle still works
    idx7, dist7 = outs(6, 64)
    assert call(qm, ql, 6, gm, gl, 40, 0, 64, idx7, dist7) == 0 and torch.equal(idx7, idx)


# ------------------------------------------------------------------------------------------------ 5. Python
def test_python_surface(V):
    nz, N = 20, 37
    model = _model(V, nz, fresh=True, ema=0.9)
    rng = np.random.default_rng(13)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    for i in range(3):                                               # a few steps, so that the average differs from the weights
        model.partial_fit([x[:B] for x in X], rng.standard_normal((B, nz)).astype(np.float32))
    post = model.posterior(X)
    mus = model.transform(X)
    assert len(post) == 2 and all(len(p) == 2 for p in post)
    for m in range(2):
        assert np.array_equal(_bits(post[m][0]), _bits(mus[m])) and post[m][1].shape == (N, nz)
        one = model.posterior(X[m], m)
        assert np.array_equal(_bits(one[0]), _bits(post[m][0])) and np.array_equal(_bits(one[1]), _bits(post[m][1]))
    # retrieve == latent_topk on posterior's outputs; tensors in, tensors out
    for metric in R.METRICS:
        a = model.retrieve(X[0], 0, post[1], k=5, metric=metric)
        assert _same(a, model.latent_topk(post[0], post[1], k=5, metric=metric))
        assert a["index"].shape == (N, 5) and a["index"].dtype == np.int32
    gal = tuple(torch.from_numpy(p).to(model.device) for p in post[1])
    d = model.retrieve(torch.from_numpy(X[0]).to(model.device), 0, gal, k=5)
    assert torch.is_tensor(d["index"]) and d["index"].is_cuda and d["index"].dtype == torch.int32 and d["distance"].is_cuda
    assert _same({k: v.cpu().numpy() for k, v in d.items()}, model.retrieve(X[0], 0, post[1], k=5))
    assert _same(model.latent_topk((post[0][0], None), (post[1][0], None), k=3, metric="l2"),
                 model.latent_topk(post[0], post[1], k=3, metric="l2"))
    with pytest.raises(ValueError, match="logvar"):
        model.latent_topk((post[0][0], None), post[1], k=3)
    with pytest.raises(ValueError, match="k must"):
        model.latent_topk(post[0], post[1], k=65)
    # the pair (n, n) against the assoc column of score_samples, at test 1's tolerance (n_z = 20, symkl), same denominator
    full = model.latent_topk(post[0], post[1], k=N)
    D = np.empty((N, N), np.float32)
    np.put_along_axis(D, full["index"].astype(np.int64), full["distance"], 1)
    assoc = model.score_samples(X, eps=np.zeros((N, nz), np.float32))["assoc"][:, 0]
    ref = R.dist64(post[0], post[1], "symkl")
    tol = 4.0 * _arith_case(nz, "symkl")[3]
    e_diag = (np.abs(np.diag(D).astype(np.float64) - assoc) / (np.diag(ref) + nz)).max()
    e_all = _rel_err(D, ref, nz, "symkl").max()
    print("posteriors: latent_topk against float64 %.3e; pair (n, n) against score_samples' assoc %.3e (bound %.3e)" % (e_all, e_diag, tol))
    assert e_all <= tol and e_diag <= tol
    # recall: the reference computed from the kernel's own matrices
    ks = (1, 5, 10)
    got = model.retrieval_recall(X, ks=ks)
    assert got.shape == (2, 2, 3) and got.dtype == np.float64
    for s in range(2):
        for t in range(2):
            r = model.latent_topk(post[s], post[t], k=N)
            Dst = np.empty((N, N), np.float32)
            np.put_along_axis(Dst, r["index"].astype(np.int64), r["distance"], 1)
            assert np.array_equal(got[s, t], R.recall(Dst, ks)), (s, t)
    assert np.all(got[0, 0] == 1.0) and np.all(got[1, 1] == 1.0)     # distinct rows: everyone finds itself first
    assert np.all(np.diff(got, axis=2) >= 0)
    l2 = model.retrieval_recall(X, ks=(1, 64), metric="l2")
    assert l2.shape == (2, 2, 2) and np.all(l2[:, :, 1] == 1.0)      # N = 37 <= 64: the partner is always among the first 64
    with pytest.raises(ValueError, match="ks"):
        model.retrieval_recall(X, ks=(1, 65))
    # inside averaged(): the averaged encoders' posteriors, looked up the same way
    with model.averaged():
        avg_post = model.posterior(X)
        in_avg = model.retrieve(X[0], 0, avg_post[1], k=5)
        rec_avg = model.retrieval_recall(X, ks=ks)
        given = model.latent_topk(post[0], post[1], k=5)             # given latents: the switch changes nothing
    assert not np.array_equal(_bits(avg_post[0][0]), _bits(post[0][0]))
    assert _same(in_avg, model.latent_topk(avg_post[0], avg_post[1], k=5))
    assert _same(given, model.latent_topk(post[0], post[1], k=5))
    assert rec_avg.shape == (2, 2, 3) and np.all(rec_avg[0, 0] == 1.0)
    assert np.array_equal(_bits(model.posterior(X)[0][0]), _bits(post[0][0]))                 # switched back


# ------------------------------------------------------------------------------------------------ 6. no side effects
def test_retrieve_has_no_side_effects_on_training(V):
    nz = 20
    rng = np.random.default_rng(21)
    Xt = synth_batch(rng, 2 * B, WIDTHS, [True, False])
    et = rng.standard_normal((2 * B, nz)).astype(np.float32)
    Xq = synth_batch(rng, 19, WIDTHS, [True, False])
    gal = R.latents(rng, 1000, nz)
    state = lambda m: m.get_opt_state() + (m.get_params(), m.cost_history(1))
    runs = []
    for with_calls in (False, True):
        model = _model(V, nz, fresh=True)
        model.partial_fit([x[:B] for x in Xt], et[:B])
        before = state(model)
        if with_calls:
            model.retrieve(Xq[0], 0, gal, k=5)
            model.retrieve(Xq[1], 1, gal, k=64, metric="l2")
            model.retrieval_recall(Xq, ks=(1, 5))
            model.synchronize()
            for x, y in zip(before, state(model)):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        cost = model.partial_fit([x[B:] for x in Xt], et[B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append((np.float32(cost), model.get_grads()) + state(model))
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x), np.asarray(y))
