"""latent_stats / avae_latent_stats on a real MI355X (include/avae.h) against tests/latent_stats_reference.py.

1. arithmetic: every statistic on the input families A, B, C x rows in {1, 2, 65, 4099, 20000}, M = 2, against the float64
   definition, within 4x the float32 restatement's worst error over the same cases (per statistic and n_z), and -- for the mean
   and the second moments, which the kernel forms in fp64 on shifted values -- within a fixed 4e-6; one row gives exact zeros and
   the row itself;
2. masks (a modality present in a single row, an empty intersection, a NULL modality, NaN in every absent entry);
3. sub-problem independence and determinism; 4. containment of non-finite values; 5. edges and errors of the C ABI;
6. the Python surface; 7. no side effects on training.

batch_size = 16, small MLPs, n_z in {7, 20, 64}, fp32."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import latent_stats_reference as R
from conftest import make_arch, shadow_err, synth_batch

pytestmark = pytest.mark.gpu

B = 16
WIDTHS = (784, 147)
# Mean, var, xcov and cov come out of fp64 sums of values shifted by a row of the data, so their error is a few fp64 roundings
# times (1 + k^2), k the shift's distance from the mean in standard deviations; the Gram's factors are rounded to fp32 once, 2^-24
# each, 1.2e-7 per product.  With k <= 5 that is at most 1.2e-7 * 26 = 3.1e-6 in the worst case of every rounding aligned.
SHIFTED_FP64_BOUND = 4e-6


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V, nz, fresh=False, **kw):
    """one fp32 relu model per n_z, shared by the tests that only hand latents in"""
    if fresh or nz not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, nz), make_arch("joint", 147, 72, 40, nz)]
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          learning_rate=1e-3, batch_size=B, compute_dtype="fp32", device=0, seed=3, **kw)
        if fresh:
            return m
        _MODELS[nz] = m
    return _MODELS[nz]


def _plan(model, rows):
    rt, ns = C.c_int32(-1), C.c_int32(-1)
    assert model._L.avae_latent_stats_plan(C.byref(model._cfg), rows, C.byref(rt), C.byref(ns), None) == 0
    return rt.value, ns.value


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, names=R.NAMES):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in names)


def _dev(model, post):
    return [None if p is None else tuple(torch.from_numpy(a).to(model.device) for a in p) for p in post]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _within(err, tol):
    return all(err[k] <= tol[k] for k in tol) and all(err[k] <= SHIFTED_FP64_BOUND for k in ("mean", "var", "xcov", "cov"))


# ------------------------------------------------------------------------------------------------ 1. arithmetic
@pytest.mark.parametrize("nz", R.NZS)
def test_every_statistic_against_the_float64_definition(V, nz):
    model = _model(V, nz)
    for rows in (4099, 20000):                                       # several slices, the last one ragged
        rt, ns = _plan(model, rows)
        assert ns >= 3 and rows % rt != 0 and (ns - 1) * rt < rows <= ns * rt
    tol, own = R.bound(nz)
    worst = {k: 0.0 for k in tol}
    for name in R.FAMILIES:
        for rows in R.ROWS:
            post, ref, _ = R.case(name, rows, nz)
            got = model.latent_stats(post)
            assert all(isinstance(got[k], np.ndarray) for k in R.NAMES) and got["count"].dtype == np.int64
            assert got["mean"].shape == (2, 2, nz) and got["kl"].shape == (2, nz) and got["cov"].shape == (2, nz, nz)
            assert (got["count"] == rows).all()
            for k, e in R.errors(got, ref).items():
                worst[k] = max(worst[k], e)
            assert not _bits(got["assoc"][[0, 1], [0, 1]]).any()                                  # the diagonal: exactly +0.0
            assert np.array_equal(_bits(got["xcov"][[0, 1], [0, 1]]), _bits(got["var"][[0, 1], [0, 1]]))
            assert np.array_equal(got["cov"], np.swapaxes(got["cov"], 1, 2))
            if rows == 1:
                for k in ("var", "xcov", "cov"):
                    assert not _bits(got[k]).any(), k                                              # exactly +0.0
                for s in range(2):
                    for d in range(2):
                        assert np.array_equal(got["mean"][s, d], post[s][0][0].astype(np.float64))
    for k in tol:
        print("n_z=%d %-8s float32 restatement worst %.3e, bound %.3e, kernel worst %.3e" % (nz, k, own[k], tol[k], worst[k]))
    assert _within(worst, tol), worst


# ------------------------------------------------------------------------------------------------ 2. masks
def _masked_case(nz=20, rows=4099, seed=11):
    """M = 4: modalities 0 and 1 on random rows, modality 2 on the single row 1234 (which modality 1 lacks: the pair (1, 2) is
    empty), modality 3 given to the reference as None.  NaN in every absent entry."""
    rng = np.random.default_rng(seed)
    post = R.family(rng, "A", rows, nz, n_mod=4)
    present = rng.random((rows, 4)) < 0.7
    present[:, 2] = False
    present[1234, 2] = True
    present[1234, 1] = False
    present[1234, 0] = True
    for m in range(4):
        post[m][0][~present[:, m]] = np.nan
        post[m][1][~present[:, m]] = np.nan
    return post, present


def test_masks_against_the_float64_definition(V):
    nz = 20
    model = _model(V, nz)
    post, present = _masked_case(nz)
    null3 = post[:3] + [None]
    ref = R.stats64(null3, present)
    got = model.latent_stats(null3, present)
    assert np.array_equal(got["count"], ref["count"])
    assert got["count"][2, 2] == 1 and got["count"][1, 2] == 0 and got["count"][0, 2] == 1 and not got["count"][3].any()
    err = R.errors(got, ref)
    tol, _ = R.bound(nz)
    print("masked: kernel worst", {k: "%.3e" % v for k, v in err.items()})
    assert _within(err, tol), err
    # empty sets: count 0 and NaN; the single row: exact
    for k in R.TABLES:
        assert np.isnan(got[k][1, 2]).all() and np.isnan(got[k][2, 1]).all() and np.isnan(got[k][3]).all() and np.isnan(got[k][:, 3]).all()
    assert np.isnan(got["post_var"][3]).all() and np.isnan(got["kl"][3]).all() and np.isnan(got["cov"][3]).all()
    assert not _bits(got["var"][2, 2]).any() and not _bits(got["cov"][2]).any() and not _bits(got["xcov"][0, 2]).any()
    assert np.array_equal(got["mean"][2, 0], post[2][0][1234].astype(np.float64))
    assert np.array_equal(got["mean"][0, 2], post[0][0][1234].astype(np.float64))
    # the flag column of a modality that is not given is never looked at; garbage in absent entries changes nothing
    flags3 = present.copy()
    flags3[:, 3] = True
    assert _same(model.latent_stats(null3, flags3), got)
    filled = [(np.where(np.isnan(mu), np.float32(7.0), mu), np.where(np.isnan(lv), np.float32(-1.0), lv)) for mu, lv in post[:3]] + [None]
    assert _same(model.latent_stats(filled, present), got)
    # all-ones flags are present=None, bit for bit
    full = R.family(np.random.default_rng(12), "B", 4099, nz, n_mod=3)
    assert _same(model.latent_stats(full, np.ones((4099, 3), bool)), model.latent_stats(full))


# ------------------------------------------------------------------------------------------------ 3. independence, determinism
def test_entries_depend_on_their_own_modalities_only_and_repeat_bit_for_bit(V):
    nz, rows, M = 20, 4099, 4
    model = _model(V, nz)
    rng = np.random.default_rng(17)
    post = R.family(rng, "C", rows, nz, n_mod=M)
    present = rng.random((rows, M)) < 0.6
    pd = _dev(model, post)
    fl = torch.from_numpy(present).to(model.device)
    big = _np(model.latent_stats(pd, fl))
    assert (big["count"] > 0).all() and len(set(big["count"].ravel().tolist())) > 4
    for sub in [(m,) for m in range(M)] + list(itertools.combinations(range(M), 2)) + [(3, 1)]:
        small = _np(model.latent_stats([pd[m] for m in sub], fl[:, list(sub)]))
        ix = np.array(sub)
        assert np.array_equal(small["count"], big["count"][np.ix_(ix, ix)]), sub
        for k in R.TABLES:
            assert np.array_equal(_bits(small[k]), _bits(big[k][np.ix_(ix, ix)])), (sub, k)
        for k in R.PER_MOD + ("cov",):
            assert np.array_equal(_bits(small[k]), _bits(big[k][ix])), (sub, k)
    assert _same(_np(model.latent_stats(pd, fl)), big)
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    with torch.cuda.stream(side):
        other = model.latent_stats(pd, fl)
    side.synchronize()
    assert _same(_np(other), big)


# ------------------------------------------------------------------------------------------------ 4. non-finite containment
def test_a_non_finite_value_stays_in_its_column(V):
    """Row 256 is the first row of the second slice: its values are that slice's shifts."""
    nz, rows = 20, 4099
    model = _model(V, nz)
    assert _plan(model, rows)[0] == 256
    clean = R.family(np.random.default_rng(23), "A", rows, nz)
    spots = ((0, "mu", 256, 3, np.nan), (0, "lv", 2000, 5, np.inf), (1, "lv", 300, 7, -np.inf))
    bad = [(mu.copy(), lv.copy()) for mu, lv in clean]
    zero = [(mu.copy(), lv.copy()) for mu, lv in clean]
    for m, which, r, j, v in spots:
        bad[m][which == "lv"][r, j] = v
        zero[m][which == "lv"][r, j] = 0.0
    a, b = model.latent_stats(bad), model.latent_stats(zero)
    may = {k: np.zeros(a[k].shape, bool) for k in R.NAMES}
    for m, _, _, j, _ in spots:
        for k in R.TABLES:
            may[k][m, :, j] = True
            may[k][:, m, j] = True
        for k in R.PER_MOD:
            may[k][m, j] = True
        may["cov"][m, j, :] = True
        may["cov"][m, :, j] = True
    for k in R.NAMES:
        differs = _bits(a[k]) != _bits(b[k])
        assert not (differs & ~may[k]).any(), (k, np.argwhere(differs & ~may[k])[:4].tolist())
    assert np.isnan(a["mean"][0, 0, 3]) and np.isnan(a["cov"][0, 3]).all() and np.isnan(a["xcov"][1, 0, 3])
    assert np.isposinf(a["post_var"][0, 5]) and not np.isfinite(a["assoc"][0, 1, 7])
    assert np.isfinite(b["cov"]).all() and all(np.isfinite(b[k]).all() for k in R.TABLES + R.PER_MOD)


# ------------------------------------------------------------------------------------------------ 5. edges and errors
def test_edges_and_errors_of_the_c_abi(V):
    from vae_assoc_amd import _capi
    nz, rows, M = 20, 300, 2
    model = _model(V, nz)
    L, h, dev = model._L, model._h, model.device
    post = _dev(model, R.family(np.random.default_rng(29), "A", rows, nz))
    shapes = {"count": (M, M), "mean": (M, M, nz), "var": (M, M, nz), "xcov": (M, M, nz), "assoc": (M, M, nz),
              "post_var": (M, nz), "kl": (M, nz), "cov": (M, nz, nz)}

    def outs(names=R.NAMES):
        return {k: torch.full(shapes[k], -7, dtype=torch.int64 if k == "count" else torch.float64, device=dev) for k in names}

    def call(n_mod, mus, lvs, present, n_rows, o, null_out=False):
        arr = lambda ts: None if ts is None else (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
        st = _capi.LatentStatsOut(**{k: t.data_ptr() for k, t in o.items()})
        rc = L.avae_latent_stats(h, n_mod, arr(mus), arr(lvs), None if present is None else present.data_ptr(), n_rows,
                                 None if null_out else C.byref(st), None)
        torch.cuda.synchronize()
        return rc
    mus, lvs = [p[0] for p in post], [p[1] for p in post]
    full = outs()
    assert call(M, mus, lvs, None, rows, full) == 0
    want = model.latent_stats(post)
    assert _same(_np(full), _np(want))
    # each output alone, then none at all
    for k in R.NAMES:
        one = outs((k,))
        assert call(M, mus, lvs, None, rows, one) == 0
        assert np.array_equal(_bits(one[k].cpu().numpy()), _bits(full[k].cpu().numpy())), k
    assert call(M, mus, lvs, None, rows, {}) == 0
    # rows = 0: count 0, NaN everywhere else; no input pointer is read
    empty = outs()
    assert call(M, [None, None], [None, None], None, 0, empty) == 0 and call(M, mus, lvs, None, 0, empty) == 0
    assert not empty["count"].any() and all(torch.isnan(empty[k]).all() for k in R.NAMES[1:])
    # errors: nonzero, a message that names the argument, outputs untouched
    kept = outs()
    for args, needle in (((0, mus, lvs, None, rows, kept), "n_mod = 0"),
                         ((5, mus + mus + mus, lvs + lvs + lvs, None, rows, kept), "n_mod = 5"),
                         ((M, mus, lvs, None, -1, kept), "rows"),
                         ((M, mus, lvs, None, rows, kept, True), "out is NULL"),
                         ((M, mus, [lvs[0], None], None, rows, kept), "logvar_dev[1]"),
                         ((M, mus, None, None, rows, kept), "logvar_dev[0]"),
                         ((M, None, lvs, None, rows, kept), "mu_dev")):
        assert call(*args) != 0, needle
        assert needle in L.avae_last_error(h).decode(), (needle, L.avae_last_error(h).decode())
    assert (kept["count"] == -7).all() and all((kept[k] == -7.0).all() for k in R.NAMES[1:])
    # ... and the handle still works
    again = outs()
    assert call(M, mus, lvs, None, rows, again) == 0 and _same(_np(again), _np(full))


# ------------------------------------------------------------------------------------------------ 6. Python
def test_python_surface(V):
    nz, N = 20, 37
    model = _model(V, nz, fresh=True, ema=0.9)
    rng = np.random.default_rng(13)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    for i in range(3):                                               # a few steps, so that the average differs from the weights
        model.partial_fit([x[:B] for x in X], rng.standard_normal((B, nz)).astype(np.float32))
    post = model.posterior(X)
    st = model.latent_stats(post)
    dg = model.latent_diagnostics(X)
    assert _same(dg, st) and all(isinstance(v, np.ndarray) for v in dg.values())
    own = st["var"][[0, 1], [0, 1]]
    assert dg["active"].dtype == np.bool_ and np.array_equal(dg["active"], own > 0.01)
    assert np.array_equal(dg["active_units"], (own > 0.01).sum(1)) and dg["active_units"].shape == (2,)
    assert np.array_equal(model.latent_diagnostics(X, au_threshold=1e9)["active_units"], [0, 0])
    prod = st["var"] * np.swapaxes(st["var"], 0, 1)
    with np.errstate(all="ignore"):
        corr = np.where(prod > 0, st["xcov"] / np.sqrt(prod), np.nan)
    assert np.allclose(dg["corr"], corr, rtol=1e-14, atol=0, equal_nan=True)
    own_corr = dg["corr"][[0, 1], [0, 1]]
    assert np.array_equal(np.isnan(own_corr), own == 0) and np.allclose(own_corr[own > 0], 1.0, atol=1e-14)
    assert np.array_equal(_bits(dg["agg_cov"]), _bits(st["cov"] + np.stack([np.diag(v) for v in st["post_var"]])))
    # tensors in, tensors out
    Xd = [torch.from_numpy(x).to(model.device) for x in X]
    dt = model.latent_diagnostics(Xd)
    assert all(torch.is_tensor(v) and v.is_cuda for v in dt.values()) and dt["count"].dtype == torch.int64 and dt["cov"].dtype == torch.float64
    assert _same(_np(dt), dg, dg.keys() - {"corr"}) and np.allclose(dt["corr"].cpu().numpy(), dg["corr"], rtol=1e-14, equal_nan=True)
    # a modality left out, with and without flags
    flags = rng.random((N, 2)) < 0.7
    half = model.latent_diagnostics([X[0], None], flags)
    assert _same(half, model.latent_stats([post[0], None], flags)) and half["active_units"][1] == 0 and np.isnan(half["corr"][0, 1]).all()
    with pytest.raises(ValueError, match="logvar"):
        model.latent_stats([(post[0][0], None), post[1]])
    # against the float64 definition and against the row means of score_samples' terms, at test 1's bound
    tol, _ = R.bound(nz)
    err = R.errors(st, R.stats64(post))
    assert _within(err, tol), err
    sc = model.score_samples(X, eps=np.zeros((N, nz), np.float32))
    e_assoc = abs(st["assoc"][0, 1].sum() - sc["assoc"][:, 0].astype(np.float64).mean()) / (st["assoc"][0, 1] + 1.0).sum()
    e_kl = [abs(st["kl"][m].sum() - sc["latent"][:, m].astype(np.float64).mean()) / (st["kl"][m] + 1.0).sum() for m in range(2)]
    print("posteriors: against float64", {k: "%.2e" % v for k, v in err.items()}, "assoc against score_samples %.3e (bound %.3e), "
          "kl %.3e %.3e (bound %.3e)" % (e_assoc, tol["assoc"], e_kl[0], e_kl[1], tol["kl"]))
    assert e_assoc <= tol["assoc"] and max(e_kl) <= tol["kl"]
    # inside averaged(): the averaged encoders
    with model.averaged():
        avg = model.latent_diagnostics(X)
        avg_post = model.posterior(X)
        given = model.latent_stats(post)                             # given latents: the switch changes nothing
    assert not np.array_equal(_bits(avg["mean"]), _bits(dg["mean"])) and _same(avg, model.latent_stats(avg_post))
    assert _same(given, st) and _same(model.latent_diagnostics(X), dg)                             # switched back


def test_active_units_of_a_model_under_a_large_kl_weight_follow_the_reference(V):
    """The kernel against the reference on what a diagnosis is for; the training outcome itself is asserted only where the
    float64 reference on the same posteriors says so too."""
    nz, N = 20, 64
    rng = np.random.default_rng(31)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    units = []
    for kw in ({}, dict(schedule=dict(kl=200.0))):
        model = _model(V, nz, fresh=True, **kw)
        if kw:
            for i in range(12):
                sel = rng.permutation(N)[:B]
                model.partial_fit([x[sel] for x in X], rng.standard_normal((B, nz)).astype(np.float32))
        post = model.posterior(X)
        dg = model.latent_diagnostics(X, au_threshold=0.01)
        ref = R.stats64(post)
        ref_units = (ref["var"][[0, 1], [0, 1]] > 0.01).sum(1)
        assert np.array_equal(dg["active_units"], ref_units)
        units.append((dg["active_units"].sum(), ref_units.sum()))
    print("active units (kernel, reference): untrained %s, after 12 steps at KL weight 200 %s" % units[0] + " %s" % (units[1],))
    if units[1][1] < units[0][1]:
        assert units[1][0] < units[0][0]


# ------------------------------------------------------------------------------------------------ 7. no side effects
def test_latent_stats_has_no_side_effects_on_training(V):
    nz = 20
    rng = np.random.default_rng(21)
    Xt = synth_batch(rng, 2 * B, WIDTHS, [True, False])
    et = rng.standard_normal((2 * B, nz)).astype(np.float32)
    Xq = synth_batch(rng, 19, WIDTHS, [True, False])
    lat = R.family(rng, "B", 1000, nz)
    state = lambda m: m.get_opt_state() + (m.get_params(), m.cost_history(1))
    runs = []
    for with_calls in (False, True):
        model = _model(V, nz, fresh=True)
        model.partial_fit([x[:B] for x in Xt], et[:B])
        before = state(model)
        if with_calls:
            model.latent_stats(lat)
            model.latent_stats([lat[0], None], rng.random((1000, 2)) < 0.5)
            model.latent_diagnostics(Xq)
            model.synchronize()
            for x, y in zip(before, state(model)):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        cost = model.partial_fit([x[B:] for x in Xt], et[B:])
        model.synchronize()
        assert shadow_err(model)[:2] == (0.0, 0.0)
        runs.append((np.float32(cost), model.get_grads()) + state(model))
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x), np.asarray(y))
