"""Sigma-lognormal strokes (avae_lognormal_eval / avae_lognormal_sample / avae_lognormal_fit, lognormal_eval / lognormal_fit /
lognormal_augment) on a real MI355X (include/avae.h) against tests/lognormal_reference.py.

1. eval, 2. the sampler and 3. the fit step for step (``tol = 0``, after 1 and 4 tries) against the float64 definition, within 4x
the float32 restatement's own worst error over the same inputs (the rule of test_gpu_motion.py; |err| / (|ref| + 1), paths of
fitted parameters as |err| / extent); 4. the fit's contract at the default options; 5. bit reproducibility and independence;
6. ``lognormal_augment`` end to end into ``strokes_to_motion``; 7. to 11. the second pass (tests/lognormal_cases.py): the fit
inside every tile and component class, the exits of its loop, its clips and weights, count NULL and out of range, the sampler's
edges.  The measured pairs are in README.md and DESIGN.md section 28."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_cases as IC
import lognormal_cases as LC
import lognormal_reference as LR
import render_reference as R
from conftest import make_arch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
START = np.asarray(LR.START_CASE, dtype=np.float32)
FIT_OUTPUTS = ("params", "loss0", "loss", "iterations", "accepted", "status")


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V):
    """one small fp32 relu model (the nets of test_gpu_render.py), shared by every test here"""
    if "m" not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS["m"] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3)
    return _MODELS["m"]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else (a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint8))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(model, a, dtype=torch.float32):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=model.device, dtype=dtype).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(model, stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream(model.device)).cuda_stream)


def _err(model):
    return model._L.avae_last_error(model._h).decode()


class _Out:
    """an output of -7s with ``guard`` rows of -7 before and behind it; ``t`` is what the call writes"""

    def __init__(self, model, shape, guard=0, dtype=torch.float32):
        self.whole = torch.full((shape[0] + 2 * guard,) + tuple(shape[1:]), -7, device=model.device, dtype=dtype)
        self.t = self.whole[guard:guard + shape[0]]
        self.guard = guard

    def numpy(self):
        g, w = self.guard, self.whole.cpu().numpy()
        assert (w[:g] == -7).all() and (w[len(w) - g:] == -7).all(), "an element outside the output was written"
        return w[g:len(w) - g]


def _eval(model, params, count, start, T, dt, velocity=True, stream=None, guard=0):
    """avae_lognormal_eval -> (path, velocity or None) as NumPy, prefilled with -7 (``count`` None: NULL; ``guard``: rows of -7
    around every output, asserted untouched)"""
    N, Cn = params.shape[0], params.shape[1]
    ts = [_dev(model, params), _dev(model, count, torch.int32), _dev(model, start)]
    path_o, vel_o = _Out(model, (N, T, 2), guard), _Out(model, (N, T, 2), guard) if velocity else None
    path, vel = path_o.t, vel_o.t if velocity else None
    torch.cuda.synchronize()                             # (the inputs and the prefill are there before another stream reads them)
    rc = model._L.avae_lognormal_eval(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, Cn, T, dt, _p(path), _p(vel), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return path_o.numpy(), None if vel is None else vel_o.numpy()


def _sample(model, params, count, start, T, dt, S, seed, shift, offset=0, want_params=True, stream=None,
            scales=(0.2, np.pi / 9, 0.1), guard=0):
    """avae_lognormal_sample -> (strokes [N, S, T, 2], perturbed [N, S, C, 6] or None) as NumPy, prefilled with -7"""
    N, Cn = params.shape[0], params.shape[1]
    ts = [_dev(model, params), _dev(model, count, torch.int32), _dev(model, start)]
    out_o, pert_o = _Out(model, (N, S, T, 2), guard), _Out(model, (N, S, Cn, 6), guard) if want_params else None
    out, pert = out_o.t, pert_o.t if want_params else None
    torch.cuda.synchronize()
    rc = model._L.avae_lognormal_sample(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, S, Cn, T, dt, seed, offset, scales[0],
                                        scales[1], scales[2], 1 if shift else 0, _p(out), _p(pert), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return out_o.numpy(), None if pert is None else pert_o.numpy()


def _fit(model, target, init, count, start, dt, n_iters=40, weights=LR.DEFAULT_WEIGHTS, tol=1e-9, free=None, bounds=None,
         want=FIT_OUTPUTS, stream=None, guard=0):
    """avae_lognormal_fit -> dict of the NumPy outputs asked for (``params`` always), prefilled with -7 (``bounds``: None or
    (lo, hi), either of them None for NULL)"""
    N, T, Cn = target.shape[0], target.shape[1], init.shape[1]
    ts = [_dev(model, target), _dev(model, init), _dev(model, count, torch.int32), _dev(model, start)]
    fr = _dev(model, free, torch.uint8)
    lo, hi = (None, None) if bounds is None else (None if b is None else _dev(model, np.asarray(b, dtype=np.float32)) for b in bounds)
    dts = dict(params=torch.float32, loss0=torch.float64, loss=torch.float64, iterations=torch.int32, accepted=torch.int32,
               status=torch.int32)
    outs = {k: _Out(model, (N, Cn, 6) if k == "params" else (N,), guard, dts[k]) for k in want}
    out = {k: v.t for k, v in outs.items()}
    torch.cuda.synchronize()
    rc = model._L.avae_lognormal_fit(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), N, Cn, T, dt, n_iters, weights[0],
                                     weights[1], tol, _p(fr), 1 if (fr is not None and fr.dim() == 3) else 0, _p(lo), _p(hi),
                                     _p(out["params"]), _p(out.get("loss0")), _p(out.get("loss")), _p(out.get("iterations")),
                                     _p(out.get("accepted")), _p(out.get("status")), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return {k: v.numpy() for k, v in outs.items()}


def _random_rows(N, Cn, seed):
    rng = np.random.default_rng(seed)
    return np.stack([LR.separated_params(Cn, rng) for _ in range(N)]).astype(np.float32)


def _dt(T):
    return float(np.float32(0.01 if T == 1 else 1.0 / (T - 1)))


# ------------------------------------------------------------------------------------------------ 1. eval
EVAL_SHAPES = [(1, 1, 1), (3, 3, 2), (5, 8, 63), (5, 8, 64), (2, 16, 65), (65, 3, 100), (2, 5, 257), (1, 2, 1024)]


@pytest.mark.parametrize("shape", EVAL_SHAPES)
def test_eval_against_the_definition(V, shape):
    model = _model(V)
    N, Cn, T = shape
    params, dt = _random_rows(N, Cn, sum(shape)), _dt(T)
    start = np.tile(START, (N, 1))
    count = np.full(N, Cn, dtype=np.int32)
    r64, r32 = LR.evaluate(params, count, start, T, dt), LR.evaluate_restated(params, count, start, T, dt)
    got = _eval(model, params, count, start, T, dt)
    for k, name in enumerate(("path", "velocity")):
        own, err = LR.rel_err(r32[k], r64[k]), LR.rel_err(got[k], r64[k])
        print("eval %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, name, err, own))
        assert got[k].shape == r64[k].shape and err <= 4.0 * own, name
    # velocity off, a row alone, the Python call
    assert _same(_eval(model, params, count, start, T, dt, velocity=False)[0], got[0])
    last = _eval(model, params[-1:], count[-1:], start[-1:], T, dt)
    assert _same(last[0], got[0][-1:]) and _same(last[1], got[1][-1:])
    py = model.lognormal_eval(params, T, start=start, dt=dt)
    assert isinstance(py["path"], np.ndarray) and _same(py["path"], got[0]) and _same(py["velocity"], got[1])


def test_eval_edges(V):
    """ragged counts with an empty row, a negative amplitude, a component that switches on mid-stroke, sigma = 0 (clamped), and a
    NaN parameter, which makes its own row NaN and no other"""
    model = _model(V)
    N, Cn, T, dt = 6, 4, 100, 0.01
    params = _random_rows(N, Cn, 5)
    count = np.array([4, 2, 0, 4, 4, 4], dtype=np.int32)
    start = (np.tile(START, (N, 1)) + np.arange(N, dtype=np.float32)[:, None]).astype(np.float32)
    params[0, 1, 0] = -0.8                               # D < 0
    params[3, 2, 1] = 0.5                                # t0 inside the time range: off until k = 50
    params[4, 0, 3] = 0.0                                # sigma = 0
    params[1, 3, 2] = np.nan                             # beyond count: never read
    r64, r32 = LR.evaluate(params, count, start, T, dt), LR.evaluate_restated(params, count, start, T, dt)
    got = _eval(model, params, count, start, T, dt)
    for k in range(2):
        own, err = LR.rel_err(r32[k], r64[k]), LR.rel_err(got[k], r64[k])
        print("eval edges %s: kernel %.3e, restatement %.3e" % (("path", "velocity")[k], err, own))
        assert np.isfinite(got[k]).all() and err <= 4.0 * own
    assert _same(got[0][2], np.broadcast_to(start[2], (T, 2)).astype(np.float32)) and not got[1][2].any()
    one = params[3:4].copy()
    one[0, :2] = 0.0
    one[0, 3, 0] = 0.0
    alone = _eval(model, one, count[3:4], start[3:4], T, dt)
    assert not alone[1][0, :50].any() and np.abs(alone[1][0, 52:]).max() > 0           # switched on at t0 = 0.5
    bad = params.copy()
    bad[3, 1, 4] = np.nan
    nan = _eval(model, bad, count, start, T, dt)
    assert np.isnan(nan[0][3]).all() and np.isnan(nan[1][3]).all()
    keep = [0, 1, 2, 4, 5]
    assert _same(nan[0][keep], got[0][keep]) and _same(nan[1][keep], got[1][keep])
    bad_start = start.copy()
    bad_start[5, 1] = np.inf
    nan = _eval(model, params, count, bad_start, T, dt)
    assert np.isnan(nan[0][5]).all() and _same(nan[0][:5], got[0][:5])


# ------------------------------------------------------------------------------------------------ 2. sample
SAMPLE_SHAPES = [(1, 1, 1, 2), (3, 10, 3, 100), (2, 7, 16, 65), (65, 2, 8, 64)]


@pytest.mark.parametrize("shape", SAMPLE_SHAPES)
def test_sample_against_the_definition(V, shape):
    model = _model(V)
    N, S, Cn, T = shape
    params, dt, seed = _random_rows(N, Cn, sum(shape)), _dt(T), 0x1234567855
    start = np.tile(START, (N, 1))
    count = np.full(N, Cn, dtype=np.int32)
    if N >= 3:
        count[1] = Cn - 1
    plain = None
    for shift in (False, True):
        r64 = LR.sample(params, count, start, T, dt, S, seed, shift_mean=shift)
        r32 = LR.sample_restated(params, count, start, T, dt, S, seed, shift_mean=shift)
        got = _sample(model, params, count, start, T, dt, S, seed, shift)
        for k, name in enumerate(("strokes", "perturbed")):
            own, err = LR.rel_err(r32[k], r64[k]), LR.rel_err(got[k], r64[k])
            print("sample %s shift_mean %s %s: kernel %.3e, restatement %.3e (bound 4x)" % (shape, shift, name, err, own))
            assert got[k].shape == r64[k].shape and err <= 4.0 * own, name
        # the strokes are avae_lognormal_eval of the returned parameters, bit for bit
        ev = _eval(model, got[1].reshape(N * S, Cn, 6), np.repeat(count, S), np.repeat(start, S, axis=0), T, dt, velocity=False)[0]
        ev = ev.reshape(N, S, T, 2)
        if shift:
            mean = np.stack([[LR.mean_restated(ev[n, s]) for s in range(S)] for n in range(N)])
            assert _same(got[0], (ev - mean[:, :, None, :]).astype(np.float32))
            assert _same(got[1], plain[1])
        else:
            assert _same(got[0], ev)
            plain = got
        assert _same(_sample(model, params, count, start, T, dt, S, seed, shift, want_params=False)[0], got[0])
    # another seed draws other samples
    other = _sample(model, params, count, start, T, dt, S, seed + 1, False)
    assert not np.array_equal(other[1][..., 0], plain[1][..., 0])


def test_sample_row_offset_and_python(V):
    model = _model(V)
    N, S, Cn, T, dt, seed = 5, 3, 4, 100, 0.01, 99
    params, start, count = _random_rows(N, Cn, 8), np.tile(START, (N, 1)), np.array([4, 3, 4, 1, 2], dtype=np.int32)
    whole = _sample(model, params, count, start, T, dt, S, seed, True)
    part = _sample(model, params[2:], count[2:], start[2:], T, dt, S, seed, True, offset=2)
    assert _same(part[0], whole[0][2:]) and _same(part[1], whole[1][2:])
    assert not np.array_equal(_sample(model, params[2:], count[2:], start[2:], T, dt, S, seed, True)[0], whole[0][2:])
    py = model.lognormal_augment(params=params, count=count, n_samples=S, seed=seed, start=start, dt=dt, n_points=T)
    assert _same(py["strokes"], whole[0]) and _same(py["perturbed"], whole[1]) and not py["status"].any()
    saved = model._lognormal_chunk
    try:
        model._lognormal_chunk = 2 * S                   # two rows a launch: the row offset keeps the stream
        chunked = model.lognormal_augment(params=params, count=count, n_samples=S, seed=seed, start=start, dt=dt, n_points=T)
    finally:
        model._lognormal_chunk = saved
    assert all(_same(chunked[k], py[k]) for k in py)
    zero = _sample(model, params, count, start, T, dt, S, seed, False, scales=(0.0, 0.0, 0.0))
    ev = _eval(model, params, count, start, T, dt, velocity=False)[0]
    assert _same(zero[0], np.broadcast_to(ev[:, None], zero[0].shape).copy())


# ------------------------------------------------------------------------------------------------ 3. the fit, step for step
_STEP_REFS = {}


def _step_refs(name, N, Cn, counts, variant):
    if name not in _STEP_REFS:
        case = LR.step_case(N, Cn, LR.step_seed(name), counts)
        _STEP_REFS[name] = (case, {it: (LR.run_step_case(case, variant, it, False), LR.run_step_case(case, variant, it, True))
                                   for it in (1, 4)})
    return _STEP_REFS[name]


def _path_err(params, count, ref_params, start):
    """worst |err| / extent of the float64 paths of ``params`` against those of ``ref_params``"""
    worst = 0.0
    for n in range(len(params)):
        a = LR.stroke(params[n, :count[n]], start[n], LR.T_CASE, LR.DT_CASE)[0]
        b = LR.stroke(ref_params[n, :count[n]], start[n], LR.T_CASE, LR.DT_CASE)[0]
        worst = max(worst, float(np.abs(a - b).max() / max(LR.extent(b), 1e-30)))
    return worst


@pytest.mark.parametrize("spec", LR.STEP_CASES, ids=[c[0] for c in LR.STEP_CASES])
def test_fit_step_for_step(V, spec):
    """``tol = 0``, after 1 and 4 tries, from the 10 % perturbation of the true parameters: tries and accepted steps equal the
    definition's, the loss and the float64 path of the returned parameters are within 4x the restatement's error; with one
    component the parameters themselves are."""
    model = _model(V)
    name, N, Cn, counts, variant = spec
    case, refs = _step_refs(*spec)
    free, bounds = LR.step_options(case, variant)
    for it in (1, 4):
        r64, r32 = refs[it]
        assert min(LR.margins(t) for t in r64["tries"]) > 1e-3                   # every decision compared is a clear one
        got = _fit(model, case["target"], case["init"], case["count"], case["start"], LR.DT_CASE, n_iters=it, tol=0.0, free=free,
                   bounds=bounds)
        assert np.array_equal(got["iterations"], r64["iterations"]) and np.array_equal(got["accepted"], r64["accepted"])
        assert np.array_equal(got["status"], r64["status"])
        assert np.array_equal(r32["accepted"], r64["accepted"])
        for k in ("loss0", "loss"):
            own, err = LR.rel_err(r32[k], r64[k]), LR.rel_err(got[k], r64[k])
            print("fit %s, %d tries, %s: kernel %.3e, restatement %.3e (bound 4x)" % (name, it, k, err, own))
            assert err <= 4.0 * own, k
        own = _path_err(r32["params"], case["count"], r64["params"], case["start"])
        err = _path_err(got["params"], case["count"], r64["params"], case["start"])
        print("fit %s, %d tries, path: kernel %.3e, restatement %.3e of the extent (bound 4x)" % (name, it, err, own))
        assert err <= 4.0 * own
        if Cn == 1:
            own, err = LR.rel_err(r32["params"], r64["params"]), LR.rel_err(got["params"], r64["params"])
            print("fit %s, %d tries, parameters: kernel %.3e, restatement %.3e" % (name, it, err, own))
            assert err <= 4.0 * own
        for n in range(N):                               # above count: zeros; a masked parameter keeps its bits
            assert not got["params"][n, case["count"][n]:].any()
            if free is not None:
                fr = np.broadcast_to(free if free.ndim == 3 else free[None, None, :], (N, Cn, 6))[n, :case["count"][n]] != 0
                assert _same(got["params"][n, :case["count"][n]][~fr], case["init"][n, :case["count"][n]][~fr])
        if bounds is not None:
            moved = got["params"] != case["init"]
            lo, hi = (np.asarray(b, dtype=np.float32) for b in bounds)
            assert ((got["params"] >= lo) & (got["params"] <= hi))[moved].all()


# ------------------------------------------------------------------------------------------------ 4. the fit's contract
@pytest.mark.parametrize("Cn", (1, 2, 3, 4, 6))
def test_fit_contract_at_the_defaults(V, Cn):
    """``init=None`` on four separated strokes: status 0 or 1, the rmse within 4x the restatement's own and, so that a broken
    solver cannot pass, under 1e-4 of the stroke's extent"""
    from vae_assoc_amd.lognormal import lognormal_initial_guess
    model = _model(V)
    strokes = np.stack([LR.contract_stroke(Cn, s)[0] for s in LR.CONTRACT_SEEDS[Cn]]).astype(np.float32)
    start = np.tile(START, (4, 1))
    out = model.lognormal_fit(strokes, start=start, dt=LR.DT_CASE)
    guess, cnt = lognormal_initial_guess(strokes, start, float(np.float32(LR.DT_CASE)))
    assert np.array_equal(out["count"], cnt) and (cnt == Cn).all() and out["params"].shape == (4, 8, 6)
    for n in range(4):
        r32 = LR.fit_row(strokes[n], guess[n, :Cn].astype(np.float32), start[n], LR.DT_CASE, restated=True)
        p32 = LR.stroke_restated(r32["params"], start[n], LR.T_CASE, LR.DT_CASE)[0]
        own = np.sqrt(((p32.astype(np.float64) - strokes[n]) ** 2).sum(1).mean())
        rmse = np.sqrt(((out["path"][n].astype(np.float64) - strokes[n]) ** 2).sum(1).mean())
        ext = LR.extent(strokes[n])
        print("fit contract C = %d seed %d: status %d after %d tries (%d accepted), rmse %.3e (restatement %.3e, status %d), extent "
              "%.3f" % (Cn, LR.CONTRACT_SEEDS[Cn][n], out["status"][n], out["iterations"][n], out["accepted"][n], rmse, own,
                        r32["status"], ext))
        assert out["status"][n] in (0, 1)
        assert rmse <= 4.0 * own and rmse < 1e-4 * ext
        assert abs(out["rmse"][n] - rmse) <= 1e-3 * rmse + 1e-9
        assert out["loss"][n] <= out["loss0"][n]
    ev = model.lognormal_eval(out["params"], LR.T_CASE, count=out["count"], start=start, dt=LR.DT_CASE)
    assert _same(ev["path"], out["path"])


def test_fit_bad_rows_and_rows_that_cannot_improve(V):
    model = _model(V)
    case = LR.step_case(5, 3, 21)
    good = _fit(model, case["target"], case["init"], case["count"], case["start"], LR.DT_CASE, n_iters=12)
    tgt, st, init = case["target"].copy(), case["start"].copy(), case["init"].copy()
    tgt[1, 40, 1] = np.nan
    st[3, 0] = np.nan
    bad = _fit(model, tgt, init, case["count"], st, LR.DT_CASE, n_iters=12)
    for n in (1, 3):
        assert np.isnan(bad["params"][n]).all() and np.isnan(bad["loss0"][n]) and np.isnan(bad["loss"][n])
        assert bad["status"][n] == 3 and bad["iterations"][n] == 0 and bad["accepted"][n] == 0
    keep = [0, 2, 4]
    assert all(_same(bad[k][keep], good[k][keep]) for k in FIT_OUTPUTS)
    init[2, 1, 5] = np.inf
    assert _fit(model, tgt, init, case["count"], st, LR.DT_CASE, n_iters=12)["status"].tolist() == [good["status"][0], 3, 3, 3,
                                                                                                  good["status"][4]]
    # every parameter masked out: no try can be accepted
    frozen = _fit(model, case["target"], case["init"], case["count"], case["start"], LR.DT_CASE, free=np.zeros(6, dtype=np.uint8))
    assert (frozen["status"] == 2).all() and (frozen["iterations"] == 8).all() and not frozen["accepted"].any()
    assert _same(frozen["params"], case["init"]) and _same(frozen["loss"], frozen["loss0"]) and _same(frozen["loss0"], good["loss0"])
    # nothing to fit: count = 0 stands still
    none = _fit(model, case["target"], case["init"], np.zeros(5, dtype=np.int32), case["start"], LR.DT_CASE)
    r64 = LR.fit(case["target"], case["init"], np.zeros(5, dtype=np.int32), case["start"], LR.DT_CASE)
    assert not none["status"].any() and not none["iterations"].any() and not none["params"].any()
    assert _same(none["loss"], none["loss0"]) and LR.rel_err(none["loss"], r64["loss"]) < 1e-5
    # tol ends a row with status 0 once an accepted step gains less than tol L
    early = _fit(model, case["target"], case["init"], case["count"], case["start"], LR.DT_CASE, n_iters=40, tol=0.5)
    assert (early["status"] == 0).all() and (early["iterations"] < 40).all()
    # errors of the C ABI leave a message and launch nothing
    t = _dev(model, case["target"])
    for args in ((-1, 3, 100, 0.01, 4), (5, 17, 100, 0.01, 4), (5, 3, 1025, 0.01, 4), (5, 3, 100, 0.0, 4), (5, 3, 100, 0.01, -1)):
        rc = model._L.avae_lognormal_fit(model._h, _p(t), _p(t), None, _p(t), args[0], args[1], args[2], args[3], args[4], 1.0, 1e-3,
                                         0.0, None, 0, None, None, _p(t), None, None, None, None, None, _stream(model))
        assert rc != 0 and "avae_lognormal_fit" in _err(model)


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_no_bit_depends_on_company_stream_repetition_chunks_or_outputs(V):
    model = _model(V)
    N, Cn, T, dt, S, seed = 65, 3, 100, 0.01, 2, 7
    case = LR.step_case(N, Cn, 31)
    params, count, start = case["true"], case["count"], case["start"]
    side = torch.cuda.Stream(device=model.device)
    # eval
    ev = _eval(model, params, count, start, T, dt)
    assert all(_same(a, b) for a, b in zip(_eval(model, params, count, start, T, dt), ev))
    assert all(_same(a, b) for a, b in zip(_eval(model, params, count, start, T, dt, stream=side), ev))
    assert _same(_eval(model, params[40:41], count[40:41], start[40:41], T, dt)[0], ev[0][40:41])
    # sample
    sm = _sample(model, params, count, start, T, dt, S, seed, True)
    assert all(_same(a, b) for a, b in zip(_sample(model, params, count, start, T, dt, S, seed, True), sm))
    assert all(_same(a, b) for a, b in zip(_sample(model, params, count, start, T, dt, S, seed, True, stream=side), sm))
    alone = _sample(model, params[40:41], count[40:41], start[40:41], T, dt, S, seed, True, offset=40)
    assert _same(alone[0], sm[0][40:41]) and _same(alone[1], sm[1][40:41])
    # fit
    ft = _fit(model, case["target"], case["init"], count, start, dt, n_iters=6)
    for again in (_fit(model, case["target"], case["init"], count, start, dt, n_iters=6),
                  _fit(model, case["target"], case["init"], count, start, dt, n_iters=6, stream=side)):
        assert all(_same(again[k], ft[k]) for k in FIT_OUTPUTS)
    alone = _fit(model, case["target"][40:41], case["init"][40:41], count[40:41], start[40:41], dt, n_iters=6)
    assert all(_same(alone[k], ft[k][40:41]) for k in FIT_OUTPUTS)
    for want in (("params",), ("params", "loss"), ("params", "status", "iterations")):
        part = _fit(model, case["target"], case["init"], count, start, dt, n_iters=6, want=want)
        assert all(_same(part[k], ft[k]) for k in want)
    # the Python calls in chunks of 16 rows
    whole = (model.lognormal_eval(params, T, count=count, start=start, dt=dt),
             model.lognormal_fit(case["target"], init=case["init"], count=count, start=start, dt=dt, n_iters=6))
    assert _same(whole[0]["path"], ev[0]) and all(_same(whole[1][k], ft[k]) for k in FIT_OUTPUTS)
    saved = model._lognormal_chunk
    try:
        model._lognormal_chunk = 16
        parts = (model.lognormal_eval(params, T, count=count, start=start, dt=dt),
                 model.lognormal_fit(case["target"], init=case["init"], count=count, start=start, dt=dt, n_iters=6))
    finally:
        model._lognormal_chunk = saved
    assert all(_same(parts[i][k], whole[i][k]) for i in range(2) for k in whole[i])
    dev = model.lognormal_fit(torch.from_numpy(case["target"]).to(model.device), init=torch.from_numpy(case["init"]).to(model.device),
                              count=torch.from_numpy(count).to(model.device), start=start, dt=dt, n_iters=6)
    assert all(torch.is_tensor(dev[k]) and _same(dev[k], whole[1][k]) for k in whole[1])


# ------------------------------------------------------------------------------------------------ 6. augment, end to end
def test_augment_end_to_end_into_strokes_to_motion(V):
    from vae_assoc_amd.kinematics import StrokeCanvas
    from vae_assoc_amd.motion import MotionBasis
    model = _model(V)
    strokes = np.stack([LR.contract_stroke(c, LR.CONTRACT_SEEDS[c][i])[0] for c, i in ((1, 0), (2, 0), (3, 0), (3, 1), (2, 1))])
    strokes = strokes.astype(np.float32)
    out = model.lognormal_augment(strokes, n_samples=4, seed=5, start=np.tile(START, (5, 1)), dt=LR.DT_CASE)
    assert out["strokes"].shape == (5, 4, 100, 2) and out["perturbed"].shape == (5, 4, 8, 6) and out["params"].shape == (5, 8, 6)
    assert np.isfinite(out["strokes"]).all() and np.isin(out["status"], (0, 1)).all()
    assert out["count"].tolist() == [1, 2, 3, 3, 2]
    assert np.abs(out["strokes"].astype(np.float64).mean(axis=2)).max() < 1e-5
    for n in range(5):
        ext = LR.extent(strokes[n])
        for s in range(4):
            assert 0.5 * ext <= LR.extent(out["strokes"][n, s]) <= 2.0 * ext
    again = model.lognormal_augment(strokes, n_samples=4, seed=5, start=np.tile(START, (5, 1)), dt=LR.DT_CASE)
    assert all(_same(again[k], out[k]) for k in out)
    # a row that cannot be fitted comes back as NaN and is named
    broken = strokes.copy()
    broken[2, 10, 0] = np.nan
    part = model.lognormal_augment(broken, n_samples=4, seed=5, start=np.tile(START, (5, 1)), dt=LR.DT_CASE)
    assert part["status"][2] == 3 and np.isnan(part["strokes"][2]).all()
    keep = [0, 1, 3, 4]
    assert _same(part["strokes"][keep], out["strokes"][keep])
    # the chain into strokes_to_motion on the fixture arm
    fx, chain = R.fixture(), IC.fixture_chain()
    mean = np.zeros((7, 21))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(147, 0.012))
    letters = out["strokes"].reshape(20, 100, 2).astype(np.float64)
    letters = 1.5 * letters / np.abs(letters).max(axis=(1, 2), keepdims=True)
    rows = model.strokes_to_motion(letters, basis, chain, StrokeCanvas(), fx["block_center"], fx["seed_pos"], orientation="seed")
    assert rows["params"].shape == (20, 147) and rows["image"].shape[0] == 20
    assert np.isfinite(rows["params"]).all() and np.isfinite(rows["image"]).all() and np.isfinite(rows["trajectory"]).all()


# ================================================================================================ the second pass (HISTORY section R20)
# 7. the fit inside its tile and component classes; 8. the exits of its loop; 9. the step's clips and the weights; 10. count NULL
# and out of range; 11. the sampler's edges.  The cases and their seeds: tests/lognormal_cases.py; the conditions they lean on:
# tests/test_lognormal_cpu.py.  Every pair is printed with its ratio; the worst ratio of a run is printed as it grows.
_WORST = {"ratio": 0.0, "where": ""}


def _pair(label, err, own):
    """print a measured pair and assert the 4x rule (an exact restatement asks for an exact kernel)"""
    ratio = err / own if own > 0 else (0.0 if err == 0 else np.inf)
    if ratio > _WORST["ratio"]:
        _WORST.update(ratio=ratio, where=label)
    print("%s: kernel %.3e, restatement %.3e, ratio %.2f (bound 4x; worst so far %.2f at %s)"
          % (label, err, own, ratio, _WORST["ratio"], _WORST["where"]))
    assert err <= 4.0 * own, label


def _path_err_at(params, count, ref_params, start, T, dt):
    """``_path_err`` at the case's own T and dt"""
    worst = 0.0
    for n in range(len(params)):
        a = LR.stroke(params[n, :count[n]], start[n], T, dt)[0]
        b = LR.stroke(ref_params[n, :count[n]], start[n], T, dt)[0]
        worst = max(worst, float(np.abs(a - b).max() / max(LR.extent(b), 1e-30)))
    return worst


def _fit_case(model, case, n_iters, count="case", rows=None, guard=0, **over):
    opt = dict(tol=0.0)
    opt.update(case["opt"])
    opt.update(over)
    rows = slice(None) if rows is None else list(rows)
    free = opt.get("free")
    if free is not None and np.asarray(free).ndim == 3:
        free = np.asarray(free)[rows]
    bounds = None if opt.get("lo") is None and opt.get("hi") is None else (opt.get("lo"), opt.get("hi"))
    return _fit(model, case["target"][rows], case["init"][rows], case["count"][rows] if isinstance(count, str) else count,
                case["start"][rows], case["dt"], n_iters=n_iters, weights=opt.get("weights", LR.DEFAULT_WEIGHTS), tol=opt["tol"],
                free=free, bounds=bounds, guard=guard)


def _check_against_refs(model, name, case, refs):
    """The comparison rule at every try count of ``refs``: a clear decision margin, the restatement deciding as the definition
    does, the integer outputs equal to the definition's, losses and the returned parameters' float64 path within 4x the
    restatement's own error; zeros above count and a masked parameter's bits kept.  -> {n_iters: the kernel's outputs}"""
    N, Cn, cnt = case["init"].shape[0], case["init"].shape[1], case["count"]
    free = case["opt"].get("free")
    out = {}
    for it, (r64, r32) in refs.items():
        assert LC.margin(r64) > 1e-3 and LC.decisions_agree(r64, r32)
        got = out[it] = _fit_case(model, case, it)
        for k in ("iterations", "accepted", "status"):
            assert np.array_equal(got[k], r64[k]), (k, got[k], r64[k])
        for k in ("loss0", "loss"):
            _pair("fit %s, %d tries, %s" % (name, it, k), LR.rel_err(got[k], r64[k]), LR.rel_err(r32[k], r64[k]))
        _pair("fit %s, %d tries, path / extent" % (name, it),
              _path_err_at(got["params"], cnt, r64["params"], case["start"], case["T"], case["dt"]),
              _path_err_at(r32["params"], cnt, r64["params"], case["start"], case["T"], case["dt"]))
        for n in range(N):
            assert not got["params"][n, cnt[n]:].any()
            if free is not None:
                fr = np.broadcast_to(free if free.ndim == 3 else free[None, None, :], (N, Cn, 6))[n, :cnt[n]] != 0
                assert _same(got["params"][n, :cnt[n]][~fr], case["init"][n, :cnt[n]][~fr])
    return out


# ------------------------------------------------------------------------------------------------ 7. tile and component classes
@pytest.mark.parametrize("shape", LC.TILE_SHAPES, ids=["C%d-T%d" % s for s in LC.TILE_SHAPES])
def test_fit_inside_the_tile_and_component_classes(V, shape):
    """Two rows, ``tol = 0``, after 1 and 4 tries, with T below, at, one past and a multiple of the tile of the class (64 / 32 / 8
    points at C <= 4 / 8 / 16), T = 2 and the limit 1024.  At T = 1 every component is still off at t = 0: the loss is exactly 0,
    no try is accepted, and that is asserted as such."""
    model = _model(V)
    Cn, T = shape
    case, refs = LC.tile_case(Cn, T)
    got = _check_against_refs(model, "C = %d, T = %d" % shape, case, refs)
    if T == 1:
        for it in LC.TRIES:
            g = got[it]
            assert not g["loss"].any() and not g["loss0"].any() and _same(g["params"], case["init"])
            assert (g["status"] == 1).all() and (g["iterations"] == it).all() and not g["accepted"].any()


@pytest.mark.parametrize("name", sorted(LC.RAGGED_CASES))
def test_fit_ragged_counts_in_the_smallest_and_widest_class(V, name):
    """counts (4, 2, 1, 0) at C = 4, (12, 9, 5, 0) at C = 12, and a mask per row at C = 12 with counts (12, 9, 5)"""
    case, refs = LC.ragged_case(name)
    _check_against_refs(_model(V), name, case, refs)


# ------------------------------------------------------------------------------------------------ 8. the exits of the loop
@pytest.mark.parametrize("which", ("pivot", "x"))
def test_fit_status_2_by_a_solve_that_fails(V, which):
    """A finite D near the top of float32.  "pivot": D = 3e38 in row 1 of three; the amplitude overflows, loss0 is not finite, M is
    NaN and every try ends at the first pivot (``LR._solve`` says so, tests/test_lognormal_cpu.py asserts it).  "x": one
    component with only sigma free and D = 1e37; M is the 1 x 1 infinity, the pivot passes and the solution is not finite.  The
    float64 definition does not overflow there, so the row is compared with the restatement: status 2 after 8 tries, none
    accepted, the parameters init's bits, and the other rows bitwise the run without that row."""
    model = _model(V)
    case = LC.overflow_case() if which == "pivot" else LC.x_reject_case()
    row = LC.OVERFLOW_ROW
    free = case["opt"].get("free")
    r32 = LR.fit_row(case["target"][row], case["init"][row], case["start"][row], case["dt"], n_iters=40, tol=case["opt"]["tol"],
                     free=free, restated=True)
    assert r32["solves"] == [which] * 8 and (r32["status"], r32["iterations"], r32["accepted"]) == (2, 8, 0)
    got = _fit_case(model, case, 40)
    print("fit solve failure (%s): status %s, tries %s, accepted %s, loss0 %s, loss %s" % (which, got["status"], got["iterations"],
          got["accepted"], got["loss0"], got["loss"]))
    assert (got["status"][row], got["iterations"][row], got["accepted"][row]) == (2, 8, 0)
    assert _same(got["params"][row], case["init"][row])
    assert not np.isfinite(got["loss0"][row]) and not np.isfinite(got["loss"][row])
    assert not np.isfinite(r32["loss0"]) and not np.isfinite(r32["loss"])
    others = [n for n in range(len(case["init"])) if n != row]
    alone = _fit_case(model, case, 40, rows=others)
    assert all(_same(alone[k], got[k][others]) for k in FIT_OUTPUTS)
    assert np.isin(alone["status"], (0, 1)).all() and alone["accepted"].all()


@pytest.mark.parametrize("name", sorted(LC.TOL_CASES))
def test_fit_tol_ends_a_row_in_the_definitions_try(V, name):
    """``tol`` > 0 on rows where definition and restatement end in the same try and every convergence decision has a margin
    |(L - L(new)) - tol L| > 1e-3 tol L: tries, accepted steps and status equal the definition's"""
    model = _model(V)
    case, refs = LC.tol_case(name)
    r64, r32 = refs[LC.TOL_TRIES]
    tol = case["opt"]["tol"]
    assert all(LC.conv_margin(t, tol) > 1e-3 for t in r64["tries"])
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(r32[k], r64[k])
    assert (r64["status"] == 0).all() and (r64["iterations"] < LC.TOL_TRIES).all()
    got = _fit_case(model, case, LC.TOL_TRIES)
    print("fit %s: tries %s, accepted %s" % (name, got["iterations"], got["accepted"]))
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(got[k], r64[k]), (k, got[k], r64[k])
    for k in ("loss0", "loss"):
        _pair("fit %s, %s" % (name, k), LR.rel_err(got[k], r64[k]), LR.rel_err(r32[k], r64[k]))
    _pair("fit %s, path / extent" % name,
          _path_err_at(got["params"], case["count"], r64["params"], case["start"], case["T"], case["dt"]),
          _path_err_at(r32["params"], case["count"], r64["params"], case["start"], case["T"], case["dt"]))


def test_fit_with_zero_tries(V):
    """``n_iters = 0``: status 1 (0 where count = 0), no try, the parameters init's bits, loss = loss0 that of init"""
    model = _model(V)
    case = LC.make(4, 3, 21, (3, 2, 1, 0))
    r64, r32 = LC.run(case, 0, False), LC.run(case, 0, True)
    got = _fit_case(model, case, 0)
    assert got["status"].tolist() == [1, 1, 1, 0] == r64["status"].tolist()
    assert not got["iterations"].any() and not got["accepted"].any()
    init = case["init"].copy()
    for n in range(4):
        init[n, case["count"][n]:] = 0.0
    assert _same(got["params"], init) and _same(got["loss"], got["loss0"])
    _pair("fit, zero tries, loss0", LR.rel_err(got["loss0"], r64["loss0"]), LR.rel_err(r32["loss0"], r64["loss0"]))


# ------------------------------------------------------------------------------------------------ 9. clips and weights
@pytest.mark.parametrize("name", sorted(LC.CLIP_CASES))
def test_fit_sigma_clip_without_bounds(V, name):
    """An initial sigma of 0.002: within four tries a sigma of that row ends on the clip [1e-3, 3] in the definition and in the
    restatement; the kernel returns the clip value's bits there"""
    model = _model(V)
    case, refs = LC.clip_case(name)
    _, row, _, clip = LC.CLIP_CASES[name]
    got = _check_against_refs(model, name, case, refs)
    on64 = refs[4][0]["params"][row, :, 3] == clip
    on32 = refs[4][1]["params"][row, :, 3] == np.float32(clip)
    assert on64.any() and np.array_equal(on64, on32)
    assert _same(got[4]["params"][row, on64, 3], np.full(int(on64.sum()), clip, dtype=np.float32))


@pytest.mark.parametrize("name", sorted(LC.BOUND_CASES))
def test_fit_one_bound_alone(V, name):
    """``lo`` without ``hi`` and ``hi`` without ``lo``, each binding: where the definition's parameter sits on the bound the
    kernel returns the bound's bits, and no moved parameter is beyond it"""
    model = _model(V)
    case, refs = LC.bound_case(name)
    got = _check_against_refs(model, name, case, refs)
    side = "lo" if "lo" in case["opt"] else "hi"
    bound = np.asarray(case["opt"][side], dtype=np.float32)
    on = np.isfinite(bound)[None, None, :] & (refs[4][0]["params"] == np.asarray(case["opt"][side], dtype=np.float64)[None, None, :])
    assert on.any()
    assert _same(got[4]["params"][on], np.broadcast_to(bound, on.shape)[on])
    moved = got[4]["params"] != case["init"]
    assert (got[4]["params"] >= bound if side == "lo" else got[4]["params"] <= bound)[moved].all()


@pytest.mark.parametrize("w", LC.WEIGHTS, ids=["wp%g-wv%g" % w for w in LC.WEIGHTS])
@pytest.mark.parametrize("shape", LC.WEIGHT_SHAPES, ids=["%dx%d" % s for s in LC.WEIGHT_SHAPES])
def test_fit_weights(V, shape, w):
    case, refs = LC.weight_case(shape[0], shape[1], w)
    _check_against_refs(_model(V), "%dx%d weights %s" % (shape + (w,)), case, refs)


@pytest.mark.parametrize("shape", LC.WEIGHT_SHAPES, ids=["%dx%d" % s for s in LC.WEIGHT_SHAPES])
def test_fit_with_both_weights_zero(V, shape):
    """the loss is 0 everywhere: no try is accepted, status 2 after 8 tries, the parameters init's bits"""
    model = _model(V)
    case = LC.make(shape[0], shape[1], 1000, weights=(0.0, 0.0))
    got = _fit_case(model, case, 40, tol=1e-9)
    r64 = LC.run(case, 40, False, tol=1e-9)
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(got[k], r64[k])
    assert (got["status"] == 2).all() and (got["iterations"] == 8).all() and not got["accepted"].any()
    assert not got["loss"].any() and not got["loss0"].any() and _same(got["params"], case["init"])


# ------------------------------------------------------------------------------------------------ 10. count
def _three_calls(model, params, count, start, target, T, dt, guard=0):
    """eval, sample (shift_mean on and off) and four fit tries -> the list of every output"""
    ev = _eval(model, params, count, start, T, dt, guard=guard)
    sm = [_sample(model, params, count, start, T, dt, 2, 11, shift, guard=guard) for shift in (True, False)]
    ft = _fit(model, target, params, count, start, dt, n_iters=4, tol=0.0, guard=guard)
    return list(ev) + [a for pair in sm for a in pair] + [ft[k] for k in FIT_OUTPUTS]


@pytest.mark.parametrize("Cn", (3, 6, 12))
def test_a_null_count_is_count_c_everywhere(V, Cn):
    model = _model(V)
    case = LC.make(2, Cn, 1000, T=70)
    full = _three_calls(model, case["init"], case["count"], case["start"], case["target"], 70, case["dt"])
    null = _three_calls(model, case["init"], None, case["start"], case["target"], 70, case["dt"])
    assert (case["count"] == Cn).all() and len(null) == len(full) == 12
    assert all(_same(a, b) for a, b in zip(null, full))
    assert np.abs(full[1]).max() > 0 and full[-3].any()                # (something moved, and tries were made)


@pytest.mark.parametrize("Cn", (3, 6, 12))
def test_counts_out_of_range_are_clamped(V, Cn):
    """counts (-3, 0, C, C + 5) give the bits of (0, 0, C, C) in all three calls, and two guard rows of -7 before and behind every
    output stay as they were"""
    model = _model(V)
    case = LC.make(4, Cn, 1000, T=70)
    wild = np.array([-3, 0, Cn, Cn + 5], dtype=np.int32)
    tame = np.array([0, 0, Cn, Cn], dtype=np.int32)
    a = _three_calls(model, case["init"], wild, case["start"], case["target"], 70, case["dt"], guard=2)
    b = _three_calls(model, case["init"], tame, case["start"], case["target"], 70, case["dt"], guard=2)
    assert all(_same(x, y) for x, y in zip(a, b))
    assert not a[-6][:2].any() and a[-6][2:].any() and a[-1].tolist()[:2] == [0, 0]      # params and status of the fit


# ------------------------------------------------------------------------------------------------ 11. the sampler's edges
@pytest.mark.parametrize("shape", LC.SAMPLE_EDGE_SHAPES, ids=["%dx%dx%dx%d" % s for s in LC.SAMPLE_EDGE_SHAPES])
def test_sample_edges_against_the_definition(V, shape):
    """T = 1024 (the whole of the staged stroke) with counts (16, 0, 9) and negative D; N = S = C = T = 1; one sample of an exact
    two chunks.  shift_mean on and off; the count = 0 row with shift_mean is start minus the butterfly mean of start, about
    3e-8 and not 0: the restatement's bits."""
    model = _model(V)
    N, S, Cn, T = shape
    params, count, start, dt = LC.sample_edge(shape)
    seed = 0x1234567855
    for shift in (False, True):
        r64 = LR.sample(params, count, start, T, dt, S, seed, shift_mean=shift)
        r32 = LR.sample_restated(params, count, start, T, dt, S, seed, shift_mean=shift)
        got = _sample(model, params, count, start, T, dt, S, seed, shift, guard=1)
        for k, what in enumerate(("strokes", "perturbed")):
            assert got[k].shape == r64[k].shape
            _pair("sample edge %s shift_mean %s %s" % (shape, shift, what), LR.rel_err(got[k], r64[k]), LR.rel_err(r32[k], r64[k]))
        ev = _eval(model, got[1].reshape(N * S, Cn, 6), np.repeat(count, S), np.repeat(start, S, axis=0), T, dt, velocity=False)[0]
        ev = ev.reshape(N, S, T, 2)
        if shift:
            mean = np.stack([[LR.mean_restated(ev[n, s]) for s in range(S)] for n in range(N)])
            assert _same(got[0], (ev - mean[:, :, None, :]).astype(np.float32))
        else:
            assert _same(got[0], ev)
        for n in np.flatnonzero(count == 0):
            assert _same(got[0][n], r32[0][n]) and not got[1][n].any()
            if shift:
                assert np.abs(got[0][n]).max() < 1e-6
            else:
                assert _same(got[0][n], np.broadcast_to(start[n], (S, T, 2)).copy())


def test_sample_scales_and_a_seed_with_high_bits(V):
    model = _model(V)
    N, S, Cn, T, dt, scales = 2, 3, 4, 100, 0.01, (0.5, 1.0, 0.7)
    params, start = _random_rows(N, Cn, 17), np.tile(START, (N, 1))
    count = np.array([4, 3], dtype=np.int32)
    r64 = LR.sample(params, count, start, T, dt, S, LC.HIGH_SEED, *scales, shift_mean=True)
    r32 = LR.sample_restated(params, count, start, T, dt, S, LC.HIGH_SEED, *scales, shift_mean=True)
    got = _sample(model, params, count, start, T, dt, S, LC.HIGH_SEED, True, scales=scales)
    for k, what in enumerate(("strokes", "perturbed")):
        _pair("sample scales %s, seed %#x, %s" % (scales, LC.HIGH_SEED, what), LR.rel_err(got[k], r64[k]), LR.rel_err(r32[k], r64[k]))
    # the high word of the seed and each scale reach the draw
    low = _sample(model, params, count, start, T, dt, S, LC.HIGH_SEED & 0xFFFFFFFF, True, scales=scales)
    assert not np.array_equal(low[1][..., 0], got[1][..., 0])
    default = _sample(model, params, count, start, T, dt, S, LC.HIGH_SEED, True)
    for j in (0, 4, 5):
        assert not np.array_equal(default[1][..., j], got[1][..., j])


@pytest.mark.parametrize("shift", (False, True))
def test_sample_a_nan_row_is_nan_and_alone(V, shift):
    model = _model(V)
    N, S, Cn, T, dt, seed = 4, 2, 3, 100, 0.01, 5
    params, start, count = _random_rows(N, Cn, 23), np.tile(START, (N, 1)), np.array([3, 3, 2, 3], dtype=np.int32)
    good = _sample(model, params, count, start, T, dt, S, seed, shift)
    assert np.isfinite(good[0]).all()
    bad_p, bad_s = params.copy(), start.copy()
    bad_p[1, 2, 1] = np.nan
    bad_p[2, 2, 3] = np.nan                               # beyond count: never read
    bad_s[3, 0] = np.nan
    got = _sample(model, bad_p, count, bad_s, T, dt, S, seed, shift)
    assert np.isnan(got[0][1]).all() and np.isnan(got[0][3]).all()
    assert _same(got[0][[0, 2]], good[0][[0, 2]]) and _same(got[1][[0, 2, 3]], good[1][[0, 2, 3]])


def test_sample_at_the_last_row_offset(V):
    """``row_offset = 2^32 - N``: the counter's first word is one short of wrapping in the last row"""
    model = _model(V)
    N, S, Cn, T, dt, seed = 3, 2, 4, 100, 0.01, 99
    params, start, count = _random_rows(N, Cn, 29), np.tile(START, (N, 1)), np.array([4, 3, 4], dtype=np.int32)
    off = 2 ** 32 - N
    r64 = LR.sample(params, count, start, T, dt, S, seed, shift_mean=True, row_offset=off)
    r32 = LR.sample_restated(params, count, start, T, dt, S, seed, shift_mean=True, row_offset=off)
    got = _sample(model, params, count, start, T, dt, S, seed, True, offset=off)
    for k, what in enumerate(("strokes", "perturbed")):
        _pair("sample row_offset 2^32 - %d %s" % (N, what), LR.rel_err(got[k], r64[k]), LR.rel_err(r32[k], r64[k]))
    part = _sample(model, params[1:], count[1:], start[1:], T, dt, S, seed, True, offset=off + 1)
    assert _same(part[0], got[0][1:]) and _same(part[1], got[1][1:])
    assert not np.array_equal(_sample(model, params, count, start, T, dt, S, seed, True)[1][..., 0], got[1][..., 0])
    ts = [_dev(model, params), _dev(model, count, torch.int32), _dev(model, start)]
    out = torch.full((N, S, T, 2), -7.0, device=model.device)
    rc = model._L.avae_lognormal_sample(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, S, Cn, T, dt, seed, off + 1, 0.2, 0.3, 0.1, 1,
                                        _p(out), None, _stream(model))
    torch.cuda.synchronize()
    assert rc != 0 and "row_offset" in _err(model) and (out == -7).all()
