"""Sigma-lognormal strokes (avae_lognormal_eval / avae_lognormal_sample / avae_lognormal_fit, lognormal_eval / lognormal_fit /
lognormal_augment) on a real MI355X (include/avae.h) against tests/lognormal_reference.py.

1. eval, 2. the sampler and 3. the fit step for step (``tol = 0``, after 1 and 4 tries) against the float64 definition, within 4x
the float32 restatement's own worst error over the same inputs (the rule of test_gpu_motion.py; |err| / (|ref| + 1), paths of
fitted parameters as |err| / extent); 4. the fit's contract at the default options; 5. bit reproducibility and independence;
6. ``lognormal_augment`` end to end into ``strokes_to_motion``.  The measured pairs are in README.md and DESIGN.md section 28."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_cases as IC
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


def _eval(model, params, count, start, T, dt, velocity=True, stream=None):
    """avae_lognormal_eval -> (path, velocity or None) as NumPy, prefilled with -7"""
    N, Cn = params.shape[0], params.shape[1]
    ts = [_dev(model, params), _dev(model, count, torch.int32), _dev(model, start)]
    path = torch.full((N, T, 2), -7.0, device=model.device)
    vel = torch.full((N, T, 2), -7.0, device=model.device) if velocity else None
    torch.cuda.synchronize()                             # (the inputs and the prefill are there before another stream reads them)
    rc = model._L.avae_lognormal_eval(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, Cn, T, dt, _p(path), _p(vel), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return path.cpu().numpy(), None if vel is None else vel.cpu().numpy()


def _sample(model, params, count, start, T, dt, S, seed, shift, offset=0, want_params=True, stream=None,
            scales=(0.2, np.pi / 9, 0.1)):
    """avae_lognormal_sample -> (strokes [N, S, T, 2], perturbed [N, S, C, 6] or None) as NumPy, prefilled with -7"""
    N, Cn = params.shape[0], params.shape[1]
    ts = [_dev(model, params), _dev(model, count, torch.int32), _dev(model, start)]
    out = torch.full((N, S, T, 2), -7.0, device=model.device)
    pert = torch.full((N, S, Cn, 6), -7.0, device=model.device) if want_params else None
    torch.cuda.synchronize()
    rc = model._L.avae_lognormal_sample(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), N, S, Cn, T, dt, seed, offset, scales[0],
                                        scales[1], scales[2], 1 if shift else 0, _p(out), _p(pert), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return out.cpu().numpy(), None if pert is None else pert.cpu().numpy()


def _fit(model, target, init, count, start, dt, n_iters=40, weights=LR.DEFAULT_WEIGHTS, tol=1e-9, free=None, bounds=None,
         want=FIT_OUTPUTS, stream=None):
    """avae_lognormal_fit -> dict of the NumPy outputs asked for (``params`` always), prefilled with -7"""
    N, T, Cn = target.shape[0], target.shape[1], init.shape[1]
    ts = [_dev(model, target), _dev(model, init), _dev(model, count, torch.int32), _dev(model, start)]
    fr = _dev(model, free, torch.uint8)
    lo, hi = (None, None) if bounds is None else (_dev(model, np.asarray(b, dtype=np.float32)) for b in bounds)
    dts = dict(params=torch.float32, loss0=torch.float64, loss=torch.float64, iterations=torch.int32, accepted=torch.int32,
               status=torch.int32)
    out = {k: torch.full((N, Cn, 6) if k == "params" else (N,), -7, device=model.device, dtype=dts[k]) for k in want}
    torch.cuda.synchronize()
    rc = model._L.avae_lognormal_fit(model._h, _p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), N, Cn, T, dt, n_iters, weights[0],
                                     weights[1], tol, _p(fr), 1 if (fr is not None and fr.dim() == 3) else 0, _p(lo), _p(hi),
                                     _p(out["params"]), _p(out.get("loss0")), _p(out.get("loss")), _p(out.get("iterations")),
                                     _p(out.get("accepted")), _p(out.get("status")), _stream(model, stream))
    torch.cuda.synchronize()
    assert rc == 0, _err(model)
    return {k: v.cpu().numpy() for k, v in out.items()}


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
