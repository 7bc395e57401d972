"""Parameter averaging on the MI355X (include/avae.h, avae_set_ema / avae_use_averaged), against the kernel's
own arithmetic (tests/ema_reference.py on the device's previous average and new parameters) and, bitwise, against twins: training
with and without averaging, replays against single steps, averaged inference against a fresh model given the average.

Shapes (tests/test_gpu_clip.py's): model A = the fused small-net plan (784-24-24 / 147-12-12, n_z 4, B 32: averaging moves it to
weight gradients -> k_adam), model B = edge tiles and a partial last quad (784-130-70 / 147-65-35, n_z 20, B 64), model C = the conv
model of tests/golden/conv_small.npz's shape (the adjoint filter shadows).  relu, weights [50, 1], assoc_lambda 8."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gpu_clip as TC
from ema_reference import decay_t, ema_step
from test_gpu_parity import opt_snapshot, shadow_err, synth_batch

pytestmark = pytest.mark.gpu

MODELS, BIN, rows = TC.MODELS, TC.BIN, TC.rows
U32 = 2.0 ** -23
DECAY = 0.999
STEPS = 21                                                   # partial_fit_steps: one 16-step, one 4-step replay and a single step


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def make(V, name, dtype, ema=None, **kw):
    model, _ = TC.make(V, name, dtype, **kw)
    if ema is not None:
        model.set_ema(**ema)
    return model


_DATA = {}


def data(name, steps, seed=21):
    """the first `steps` of 24 batches (computed once per model, shared, never written to)"""
    archs, B = MODELS[name]
    if (name, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = synth_batch(rng, 24 * B, [a["n_input"] for a in archs], BIN)
        _DATA[(name, seed)] = (X, rng.standard_normal((24 * B, archs[0]["n_z"])).astype(np.float32))
    X, eps = _DATA[(name, seed)]
    return [x[:steps * B] for x in X], eps[:steps * B], B


def head(X, eps, B, n):
    """the first n batches, as partial_fit_steps(X, n, eps) takes them"""
    return [x[:n * B] for x in X], n, eps[:n * B]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def master(model):
    """the average as it lies in memory: the padded internal layout (avae_debug_fetch "ema_master")"""
    n = model._grad_tensor().numel() - 1                     # P_int
    buf = np.empty(n, np.float32)
    cnt = C.c_size_t(0)
    rc = model._L.avae_debug_fetch(model._h, b"ema_master", buf.ctypes.data_as(C.c_void_p), n, C.byref(cnt))
    assert rc == 0 and cnt.value == n, model._L.avae_last_error(model._h)
    return buf


def check_ema_step(e_prev, th_new, e_new, decay, warmup, step):
    """The kernel's e + (theta - e) * omd from HIP's own previous average and new parameters: the difference and the fused
    multiply-add round once each -- 1/2 ulp of |theta - e| <= 2a times omd <= 1, and 1/2 ulp of the result, |e_new| <= a,
    a = max(|e_prev|, |theta|): at most 2^-23 a -- and nothing is rounded where theta == e."""
    want = ema_step(e_prev, th_new, decay, warmup, step)
    err = np.abs(e_new.astype(np.float64) - want)
    a = np.maximum(np.abs(e_prev), np.abs(th_new)).astype(np.float64)
    worst = int(np.argmax(err - U32 * a))
    print("step %d: d_t %.9g max err %.3e (bound there %.3e), %d of %d elements moved" % (
        step, decay_t(decay, warmup, step), err.max(), U32 * a[np.argmax(err)], int(np.sum(bits(e_new) != bits(e_prev))), e_new.size))
    assert err[worst] <= U32 * a[worst], "step %d element %d: e %r theta %r -> %r, want %r" % (
        step, worst, e_prev[worst], th_new[worst], e_new[worst], want[worst])
    still = bits(th_new) == bits(e_prev)
    assert np.array_equal(bits(e_new)[still], bits(e_prev)[still]), "an element with theta == e moved"


# ----------------------------------------------------------------------------- 1. the update, step by step
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_update_step_by_step(V, name, dtype, warmup):
    """Five single steps, each against ema_reference.ema_step.  The padding of the internal layout never changes (the average has
    no cost slot: its allocation ends with the last parameter row)."""
    X, eps, B = data(name, 5)
    model = make(V, name, dtype, ema=dict(decay=DECAY, warmup=warmup))
    th0 = model.get_params()
    assert same(model.get_ema_params(), th0), "the average starts at the current parameters"
    # which floats of the internal layout are padding: the ones a flat vector of ones does not reach
    model.set_ema_params(np.ones(model.n_params, np.float32))
    raw = master(model)
    pad = raw == 0.0
    assert np.all(raw[~pad] == 1.0) and int((~pad).sum()) == model.n_params and pad.any()
    model.set_ema_params(th0)
    assert same(model.get_ema_params(), th0) and not master(model)[pad].any()
    moved = 0
    for s in range(5):
        e_prev = model.get_ema_params()
        model.partial_fit(*rows(X, eps, B, s))
        th, e = model.get_params(), model.get_ema_params()
        assert model.get_opt_state()[2] == s + 1
        check_ema_step(e_prev, th, e, DECAY, warmup, s + 1)
        moved += int(np.sum(bits(e) != bits(e_prev)))
        assert not bits(master(model))[pad].any(), "step %d wrote padding of the average" % s
        assert shadow_err(model)[:2] == (0.0, 0.0)
    assert moved > model.n_params // 2, "the average must move"


# ----------------------------------------------------------------------------- 2. training is untouched
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_training_is_bitwise_untouched(V, name, dtype):
    """theta, m, v, the step and the costs with averaging on against a twin without it (model A: k_adam against the fused launch)."""
    X, eps, B = data(name, STEPS)
    on = make(V, name, dtype, ema=dict(decay=DECAY, warmup=True))
    off = make(V, name, dtype)
    on.partial_fit_steps(X, STEPS, eps)
    off.partial_fit_steps(X, STEPS, eps)
    assert TC.same_state(on, off) and TC.state(on)[3] == STEPS
    assert np.array_equal(on.cost_history(STEPS), off.cost_history(STEPS))
    assert shadow_err(on)[:2] == (0.0, 0.0)
    assert not same(on.get_ema_params(), on.get_params())
    # switched off again: the previous plan is back, and still the same training
    on.set_ema(None)
    Xs, es = rows(X, eps, B, 0)
    assert on.partial_fit(Xs, es) == off.partial_fit(Xs, es) and TC.same_state(on, off)
    with pytest.raises(RuntimeError, match="averaging is off"):
        on.get_ema_params()


# ----------------------------------------------------------------------------- 3. replays equal eager
def _variant(V, variant, name, dtype, X, B):
    kw, fit = {}, {}
    if variant == "clip":
        n0, _ = TC.first_norm(V, name, dtype)
        kw["clip"] = dict(max_norm=0.5 * n0)
    elif variant == "masked":
        fit["present"] = np.ones((STEPS * B, 2), np.uint8)
    elif variant == "inputs":
        rng = np.random.default_rng(5)
        fit["inputs"] = [np.where(rng.random(X[0].shape) < 0.2, 0.0, X[0]).astype(np.float32), None]
    return kw, fit


@pytest.mark.parametrize("variant", ["plain", "clip", "masked", "inputs"])
def test_replays_equal_single_steps(V, variant):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, STEPS)
    kw, fit = _variant(V, variant, name, dtype, X, B)
    ema = dict(decay=0.9, warmup=True)                       # (warm-up up to step 80: every step has its own factor)
    run = make(V, name, dtype, ema=ema, **kw)
    run.partial_fit_steps(X, STEPS, eps, **fit)
    single = make(V, name, dtype, ema=ema, **kw)
    for i in range(STEPS):
        sl = slice(i * B, (i + 1) * B)
        f = {k: (v[sl] if k == "present" else [None if t is None else t[sl] for t in v]) for k, v in fit.items()}
        single.partial_fit(*rows(X, eps, B, i), **f)
    assert TC.same_state(run, single)
    assert same(run.get_ema_params(), single.get_ema_params())
    assert not same(run.get_ema_params(), run.get_params())
    if variant == "clip":
        assert np.sum(run.grad_norm_history(STEPS)[0] > np.float32(kw["clip"]["max_norm"])) >= 3, "the run must hold clipped steps"
    if variant == "plain":                                    # and without graphs
        eager = make(V, name, dtype, ema=ema, use_graph=False)
        eager.partial_fit_steps(X, STEPS, eps)
        assert TC.same_state(run, eager) and same(run.get_ema_params(), eager.get_ema_params())
    if variant == "masked":                                   # an all-present masked run is the plain run
        plain = make(V, name, dtype, ema=ema)
        plain.partial_fit_steps(X, STEPS, eps)
        assert same(run.get_ema_params(), plain.get_ema_params())


# ----------------------------------------------------------------------------- 4. skipping
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_skipped_step_keeps_the_average(V, name, dtype):
    X, eps, B = data(name, 8)
    bad = [X[0], X[1].copy()]
    bad[1][5 * B + 3, 7] = np.nan
    model = make(V, name, dtype, ema=dict(decay=DECAY, warmup=True), clip=dict(skip_nonfinite=True))
    model.partial_fit(*rows(X, eps, B, 0))
    before, e_before = opt_snapshot(model), model.get_ema_params()
    raw_before = master(model)
    c = model.partial_fit(*rows(bad, eps, B, 5))
    after = opt_snapshot(model)
    assert np.isnan(c) and after[3] == before[3] + 1 == 2 and model.grad_norm_history(1)[2] == 1
    assert all(same(a, b) for a, b in zip(before[:3], after[:3]))
    assert np.array_equal(bits(master(model)), bits(raw_before)), "a skipped step wrote the average"
    model.partial_fit(*rows(X, eps, B, 1))
    assert model.get_opt_state()[2] == 3
    check_ema_step(e_before, model.get_params(), model.get_ema_params(), DECAY, True, 3)      # the skipped step consumed number 2
    assert decay_t(DECAY, True, 3) != decay_t(DECAY, True, 2)


# ----------------------------------------------------------------------------- 5. averaged inference
def _inference(model, X, eps, z, P):
    out = list(model.generate(z)) + list(model.transform(X))
    sc = model.score_samples(X, eps)
    out += [sc[k] for k in ("cost", "recon", "latent", "assoc")]
    im = model.impute(X, present=P)
    out += [im["mu"], im["logvar"]] + list(im["mean"])
    out.append(np.float32(model.evaluate_cost(X, eps)))
    return [np.array(o, np.float32) for o in out]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_averaged_inference(V, name, dtype):
    X, eps, B = data(name, 9)
    model = make(V, name, dtype, ema=dict(decay=0.9))
    model.partial_fit_steps(*head(X, eps, B, 8))
    Xe, ee = rows(X, eps, B, 8)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((B, MODELS[name][0][0]["n_z"])).astype(np.float32)
    P = np.ones((B, len(MODELS[name][0])), np.uint8)
    P[::3, 1] = 0
    P[1::3, 0] = 0
    live = _inference(model, Xe, ee, z, P)
    avg = model.get_ema_params()
    assert not same(avg, model.get_params())
    fresh = make(V, name, dtype)
    fresh.set_params(avg)
    want = _inference(fresh, Xe, ee, z, P)
    state = opt_snapshot(model)
    with model.averaged() as m:
        assert m is model
        got = _inference(model, Xe, ee, z, P)
        assert shadow_err(model)[:2] == (0.0, 0.0)              # (against the average, rounded once to the compute dtype)
        assert same(model.get_params(), state[0]), "get_params returns the live parameters"
    assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    assert any(not same(g, l) for g, l in zip(got, live)), "the averaged results must differ from the live ones"
    assert shadow_err(model)[:2] == (0.0, 0.0)                  # (against theta again)
    again = _inference(model, Xe, ee, z, P)
    assert all(same(a, l) for a, l in zip(again, live))
    now = opt_snapshot(model)
    assert all(same(a, b) for a, b in zip(state[:3], now[:3])) and now[3] == state[3] and same(model.get_ema_params(), avg)
    # the block switches back when it raises
    with pytest.raises(KeyError):
        with model.averaged():
            raise KeyError("x")
    model.partial_fit(Xe, ee)
    # set_params leaves the model on the live parameters
    model.use_averaged(True)
    model.set_params(state[0])
    assert shadow_err(model)[:2] == (0.0, 0.0)
    model.partial_fit(Xe, ee)


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(V):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 4)
    model = make(V, name, dtype, ema=dict(decay=DECAY))
    model.partial_fit_steps(*head(X, eps, B, 2))
    snap, avg = opt_snapshot(model), model.get_ema_params()
    x1, e1 = rows(X, eps, B, 2)
    model._staged_j = 0                                          # (what a successful _stage leaves for _backward_bucket)
    with model.averaged():
        for call in (lambda: model.partial_fit(x1, e1),
                     lambda: model.partial_fit_steps(X, 4, eps),
                     lambda: model.partial_fit(x1, e1, present=np.ones((B, 2), np.uint8)),
                     lambda: model.partial_fit_steps(X, 4, eps, present=np.ones((4 * B, 2), np.uint8)),
                     lambda: model.partial_fit(x1, e1, inputs=[x1[0], None]),
                     lambda: model._stage(x1, e1),
                     lambda: model._backward_bucket(0),
                     lambda: model._apply_bucket(0)):
            with pytest.raises(RuntimeError, match="avae_use_averaged"):
                call()
        now = opt_snapshot(model)
        assert all(same(a, b) for a, b in zip(snap[:3], now[:3])) and now[3] == snap[3]
        assert same(model.get_ema_params(), avg)
        model.evaluate_cost(x1, e1)                              # evaluation is served
    model.partial_fit(x1, e1)                                    # and training after the block
    assert model.get_opt_state()[2] == snap[3] + 1
    # set_ema(0) while averaged switches back first
    model.use_averaged(True)
    model.set_ema(0)
    assert shadow_err(model)[:2] == (0.0, 0.0)
    model.partial_fit(x1, e1)
    for call in (model.get_ema_params, lambda: model.set_ema_params(avg), lambda: model.use_averaged(True)):
        with pytest.raises(RuntimeError, match="averaging is off"):
            call()
    model.use_averaged(False)                                    # off while off: nothing to do
    # bad arguments: ValueError before any device call (the handle is not even looked at)
    h, model._h = model._h, None
    try:
        for bad in (dict(decay=1.0), dict(decay=-0.5), dict(decay=float("nan")), dict(decay=0.9, warmup=2), dict(decay="0.9")):
            with pytest.raises(ValueError):
                model.set_ema(**bad)
        with pytest.raises(ValueError, match="expected"):
            model.set_ema_params(np.zeros(3, np.float32))
    finally:
        model._h = h
    with pytest.raises(ValueError, match="unknown key"):
        V.AssocVariationalAutoEncoder(MODELS[name][0], ema=dict(decay=0.9, rate=2))
    # the library's own checks
    L = model._L
    for d, w, needle in ((float("nan"), 0, b"decay"), (-0.1, 0, b"decay"), (1.0, 0, b"decay"), (0.9, 2, b"warmup")):
        assert L.avae_set_ema(model._h, C.c_float(d), w) != 0 and needle in L.avae_last_error(model._h)
    assert L.avae_use_averaged(model._h, 2) != 0


# ----------------------------------------------------------------------------- 7. checkpoint
def _ckpt_layout(model, name):
    archs = MODELS[name][0]
    hdr = 8 + 12
    for na in archs:
        L = 2
        hdr += 4 * (2 + L + 3)
    return hdr + 16, model.n_params


def test_checkpoint(V, tmp_path):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 16)
    model = make(V, name, dtype)
    model.partial_fit_steps(*head(X, eps, B, 3))
    # averaging off: the version-2 file, byte for byte
    f2 = str(tmp_path / "v2.ckpt")
    model.save_model(f2)
    raw = open(f2, "rb").read()
    hdr, P = _ckpt_layout(model, name)
    assert raw[:8] == b"AVAECKPT" and int.from_bytes(raw[8:12], "little") == 2 and len(raw) == hdr + 12 * P
    th, m, v, t = opt_snapshot(model)
    assert int.from_bytes(raw[hdr - 16:hdr - 8], "little") == P and int.from_bytes(raw[hdr - 8:hdr], "little") == t == 3
    assert raw[hdr:] == th.tobytes() + m.tobytes() + v.tobytes()
    # averaging on: version 3 = the same body + decay, warmup, the average
    ema = dict(decay=0.6, warmup=True)                       # (1 + t) / (10 + t) crosses 0.6 at t = 13
    model.set_ema(**ema)
    model.partial_fit_steps(*head(X, eps, B, 7))
    f3 = str(tmp_path / "v3.ckpt")
    model.save_model(f3)
    raw3 = open(f3, "rb").read()
    assert int.from_bytes(raw3[8:12], "little") == 3 and len(raw3) == hdr + 12 * P + 8 + 4 * P
    th, m, v, t = opt_snapshot(model)
    avg = model.get_ema_params()
    assert t == 10 and raw3[12:hdr - 8] == raw[12:hdr - 8]
    assert raw3[hdr:] == (th.tobytes() + m.tobytes() + v.tobytes() + np.float32(0.6).tobytes() + (1).to_bytes(4, "little")
                           + avg.tobytes())
    fresh = make(V, name, dtype)
    fresh.restore_model(str(tmp_path), "v3.ckpt")
    assert TC.same_state(model, fresh) and same(fresh.get_ema_params(), avg)
    f3b = str(tmp_path / "v3b.ckpt")
    fresh.save_model(f3b)
    assert open(f3b, "rb").read() == raw3, "decay / warmup did not come back"
    for mdl in (model, fresh):
        for i in range(10, 15):                                  # steps 11..15: warm-up factors, then decay itself
            mdl.partial_fit(*rows(X, eps, B, i))
    assert TC.same_state(model, fresh) and same(model.get_ema_params(), fresh.get_ema_params())
    assert not same(model.get_ema_params(), avg)
    # switched off again: version 2 again
    model.set_ema(None)
    model.save_model(f2)
    raw = open(f2, "rb").read()
    assert int.from_bytes(raw[8:12], "little") == 2 and len(raw) == hdr + 12 * P
    # a version-2 file loaded with averaging on: the average restarts at the loaded parameters
    fresh.restore_model(str(tmp_path), "v2.ckpt")
    assert TC.same_state(model, fresh)
    assert same(fresh.get_ema_params(), fresh.get_params())
    # a load leaves the model on the live parameters
    fresh.partial_fit(*rows(X, eps, B, 15))
    fresh.use_averaged(True)
    fresh.restore_model(str(tmp_path), "v3.ckpt")
    assert shadow_err(fresh)[:2] == (0.0, 0.0) and same(fresh.get_ema_params(), avg)
    fresh.partial_fit(*rows(X, eps, B, 15))
    assert os.path.getsize(f3) == len(raw3)


# ----------------------------------------------------------------------------- 8. data parallelism on one GPU
@pytest.mark.parametrize("comm", ["ipc", "library"])
@pytest.mark.parametrize("buckets", [1, 2])
def test_one_rank_pipeline_is_the_single_replica_average(V, comm, buckets):
    name, dtype = "A", "bf16"
    ema = dict(decay=0.9, warmup=True)
    X, eps, B = data(name, STEPS)
    plain = make(V, name, dtype, ema=ema)
    plain.partial_fit_steps(X, STEPS, eps)
    dp = make(V, name, dtype, ema=ema, comm=comm, comm_buckets=buckets)
    assert dp._comm_lib and len(dp._buckets) == buckets
    dp.partial_fit_steps(X, STEPS, eps)
    assert TC.same_state(plain, dp)
    assert same(plain.get_ema_params(), dp.get_ema_params())
    assert not same(dp.get_ema_params(), dp.get_params())


def test_host_owned_seam_replicas_hold_equal_averages(V):
    from vae_assoc_amd import _capi
    name, dtype = "A", "bf16"
    archs, B = MODELS[name]
    X, eps, _ = data(name, 6)                                   # three global batches of 2 * B rows
    reps = []
    for r in range(2):
        rep = make(V, name, dtype)
        p0 = rep.get_params()
        rep._L.avae_destroy(rep._h)
        rep._cfg.row_offset, rep._cfg.batch_global = B * r, 2 * B
        h = C.c_void_p()
        _capi.check(None, rep._L.avae_create(C.byref(rep._cfg), C.byref(h)), "avae_create")
        rep._h = h
        rep.set_params(p0)
        rep.set_ema(0.9, warmup=True)
        reps.append(rep)
    for s in range(3):
        e_prev = reps[0].get_ema_params()
        for r, rep in enumerate(reps):
            rep._backward(*rows(X, eps, B, 2 * s + r))
        torch.cuda.synchronize()
        gsum = reps[0]._grad_tensor() + reps[1]._grad_tensor()
        for rep in reps:
            rep._grad_tensor().copy_(gsum)
        torch.cuda.synchronize()
        for rep in reps:
            rep._apply()
        assert TC.same_state(reps[0], reps[1])
        assert same(reps[0].get_ema_params(), reps[1].get_ema_params())
        check_ema_step(e_prev, reps[0].get_params(), reps[0].get_ema_params(), 0.9, True, s + 1)
    assert not same(reps[0].get_ema_params(), reps[0].get_params())


# ----------------------------------------------------------------------------- the route
def test_timing_report_names_the_route(V):
    """Timing mode (eager launches): averaging on = wgrad, adam; off = the fused launch; a switch = one shadow_refresh."""
    m = make(V, "A", "bf16")
    X, eps, B = data("A", 2)

    def launches(work):
        assert m._L.avae_timing_enable(m._h, 1) == 0
        work()
        buf = C.create_string_buffer(1 << 16)
        assert m._L.avae_timing_report(m._h, buf, len(buf)) == 0 and m._L.avae_timing_enable(m._h, 0) == 0
        return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}

    off = launches(lambda: m.partial_fit_steps(X, 2, eps))
    assert off.get("wgrad+adam") == 2 and "adam" not in off
    m.set_ema(DECAY)
    on = launches(lambda: m.partial_fit_steps(X, 2, eps))
    assert on.get("adam") == 2 and on.get("wgrad") == 2 and "wgrad+adam" not in on and "grad_sumsq" not in on
    sw = launches(lambda: m.use_averaged(True))
    assert sw.get("shadow_refresh") == 1 and "adam" not in sw
    m.use_averaged(False)
