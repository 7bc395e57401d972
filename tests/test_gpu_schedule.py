"""On-device training schedules on the MI355X (include/avae.h, avae_set_schedule): the recorded
multipliers against the fp64 evaluator, the scheduled cost and gradient against the torch fp64 restatement
(tests/schedule_reference.py), and -- bitwise -- against unscheduled handles built with the scheduled values, across every
training route.

Models: A = the fused small-net plan (784-24-24 / 147-12-12, n_z 4, B 32); B = edge tiles and a partial last quad
(784-130-70 / 147-65-35, n_z 20, B 64); C = the conv model of tests/golden/conv_small.npz's shape (its latent and cost items run
on k_grouped); D = three modalities 60-20-16 / 21-12-10 / 17-8-8, n_z 3, B 8 (three pairs).  relu with the kernels' own relu
decisions for A / B / C, softplus for D; weights [50, 1] ([50, 1, 1] for D); assoc_lambda 8.

Model C's cost item runs on k_grouped, but in the default plan its latent item rides in the lean output + loss launch
(k_small_loss, tile configuration 9) like A's and B's.  "Cg" is the same model planned under AVAE_NO_LEAN_LOSS=1, the planner's
own switch, which puts that launch -- and the latent item -- on k_grouped; test_conv_model_covers_the_grouped_kernel asserts both
plans through tests/plan_dump.py, and the bitwise tests run C and Cg."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import plan_dump
from conftest import hip_relu_masks, make_arch
from schedule_reference import hyper, schedule_value, scheduled_cost_and_grads, ulp_distance
from test_gpu_parity import _load_big, build_pair, check_adam_step, opt_snapshot, per_tensor_err, shadow_err, synth_batch

pytestmark = pytest.mark.gpu

LAM, LR = 8.0, 1e-3
F32 = np.float32
KL = dict(knots=[(0, 0), (5, 0.5), (18, 1)])
ASSOC = dict(knots=[(0, 0), (3, 1)], period=7)
LRS = dict(decay_rate=0.9, decay_steps=4, staircase=False)
SCHED = dict(kl=KL, assoc=ASSOC, lr=LRS)


def _models():
    conv = _load_big().SMALL["conv_small"][0]
    two, three = ([True, False], [50, 1], "relu"), ([True, False, False], [50, 1, 1], "softplus")
    return {"A": ([make_arch("image", 784, 24, 24, 4), make_arch("joint", 147, 12, 12, 4)], 32) + two,
            "B": ([make_arch("image", 784, 130, 70, 20), make_arch("joint", 147, 65, 35, 20)], 64) + two,
            "C": (conv["archs"], conv["B"]) + two,
            "Cg": (conv["archs"], conv["B"]) + two,
            "D": ([make_arch("image", 60, 20, 16, 3), make_arch("joint", 21, 12, 10, 3), make_arch("aux", 17, 8, 8, 3)], 8) + three}


MODELS = _models()


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


PLAN_ENV = {"Cg": {"AVAE_NO_LEAN_LOSS": "1"}}           # planner switches, read while the handle plans its step


def make(V, name, dtype, schedule=None, lam=LAM, lr=LR, **kw):
    archs, B, binary, w, act = MODELS[name]
    env = PLAN_ENV.get(name, {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        model, ref = build_pair(V, archs, binary, w, lam, act, B, dtype, lr=lr, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if schedule is not None:
        model.set_schedule(**schedule)
    return model, ref


_DATA = {}


def data(name, steps, seed=11):
    """the first `steps` of 21 batches (computed once per model and seed, shared, never written to)"""
    archs, B, binary = MODELS[name][:3]
    if (name, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = synth_batch(rng, 21 * B, [a["n_input"] for a in archs], binary)
        _DATA[(name, seed)] = (X, rng.standard_normal((21 * B, archs[0]["n_z"])).astype(np.float32))
    X, eps = _DATA[(name, seed)]
    return [x[:steps * B] for x in X], eps[:steps * B], B


def rows(X, eps, B, i):
    return [x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B]


def same_state(a, b):
    sa, sb = opt_snapshot(a), opt_snapshot(b)
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(sa[:3], sb[:3])) and sa[3] == sb[3]


def same_history(a, b, n):
    ha, hb = a.hyper_history(n), b.hyper_history(n)
    return ha[0].tobytes() == hb[0].tobytes() and ha[1] == hb[1]


def check_history(hist, first_t, kl=KL, assoc=ASSOC, lr=LRS, lam=LAM, lr0=LR):
    """rows of hyper_history against the reference: the piecewise columns (and their fp32 product with lambda) bitwise, an EXP
    multiplier within one fp32 ulp -- the learning-rate column must be the fp32 product of learning_rate with such a value"""
    assert hist.dtype == np.float32 and hist.shape[1] == 3
    for i, (k, l, r) in enumerate(hist):
        t = first_t + i
        wk, wl, _ = hyper(kl, assoc, None, lam, lr0, t)
        assert k.tobytes() == wk.tobytes() and l.tobytes() == wl.tobytes(), (t, k, wk, l, wl)
        m = schedule_value(lr, t)
        near = [np.nextafter(m, F32(0)), m, np.nextafter(m, F32(np.inf))]
        assert all(ulp_distance(x, m) <= 1 for x in near)
        assert any(r.tobytes() == (F32(lr0) * x).tobytes() for x in near), (t, r, F32(lr0) * m)


# ----------------------------------------------------------------------------- 1. history
def test_history_matches_the_evaluator(V):
    X, eps, B = data("A", 21)
    m, _ = make(V, "A", "bf16", SCHED)
    m.partial_fit_steps(X, 21, eps)                       # 16 + 4 + 1
    hist, last = m.hyper_history(21)
    assert last == 21
    check_history(hist, 1)
    assert hist[0, 0] == 0 and hist[0, 1] == 0 and hist[0, 2] == F32(LR), "the first step: u = 0"
    assert hist[5, 0] == F32(0.5) and hist[20, 0] == 1 and hist[7, 1] == 0 and hist[10, 1] == F32(LAM)
    # the counter restored beyond 2^31: the schedules go on from there
    big = 2 ** 31 + 3
    th, mm, vv, _t = opt_snapshot(m)
    m.set_opt_state(mm, vv, big)
    m.partial_fit_steps(X, 21, eps)
    hist, last = m.hyper_history(21)
    assert last == big + 21
    check_history(hist, big + 1)
    assert np.all(hist[:, 0] == 1)


# ----------------------------------------------------------------------------- 2. beta against fp64
BETA = dict(knots=[(0, 0), (1, 0.37), (2, 1)])


@pytest.mark.parametrize("name,dtype", [("A", "fp32"), ("B", "fp32"), ("D", "fp32"), ("A", "bf16")])
def test_kl_multiplier_against_fp64(V, name, dtype):
    """Cost and gradient of steps 1-3 (kl_t = 0, 0.37, 1) at the handle's own weights of each step against the torch fp64
    restatement: the project's fp32 tolerances (cost 1e-5, gradients 1e-4 of the tensor maximum); bf16: the
    cost within 1e-3."""
    archs, B, binary, w, act = MODELS[name]
    X, eps, _ = data(name, 3)
    model, _ = make(V, name, dtype, dict(kl=BETA))
    for s, kl in enumerate((0.0, 0.37, 1.0)):
        x, e = rows(X, eps, B, s)
        th = model.get_params().astype(np.float64)
        cost = model.partial_fit(x, e)
        g = model.get_grads()
        h = model.hyper_history(1)[0][0]
        assert h[0] == F32(kl) and h[1] == F32(LAM) and h[2] == F32(LR)
        masks = hip_relu_masks(model, archs) if act == "relu" else None
        c_ref, g_ref = scheduled_cost_and_grads(archs, th, x, e, binary, w, LAM, act, kl=float(F32(kl)), masks=masks)
        rel = abs(cost - c_ref) / abs(c_ref)
        errs = per_tensor_err(archs, g.astype(np.float64), g_ref)
        worst = max(errs, key=lambda kv: kv[1])
        print("model %s %s step %d kl %.2f: cost %.7g fp64 %.7g rel %.2e; worst gradient tensor %s %.2e" %
              ((name, dtype, s + 1, kl, cost, c_ref, rel) + worst))
        if dtype == "fp32":
            assert rel <= 1e-5
            assert worst[1] <= 1e-4, worst
        else:
            assert rel <= 1e-3


# ----------------------------------------------------------------------------- 3. lambda and lr twins
TWIN = dict(assoc=dict(knots=[(0, 0.25), (4, 1.5)]), lr=dict(decay_rate=0.7, decay_steps=3, staircase=False))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C", "Cg"])
def test_scheduled_lambda_and_lr_equal_configured_ones_bitwise(V, name, dtype):
    """Step t of a scheduled handle against an unscheduled handle built with assoc_lambda = lambda_t and learning_rate =
    lr_eff_t (both from the device's own history) on the same theta, m, v and step counter: equal in every bit."""
    X, eps, B = data(name, 3)
    sch, _ = make(V, name, dtype, TWIN)
    for t in (1, 3):
        while opt_snapshot(sch)[3] < t - 1:
            sch.partial_fit(*rows(X, eps, B, opt_snapshot(sch)[3]))
        before = opt_snapshot(sch)
        assert before[3] == t - 1
        x, e = rows(X, eps, B, t - 1)
        c_s = sch.partial_fit(x, e)
        g_s, after = sch.get_grads(), opt_snapshot(sch)
        (kl_t, lam_t, lr_t), last = sch.hyper_history(1)[0][0], sch.hyper_history(1)[1]
        assert last == t and kl_t == 1
        wk, wl, _ = hyper(None, TWIN["assoc"], None, LAM, LR, t)
        assert lam_t.tobytes() == wl.tobytes() and lam_t != F32(LAM) and (t == 1 or lr_t != F32(LR))
        plain, _ = make(V, name, dtype, lam=float(lam_t), lr=float(lr_t))
        plain.set_params(before[0])
        plain.set_opt_state(before[1], before[2], before[3])
        c_p = plain.partial_fit(x, e)
        assert F32(c_s).tobytes() == F32(c_p).tobytes(), (t, c_s, c_p)
        assert np.array_equal(g_s, plain.get_grads()), "gradient, step %d" % t
        assert same_state(sch, plain), "theta / m / v / counter, step %d" % t
        assert shadow_err(sch)[:2] == (0.0, 0.0) and shadow_err(plain)[:2] == (0.0, 0.0)
        check_adam_step(before, after, g_s, float(lr_t))
        del plain


LEAN_CFGS = (7, 9, 10, 11, 12, 13)                      # the lean small-net kernels' tile configurations (tests/plan_dump.py)
K_COST = 8


def test_conv_model_covers_the_grouped_kernel(V, monkeypatch, capfd):
    """Where model C's latent and cost items run (see the module docstring): the cost item on k_grouped in either plan, the
    latent item on k_grouped under AVAE_NO_LEAN_LOSS=1 (model Cg) and in the lean loss launch otherwise."""
    archs, B, binary, w, act = MODELS["C"]
    X, eps, _ = data("C", 1)
    for name, lean_latent in (("C", True), ("Cg", False)):
        plan = plan_dump.step_plan(V, monkeypatch, capfd, archs, B, "bf16", X, eps, env=PLAN_ENV.get(name), binary=binary,
                                   transfer_fct=act, weights=w, assoc_lambda=LAM)
        lat = [(n, c) for n, c, items in plan if any(it[0] == plan_dump.K_LATENT for it in items)]
        cost = [(n, c) for n, c, items in plan if any(it[0] == K_COST for it in items)]
        assert len(lat) == 1 and len(cost) == 1, (lat, cost)
        assert cost[0][1] not in LEAN_CFGS, (name, cost)
        assert (lat[0][1] in LEAN_CFGS) == lean_latent, (name, lat)


# ----------------------------------------------------------------------------- 4. unit multipliers
def launches(m, X, eps):
    assert m._L.avae_timing_enable(m._h, 1) == 0
    m.partial_fit_steps(X, 2, eps)
    buf = C.create_string_buffer(1 << 16)
    assert m._L.avae_timing_report(m._h, buf, len(buf)) == 0 and m._L.avae_timing_enable(m._h, 0) == 0
    return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}


@pytest.mark.parametrize("name", ["A", "B", "C", "Cg"])
def test_unit_multipliers_are_the_plain_step_bitwise(V, name):
    dtype = "bf16"
    X, eps, B = data(name, 6)
    plain, _ = make(V, name, dtype)

    def run(m, lo, hi):
        out = []
        for i in range(lo, hi):
            x, e = rows(X, eps, B, i)
            out.append((m.partial_fit(x, e), m.get_grads()))
        return out

    def check(got, want, b, what):
        for s, ((c0, g0), (c1, g1)) in enumerate(zip(want, got)):
            assert c0 == c1 and np.array_equal(g0, g1), "%s: step %d" % (what, s)
        assert same_state(plain, b), what
        assert shadow_err(b)[:2] == (0.0, 0.0), what

    want = run(plain, 0, 4)
    const, _ = make(V, name, dtype, dict(kl=1.0, assoc=1.0, lr=1.0))
    check(run(const, 0, 4), want, const, "constant 1")
    assert np.array_equal(const.hyper_history(4)[0], np.tile(np.array([1.0, LAM, LR], F32), (4, 1)))
    flat = dict(knots=[(0, 1), (10, 1), (20, 0)])
    piece, _ = make(V, name, dtype, dict(kl=flat, assoc=flat, lr=flat))
    check(run(piece, 0, 4), want, piece, "piecewise, 1 at the tested steps")
    # the scheduled step has exactly the launches of the unscheduled one; so has the handle after switching off again
    X2, eps2, _ = data(name, 2, seed=12)
    off = launches(plain, X2, eps2)
    assert launches(const, X2, eps2) == off, "a scheduled step must not add or rename a launch"
    assert same_state(plain, const)
    want = run(plain, 4, 6)
    const.set_schedule()
    check(run(const, 4, 6), want, const, "after set_schedule()")
    assert launches(const, X2, eps2) == launches(plain, X2, eps2) == off
    with pytest.raises(RuntimeError):
        const.hyper_history(1)


# ----------------------------------------------------------------------------- 5. routes
@pytest.mark.parametrize("clip", [None, dict(max_norm=float("inf"))])
def test_routes_agree_bitwise(V, clip):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 21)
    kw = {} if clip is None else dict(grad_clip=clip)
    run, _ = make(V, name, dtype, SCHED, **kw)
    p_init = run.get_params()
    run.partial_fit_steps(X, 21, eps)                      # 16 + 4 + 1
    check_history(run.hyper_history(21)[0], 1)

    def agrees(other, what):
        assert same_state(run, other), what
        assert np.array_equal(run.cost_history(21), other.cost_history(21)), what
        assert same_history(run, other, 21), what

    single, _ = make(V, name, dtype, SCHED, **kw)
    for i in range(21):
        single.partial_fit(*rows(X, eps, B, i))
    agrees(single, "21 single steps")
    eager, _ = make(V, name, dtype, SCHED, use_graph=False, **kw)
    eager.partial_fit_steps(X, 21, eps)
    agrees(eager, "use_graph=0")
    masked, _ = make(V, name, dtype, SCHED, **kw)
    masked.partial_fit_steps(X, 21, eps, present=np.ones((21 * B, 2), np.uint8))
    agrees(masked, "all-present masks")
    given, _ = make(V, name, dtype, SCHED, **kw)
    given.partial_fit_steps(X, 21, eps, inputs=X)
    agrees(given, "inputs= equal to X")
    ctor = V.AssocVariationalAutoEncoder(MODELS[name][0], binary=MODELS[name][2], transfer_fct="relu", weights=MODELS[name][3],
                                         assoc_lambda=LAM, learning_rate=LR, batch_size=B, compute_dtype=dtype, seed=5,
                                         schedule=SCHED, **kw)
    ctor.set_params(p_init)
    ctor.partial_fit_steps(X, 21, eps)
    agrees(ctor, "the schedule= keyword of the constructor")
    if clip is None:
        # the schedule did change the run
        plain, _ = make(V, name, dtype)
        plain.partial_fit_steps(X, 21, eps)
        assert not np.array_equal(plain.cost_history(21), run.cost_history(21))
        return
    # monitor-only clipping is bitwise the unclipped scheduled run
    unclipped, _ = make(V, name, dtype, SCHED)
    unclipped.partial_fit_steps(X, 21, eps)
    agrees(unclipped, "max_norm=inf against no clipping")
    # a poisoned, skipped step still consumes its step number: the schedule goes on
    bad = [X[0], X[1].copy()]
    bad[1][5 * B + 3, 7] = np.nan
    skip = dict(max_norm=float("inf"), skip_nonfinite=True)
    a, _ = make(V, name, dtype, SCHED, grad_clip=skip)
    a.partial_fit_steps(bad, 21, eps)
    b, _ = make(V, name, dtype, SCHED, grad_clip=skip)
    for i in range(21):
        b.partial_fit(*rows(bad, eps, B, i))
    assert same_state(a, b) and np.all(np.isfinite(opt_snapshot(a)[0]))
    for m in (a, b):
        assert m.grad_norm_history(21)[1:] == (21, 1)
        assert list(np.flatnonzero(np.isnan(m.cost_history(21)))) == [5]
        assert same_history(m, run, 21), "the skipped step must not shift the schedule"


# ----------------------------------------------------------------------------- 6. data parallel on one GPU
@pytest.mark.parametrize("comm", ["ipc", "library"])
@pytest.mark.parametrize("buckets", [1, 2])
def test_one_rank_pipeline_is_the_plain_scheduled_step(V, comm, buckets):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 21)
    plain, _ = make(V, name, dtype, SCHED)
    plain.partial_fit_steps(X, 21, eps)
    dp, _ = make(V, name, dtype, SCHED, comm=comm, comm_buckets=buckets)
    assert dp._comm_lib and len(dp._buckets) == buckets
    dp.partial_fit_steps(X, 21, eps)
    assert same_state(plain, dp)
    assert np.array_equal(plain.cost_history(21), dp.cost_history(21))
    assert same_history(plain, dp, 21)
    check_history(dp.hyper_history(21)[0], 1)


def test_host_owned_seam_two_scheduled_replicas_equal_the_global_batch(V):
    """Two replicas (row_offset / batch_global) through avae_stage_batches -> avae_dp_backward -> avae_dp_apply at step 3 of the
    schedules: their summed gradient equals the scheduled global-batch replica's to accumulation-order rounding (the bounds of
    test_two_shard_replicas_sum_to_global_batch), both apply it with the scheduled learning rate, bitwise alike."""
    from vae_assoc_amd import _capi
    name, dtype = "A", "fp32"
    archs, B, binary, w, act = MODELS[name]
    X, eps, _ = data(name, 2)                              # a global batch of 2 * B rows
    sched = dict(kl=0.37, assoc=TWIN["assoc"], lr=TWIN["lr"])
    kw = dict(binary=binary, transfer_fct=act, weights=w, assoc_lambda=LAM, learning_rate=LR, compute_dtype=dtype, seed=2)
    full = V.AssocVariationalAutoEncoder(archs, batch_size=2 * B, schedule=sched, **kw)
    p0 = full.get_params()
    zeros = np.zeros_like(p0)
    full.set_opt_state(zeros, zeros, 2)
    full._backward(X, eps)
    torch.cuda.synchronize()
    g_full = full._grad_tensor().clone()
    reps = []
    for r in range(2):
        rep = V.AssocVariationalAutoEncoder(archs, batch_size=B, **kw)
        rep._L.avae_destroy(rep._h)
        rep._cfg.row_offset, rep._cfg.batch_global = B * r, 2 * B
        h = C.c_void_p()
        _capi.check(None, rep._L.avae_create(C.byref(rep._cfg), C.byref(h)), "avae_create")
        rep._h = h
        rep.set_params(p0)
        rep.set_opt_state(zeros, zeros, 2)
        rep.set_schedule(**sched)
        if r == 0:
            before = opt_snapshot(rep)
        rep._backward(*rows(X, eps, B, r))
        reps.append(rep)
    torch.cuda.synchronize()
    gsum = reps[0]._grad_tensor() + reps[1]._grad_tensor()
    gf, gs = g_full.cpu().numpy().astype(np.float64), gsum.cpu().numpy().astype(np.float64)
    assert abs(gf[-1] - gs[-1]) <= 1e-5 * abs(gf[-1])
    assert np.abs(gf[:-1] - gs[:-1]).max() <= 2e-5 * np.abs(gf[:-1]).max()
    # the unscheduled global-batch gradient is another one
    plain = V.AssocVariationalAutoEncoder(archs, batch_size=2 * B, **kw)
    plain._backward(X, eps)
    torch.cuda.synchronize()
    assert abs(plain._grad_tensor()[-1].item() - gf[-1]) > 1e-4 * abs(gf[-1])
    for rep in reps:
        rep._grad_tensor().copy_(gsum)
    torch.cuda.synchronize()
    g = reps[0].get_grads()
    for rep in reps:
        rep._apply()
    assert same_state(reps[0], reps[1]) and same_history(reps[0], reps[1], 1)
    hist, last = reps[0].hyper_history(1)
    assert last == 3
    check_history(hist, 3, kl=0.37, assoc=TWIN["assoc"], lr=TWIN["lr"])
    check_adam_step(before, opt_snapshot(reps[0]), g, float(hist[0, 2]))
    assert shadow_err(reps[0])[:2] == (0.0, 0.0) and shadow_err(reps[1])[:2] == (0.0, 0.0)


# ----------------------------------------------------------------------------- 7. resume
def test_resume_continues_the_schedule(V, tmp_path):
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 6)
    straight, _ = make(V, name, dtype, SCHED)
    straight.partial_fit_steps(X, 6, eps)
    first, _ = make(V, name, dtype, SCHED)
    first.partial_fit_steps([x[:3 * B] for x in X], 3, eps[:3 * B])
    first.save_model(os.path.join(str(tmp_path), "m.ckpt"))
    second, _ = make(V, name, dtype, seed=99)
    second.set_schedule(**SCHED)                           # (schedules are not part of the file)
    second.restore_model(folder=str(tmp_path))
    assert opt_snapshot(second)[3] == 3
    second.partial_fit_steps([x[3 * B:] for x in X], 3, eps[3 * B:])
    assert same_state(straight, second)
    assert np.array_equal(straight.cost_history(3), second.cost_history(3))
    assert same_history(straight, second, 3)
    check_history(second.hyper_history(3)[0], 4)


# ----------------------------------------------------------------------------- 8. evaluation is untouched
def bitwise(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(bitwise(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(bitwise(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_evaluation_and_inference_never_read_a_schedule(V):
    name, dtype = "A", "bf16"
    archs, B = MODELS[name][:2]
    X, eps, _ = data(name, 2)
    x, e = rows(X, eps, B, 1)
    wild = dict(kl=0.0, assoc=5.0, lr=dict(decay_rate=0.1, decay_steps=1))
    sch, _ = make(V, name, dtype, wild)
    sch.partial_fit(*rows(X, eps, B, 0))                   # the schedule is live: a step has run under it
    plain, _ = make(V, name, dtype)
    plain.set_params(sch.get_params())
    P = np.ones((B, 2), np.uint8)
    P[::3, 1] = 0
    rng = np.random.default_rng(3)
    e4 = rng.standard_normal((B, 4, archs[0]["n_z"])).astype(np.float32)
    for m in (sch, plain):
        m.calls = dict(cost=m.evaluate_cost(x, e), masked=m.evaluate_cost(x, e, present=P),
                       score=m.score_samples(x, e, cross_modal=True), loglik=m.log_likelihood(x, n_samples=4, eps=e4),
                       impute=m.impute(x, present=P), impute_k=m.impute(x, present=P, n_samples=4, eps=e4))
    for k in sch.calls:
        assert bitwise(sch.calls[k], plain.calls[k]), k
    assert np.isfinite(sch.calls["cost"]) and sch.calls["cost"] != sch.cost_history(1)[0]
    # ... and a training step after them still reads it
    sch.partial_fit(x, e)
    hist, last = sch.hyper_history(2)
    assert last == 2 and hist[1, 0] == 0 and hist[1, 1] == F32(LAM) * F32(5.0) and ulp_distance(hist[1, 2], F32(LR) * F32(0.1)) <= 1


# ----------------------------------------------------------------------------- 9. errors, train()
def test_errors(V):
    from vae_assoc_amd import _capi
    m, _ = make(V, "A", "bf16")
    L, h = m._L, m._h
    out = np.zeros(3 * 8192, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.avae_hyper_history(h, 0, p, None) == 0              # fine on a handle that never had a schedule
    assert L.avae_hyper_history(h, 1, p, None) != 0
    bad = _capi.Schedule()
    bad.kind, bad.n_knots = _capi.SCHED_PIECEWISE, 2
    bad.knot_step[0], bad.knot_step[1] = 4, 4
    for pos, who in enumerate(("kl", "assoc", "lr")):
        args = [None, None, None]
        args[pos] = C.byref(bad)
        assert L.avae_set_schedule(h, *args) != 0
        msg = L.avae_last_error(h)
        assert who.encode() in msg and b"knot_step[1]" in msg, msg
    bad.kind, bad.decay_rate, bad.decay_steps = _capi.SCHED_EXP, 0.5, 0
    assert L.avae_set_schedule(h, None, None, C.byref(bad)) != 0 and b"decay_steps" in L.avae_last_error(h)
    # a refused call changes nothing: the handle is still unscheduled
    X, eps, B = data("A", 2)
    m.partial_fit_steps(X, 2, eps)
    assert L.avae_hyper_history(h, 1, p, None) != 0
    m.set_schedule(kl=0.5)
    m.partial_fit_steps(X, 2, eps)
    assert L.avae_hyper_history(h, 4097, p, None) != 0           # above the history depth
    assert L.avae_hyper_history(h, 3, p, None) != 0              # above the steps since switch-on
    assert m.hyper_history(2)[0].shape == (2, 3) and m.hyper_history(0)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="knot_value"):
        m.set_schedule(kl=-1.0)
    with pytest.raises(ValueError, match="decay_rate"):
        V.AssocVariationalAutoEncoder(MODELS["A"][0], batch_size=8, schedule=dict(lr=dict(decay_rate=-1, decay_steps=3)))
    with pytest.raises(ValueError, match="unit"):
        V.AssocVariationalAutoEncoder(MODELS["A"][0], batch_size=8, schedule=dict(kl=0.5, unit="epoch"))
    with pytest.raises(RuntimeError):
        m.hyper_history(3)


def test_train_converts_epochs_on_a_device_data_set(V):
    from vae_assoc_amd import dataset, linear_warmup, exponential_decay
    archs = [make_arch("image", 784, 16, 12, 4), make_arch("joint", 147, 12, 8, 4)]
    rng = np.random.default_rng(6)
    data_ = np.concatenate(synth_batch(rng, 100, [784, 147], [True, False]), axis=1)
    np.random.seed(11)
    ds = dataset.to_device(dataset.construct_datasets(data_.copy()))
    B = ds.train._data.shape[0] // 4                      # four batches per epoch
    assert ds.train._data.shape[0] // B == 4
    sched = dict(kl=linear_warmup(1.5), lr=exponential_decay(0.5, 1, staircase=True), unit="epoch")
    with pytest.raises(ValueError, match="decay_steps"):
        V.train(ds, archs, binary=[True, False], batch_size=B, training_epochs=1, schedule=dict(lr=exponential_decay(0.5, 0), unit="epoch"))
    model, hist = V.train(ds, archs, binary=[True, False], assoc_lambda=LAM, learning_rate=LR, batch_size=B, training_epochs=2,
                          display_step=10, compute_dtype="bf16", seed=3, schedule=sched)
    assert len(hist) == 8
    h, last = model.hyper_history(8)
    assert last == 8
    check_history(h, 1, kl=dict(knots=[(0, 0), (6, 1)]), assoc=None, lr=dict(decay_rate=0.5, decay_steps=4, staircase=True))
    assert h[0, 0] == 0 and h[3, 0] == F32(0.5) and h[6, 0] == 1 and h[3, 2] == F32(LR) and h[4, 2] == F32(LR) * F32(0.5)
