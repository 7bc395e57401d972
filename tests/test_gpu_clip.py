"""Global-norm gradient clipping and non-finite step skipping on the MI355X (include/avae.h, avae_set_grad_clip; DESIGN.md
section 15), against the kernel's own arithmetic (check_adam_step on the device's recorded norm), the fp64 reference
(tests/clip_reference.py) and, bitwise, against the unclipped step wherever the factor is 1.

Shapes: model A = the fused small-net plan (784-24-24 / 147-12-12, n_z 4, B 32), model B = edge tiles and a partial last quad
(784-130-70 / 147-65-35, n_z 20, B 64), model C = the conv model of tests/golden/conv_small.npz's shape (k_adam's adjoint-shadow
path).  relu, weights [50, 1], assoc_lambda 8."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from clip_reference import clipped_step
from oracle import vae_assoc_oracle as O
from test_gpu_parity import _load_big, build_pair, check_adam_step, opt_snapshot, shadow_err, synth_batch
from conftest import make_arch

pytestmark = pytest.mark.gpu

BIN, W, LAM, ACT, LR = [True, False], [50, 1], 8.0, "relu", 1e-3
F32 = np.float32


def _models():
    conv = _load_big().SMALL["conv_small"][0]
    return {"A": ([make_arch("image", 784, 24, 24, 4), make_arch("joint", 147, 12, 12, 4)], 32),
            "B": ([make_arch("image", 784, 130, 70, 20), make_arch("joint", 147, 65, 35, 20)], 64),
            "C": (conv["archs"], conv["B"])}


MODELS = _models()


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def make(V, name, dtype, clip=None, **kw):
    archs, B = MODELS[name]
    model, ref = build_pair(V, archs, BIN, W, LAM, ACT, B, dtype, lr=LR, **kw)
    if clip is not None:
        model.set_grad_clip(**clip)
    return model, ref


_DATA = {}


def data(name, steps, seed=11):
    """the first `steps` of 20 batches (computed once per model and seed, shared, never written to)"""
    archs, B = MODELS[name]
    if (name, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = synth_batch(rng, 20 * B, [a["n_input"] for a in archs], BIN)
        _DATA[(name, seed)] = (X, rng.standard_normal((20 * B, archs[0]["n_z"])).astype(np.float32))
    X, eps = _DATA[(name, seed)]
    return [x[:steps * B] for x in X], eps[:steps * B], B


def rows(X, eps, B, i):
    return [x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B]


def state(model):
    th, m, v, t = opt_snapshot(model)
    return th, m, v, t


def same_state(a, b):
    sa, sb = state(a), state(b)
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(sa[:3], sb[:3])) and sa[3] == sb[3]


_N0 = {}


def first_norm(V, name, dtype):
    """(norm, raw gradient) of the first step of the model on data(name, ...), measured once on a monitoring twin"""
    if (name, dtype) not in _N0:
        twin, _ = make(V, name, dtype, clip=dict(max_norm=float("inf")))
        X, eps, B = data(name, 1)
        twin.partial_fit(X, eps)
        _N0[(name, dtype)] = (float(twin.grad_norm_history(1)[0][0]), twin.get_grads())
    return _N0[(name, dtype)]


def factor(max_norm, norm):
    """the kernel's c: one fp32 division behind a select"""
    mx, n = F32(max_norm), F32(norm)
    return mx / n if (mx > 0 and n > mx) else F32(1.0)


# k_grad_sumsq's shape, mirrored from avae_device.h: kSumsqThreads, kSumsqMaxBlocks, kSumsqQuads, sumsq_blocks(), sumsq_chain()
SUMSQ_THREADS, SUMSQ_MAX_BLOCKS, SUMSQ_QUADS = 256, 256, 8


def sumsq_shape(p_int):
    quads = p_int // 4
    G = min(max(-(-quads // (SUMSQ_THREADS * SUMSQ_QUADS)), 1), SUMSQ_MAX_BLOCKS)
    return G, -(-quads // (SUMSQ_THREADS * G))


# ----------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_norm_accuracy_and_determinism(V, name, dtype):
    """The recorded norm against the fp64 norm of get_grads() -- the very fp32 values the kernel summed.  Bound on s = sum g^2,
    derived: every accumulator makes at most L sequential fused multiply-adds (its chain of sumsq_chain(P_int) quads) plus the two
    adds that join a thread's four accumulators; the shuffle tree, the cross-wave sum and the sum of the G partials add
    log2(threads * G) levels; + 3 for the squares and the final adds.  Each level costs 2^-24 relative (all terms are >= 0).  The
    norm's bound is half of it plus 2^-24 for the root."""
    X, eps, B = data(name, 1)
    norms = []
    for _ in range(2):
        m, _ = make(V, name, dtype, clip=dict(max_norm=float("inf")))
        m.partial_fit(X, eps)
        h, last, skipped = m.grad_norm_history(1)
        assert last == 1 and skipped == 0 and h.dtype == np.float32
        norms.append(h[0])
    assert norms[0].tobytes() == norms[1].tobytes(), "the norm differs between two handles on the same inputs"
    p_int = m._grad_tensor().numel() - 1
    assert p_int % 32 == 0
    G, chain = sumsq_shape(p_int)
    L = chain + 2
    bound_s = (L + math.ceil(math.log2(SUMSQ_THREADS * G)) + 3) * 2.0 ** -24
    want = float(np.sqrt(np.sum(m.get_grads().astype(np.float64) ** 2)))
    rel = abs(float(norms[0]) - want) / want
    print("model %s %s: P_int %d G %d chain %d norm %.9g fp64 %.9g rel %.3e bound %.3e" % (name, dtype, p_int, G, chain, norms[0], want,
                                                                                       rel, 0.5 * bound_s + 2.0 ** -24))
    assert want > 0 and rel <= 0.5 * bound_s + 2.0 ** -24
    if name != "C":
        assert G > 1, "the test shape must take more than one workgroup"


# ----------------------------------------------------------------------------- 2. c == 1 is today's step, bit for bit
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_monitor_only_is_bitwise_the_plain_step(V, name, dtype):
    X, eps, B = data(name, 6)
    plain, _ = make(V, name, dtype)

    def run(m, lo, hi):
        out = []
        for i in range(lo, hi):
            x, e = rows(X, eps, B, i)
            out.append((m.partial_fit(x, e), m.get_grads()))
        return out

    want = run(plain, 0, 4)
    mon, _ = make(V, name, dtype, clip=dict(max_norm=float("inf")))
    got = run(mon, 0, 4)
    norms = mon.grad_norm_history(4)[0]
    assert np.all(np.isfinite(norms)) and np.all(norms > 0)

    def check(got, a, b, what):
        for s, ((c0, g0), (c1, g1)) in enumerate(zip(want, got)):
            assert c0 == c1 and np.array_equal(g0, g1), "%s: step %d" % (what, s)
        assert same_state(a, b), what
        assert shadow_err(b)[:2] == (0.0, 0.0), what

    check(got, plain, mon, "monitor only")
    loose, _ = make(V, name, dtype, clip=dict(max_norm=4.0 * float(norms.max())))
    check(run(loose, 0, 4), plain, loose, "max_norm above every norm")
    assert np.array_equal(loose.grad_norm_history(4)[0], norms)
    # switched off again: the previous plan (the fused launch and its graphs) is back
    mon.set_grad_clip(0.0, False)
    want, got = run(plain, 4, 6), run(mon, 4, 6)
    check(got, plain, mon, "after set_grad_clip(0, False)")
    X20, eps20, _ = data(name, 20, seed=12)
    plain.partial_fit_steps(X20, 20, eps20)
    mon.partial_fit_steps(X20, 20, eps20)
    assert same_state(plain, mon) and np.array_equal(plain.cost_history(26), mon.cost_history(26))


# ----------------------------------------------------------------------------- 3. active clipping
def clipped_steps(model, X, eps, B, max_norm, steps, present=None, g_first=None):
    """`steps` single steps; each checked against the kernel's arithmetic on f32(g) * f32(c), c from the device's recorded norm.
    g_first: what the gradient buffer must hold after the first step, bitwise."""
    costs = []
    for s in range(steps):
        x, e = rows(X, eps, B, s)
        before = opt_snapshot(model)
        kw = {} if present is None else dict(present=present[s * B:(s + 1) * B])
        costs.append(model.partial_fit(x, e, **kw))
        g = model.get_grads()
        norm = model.grad_norm_history(1)[0][0]
        c = factor(max_norm, norm)
        print("step %d: norm %.7g max_norm %.7g c %.6f" % (s, norm, max_norm, c))
        if present is None:
            assert c < 1.0, "step %d is not clipped (norm %r, max_norm %r)" % (s, norm, max_norm)
        if s == 0 and g_first is not None:
            assert np.array_equal(g, g_first), "the gradient buffer must keep the raw gradient"
        check_adam_step(before, opt_snapshot(model), g.astype(F32) * c, LR)
        assert shadow_err(model)[:2] == (0.0, 0.0), "step %d" % s
    return costs


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_active_clipping(V, name, dtype):
    n0, g_twin = first_norm(V, name, dtype)
    mx = 0.5 * n0
    X, eps, B = data(name, 3)
    model, ref = make(V, name, dtype, clip=dict(max_norm=mx))
    p0 = model.get_params().astype(np.float64)
    costs = clipped_steps(model, X, eps, B, mx, 3, g_first=g_twin)
    # costs against the fp64 reference run like for like
    emu = ref if dtype == "fp32" else O.OracleAssocVAE(MODELS[name][0], BIN, ACT, W, LAM, LR, B, params_flat=p0, quant="bf16")
    tol = 1e-5 if dtype == "fp32" else 5e-5
    for s in range(3):
        x, e = rows(X, eps, B, s)
        r = clipped_step(emu, x, e, max_norm=mx)
        rel = abs(costs[s] - r["cost"]) / abs(r["cost"])
        print("model %s %s step %d: cost %.7g reference %.7g rel %.2e (c %.4f)" % (name, dtype, s, costs[s], r["cost"], rel, r["c"]))
        assert r["c"] < 1.0
        assert rel <= tol, "step %d cost %.7g vs reference %.7g" % (s, costs[s], r["cost"])


# ----------------------------------------------------------------------------- 4. replays and twins
def test_replays_masks_and_eager_are_bitwise(V):
    name, dtype = "A", "bf16"
    n0, _ = first_norm(V, name, dtype)
    clip = dict(max_norm=0.5 * n0)
    X, eps, B = data(name, 20)
    run, _ = make(V, name, dtype, clip=clip)
    c_before = run.evaluate_cost(*rows(X, eps, B, 0))
    run.partial_fit_steps(X, 20, eps)                      # one 16-step and one 4-step replay
    single, _ = make(V, name, dtype, clip=clip)
    for i in range(20):
        single.partial_fit(*rows(X, eps, B, i))
    assert same_state(run, single)
    assert np.array_equal(run.cost_history(20), single.cost_history(20))
    nr, ns = run.grad_norm_history(20), single.grad_norm_history(20)
    assert np.array_equal(nr[0], ns[0]) and nr[1:] == ns[1:] == (20, 0)
    assert nr[0][0] > F32(clip["max_norm"]) and np.sum(nr[0] > F32(clip["max_norm"])) >= 3, "the run must hold clipped steps"

    masked, _ = make(V, name, dtype, clip=clip)
    masked.partial_fit_steps(X, 20, eps, present=np.ones((20 * B, 2), np.uint8))
    assert same_state(run, masked) and np.array_equal(run.grad_norm_history(20)[0], masked.grad_norm_history(20)[0])

    eager, _ = make(V, name, dtype, clip=clip, use_graph=False)
    eager.partial_fit_steps(X, 20, eps)
    assert same_state(run, eager) and np.array_equal(run.grad_norm_history(20)[0], eager.grad_norm_history(20)[0])

    # half of the rows carry the image alone
    P = np.ones((3 * B, 2), np.uint8)
    P[::2, 1] = 0
    part, _ = make(V, name, dtype)
    part.partial_fit(*rows(X, eps, B, 0), present=P[:B])    # (the masked twin exists before clipping is switched on)
    part.set_grad_clip(**clip)
    clipped_steps(part, X, eps, B, clip["max_norm"], 3, present=P)

    # evaluation is untouched by the setting
    fresh, _ = make(V, name, dtype)
    assert fresh.evaluate_cost(*rows(X, eps, B, 0)) == c_before
    fresh.set_grad_clip(**clip)
    assert fresh.evaluate_cost(*rows(X, eps, B, 0)) == c_before


# ----------------------------------------------------------------------------- 5. skipping
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_nonfinite_step_is_skipped(V, name, dtype):
    X, eps, B = data(name, 20)
    bad = [X[0], X[1].copy()]
    bad[1][5 * B + 3, 7] = np.nan                          # one NaN in a present element of the joint modality, batch 5
    model, _ = make(V, name, dtype, clip=dict(skip_nonfinite=True))
    model.partial_fit(*rows(X, eps, B, 0))
    before = opt_snapshot(model)
    c = model.partial_fit(*rows(bad, eps, B, 5))
    after = opt_snapshot(model)
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])), "a skipped step wrote parameters or moments"
    assert shadow_err(model)[:2] == (0.0, 0.0)
    norms, last, skipped = model.grad_norm_history(2)
    assert after[3] == before[3] + 1 == last and skipped == 1
    assert np.isfinite(norms[0]) and not np.isfinite(norms[1])
    assert np.isnan(c) and np.isnan(model.cost_history(1)[0])
    before = after
    model.partial_fit(*rows(X, eps, B, 1))
    check_adam_step(before, opt_snapshot(model), model.get_grads(), LR)
    assert model.grad_norm_history(1)[2] == 1

    # inside a replay: 20 batches, the NaN batch at index 5
    run, _ = make(V, name, dtype, clip=dict(skip_nonfinite=True))
    run.partial_fit_steps(bad, 20, eps)
    single, _ = make(V, name, dtype, clip=dict(skip_nonfinite=True))
    for i in range(20):
        single.partial_fit(*rows(bad, eps, B, i))
    assert same_state(run, single) and np.all(np.isfinite(state(run)[0]))
    for m in (run, single):
        norms, last, skipped = m.grad_norm_history(20)
        assert last == 20 and skipped == 1
        assert list(np.flatnonzero(~np.isfinite(norms))) == [5]
        assert list(np.flatnonzero(np.isnan(m.cost_history(20)))) == [5]
    assert np.array_equal(run.grad_norm_history(20)[0], single.grad_norm_history(20)[0], equal_nan=True)


def test_absent_nan_rows_are_not_skipped(V):
    """The masked steps' never-read guarantee: NaN in an absent (row, modality) reaches neither the gradient nor the norm."""
    name, dtype = "A", "bf16"
    X, eps, B = data(name, 2)
    P = np.ones((2 * B, 2), np.uint8)
    P[3::4, 1] = 0
    bad = [X[0], X[1].copy()]
    bad[1][P[:, 1] == 0] = np.nan
    a, _ = make(V, name, dtype, clip=dict(skip_nonfinite=True))
    b, _ = make(V, name, dtype, clip=dict(skip_nonfinite=True))
    a.partial_fit_steps(bad, 2, eps, present=P)
    b.partial_fit_steps(X, 2, eps, present=P)
    norms, last, skipped = a.grad_norm_history(2)
    assert skipped == 0 and last == 2 and np.all(np.isfinite(norms))
    assert same_state(a, b) and np.array_equal(norms, b.grad_norm_history(2)[0])


# ----------------------------------------------------------------------------- 6. data parallel on one GPU
def test_host_owned_seam_clips_the_summed_gradient(V):
    from vae_assoc_amd import _capi
    name, dtype = "A", "bf16"
    archs, B = MODELS[name]
    X, eps, _ = data(name, 2)                              # a global batch of 2 * B rows
    reps = []
    for r in range(2):
        rep, _ = make(V, name, dtype)
        p0 = rep.get_params()
        rep._L.avae_destroy(rep._h)
        rep._cfg.row_offset, rep._cfg.batch_global = B * r, 2 * B
        h = C.c_void_p()
        _capi.check(None, rep._L.avae_create(C.byref(rep._cfg), C.byref(h)), "avae_create")
        rep._h = h
        rep.set_params(p0)
        if r == 0:
            before = opt_snapshot(rep)                     # (the step counter advances in the backward half)
        rep._backward(*rows(X, eps, B, r))
        reps.append(rep)
    torch.cuda.synchronize()
    gsum = reps[0]._grad_tensor() + reps[1]._grad_tensor()
    for rep in reps:
        rep._grad_tensor().copy_(gsum)
    torch.cuda.synchronize()
    g = reps[0].get_grads()
    assert np.array_equal(g, reps[1].get_grads())
    mx = 0.5 * float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    for rep in reps:
        rep.set_grad_clip(max_norm=mx)
        rep._apply()
    assert same_state(reps[0], reps[1])
    n = [rep.grad_norm_history(1) for rep in reps]
    assert n[0][0].tobytes() == n[1][0].tobytes() and n[0][1:] == n[1][1:] == (1, 0)
    c = factor(mx, n[0][0][0])
    assert c < 1.0
    check_adam_step(before, opt_snapshot(reps[0]), g.astype(F32) * c, LR)
    assert shadow_err(reps[0])[:2] == (0.0, 0.0) and shadow_err(reps[1])[:2] == (0.0, 0.0)


@pytest.mark.parametrize("comm", ["ipc", "library"])
@pytest.mark.parametrize("buckets", [1, 2])
def test_one_rank_pipeline_is_the_plain_clipped_step(V, comm, buckets):
    name, dtype = "A", "bf16"
    n0, _ = first_norm(V, name, dtype)
    clip = dict(max_norm=0.5 * n0)
    X, eps, B = data(name, 20)
    plain, _ = make(V, name, dtype, clip=clip)
    plain.partial_fit_steps(X, 20, eps)
    dp, _ = make(V, name, dtype, clip=clip, comm=comm, comm_buckets=buckets)
    assert dp._comm_lib and len(dp._buckets) == buckets
    dp.partial_fit_steps(X, 20, eps)
    assert same_state(plain, dp)
    assert np.array_equal(plain.cost_history(20), dp.cost_history(20))
    a, b = plain.grad_norm_history(20), dp.grad_norm_history(20)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] == (20, 0)
    assert np.sum(a[0] > F32(clip["max_norm"])) >= 3, "the run must hold clipped steps"


# ----------------------------------------------------------------------------- 7. errors
def test_errors(V):
    m, _ = make(V, "A", "bf16")
    L, h = m._L, m._h
    for bad in (-1.0, float("nan")):
        assert L.avae_set_grad_clip(h, C.c_float(bad), 0) != 0
        assert b"max_norm" in L.avae_last_error(h)
    out = np.zeros(8192, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.avae_grad_norm_history(h, 0, p, None, None) == 0            # fine on a handle that never clipped
    assert L.avae_grad_norm_history(h, 1, p, None, None) != 0
    m.set_grad_clip(max_norm=float("inf"))
    X, eps, B = data("A", 2)
    m.partial_fit_steps(X, 2, eps)
    assert L.avae_grad_norm_history(h, 4097, p, None, None) != 0          # above the history depth
    assert L.avae_grad_norm_history(h, 3, p, None, None) != 0             # above the steps since switch-on
    assert len(m.grad_norm_history(2)[0]) == 2 and len(m.grad_norm_history(0)[0]) == 0
    with pytest.raises(ValueError, match="max_norm"):
        m.set_grad_clip(max_norm=-3.0)
    with pytest.raises(RuntimeError):
        m.grad_norm_history(3)


def test_timing_report_names_the_norm_launch(V):
    """Timing mode (eager launches) goes through the same tail: clipping on = wgrad, grad_sumsq, adam; off = the fused launch."""
    m, _ = make(V, "A", "bf16")
    X, eps, B = data("A", 2)

    def launches():
        assert m._L.avae_timing_enable(m._h, 1) == 0
        m.partial_fit_steps(X, 2, eps)
        buf = C.create_string_buffer(1 << 16)
        assert m._L.avae_timing_report(m._h, buf, len(buf)) == 0 and m._L.avae_timing_enable(m._h, 0) == 0
        return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}

    off = launches()
    assert off.get("wgrad+adam") == 2 and "grad_sumsq" not in off and "adam" not in off
    m.set_grad_clip(max_norm=1.0)
    on = launches()
    assert on.get("grad_sumsq") == 2 and on.get("adam") == 2 and on.get("wgrad") == 2 and "wgrad+adam" not in on
