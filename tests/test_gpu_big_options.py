"""The training options -- presence masks, schedules, denoising, clipping, averaging -- on the plan the big nets run (MI355X):
the 8-wave 256x64 loss tiles (tile configuration 6) with their bf16 register epilogue, the latent item in a launch of its own,
k_adam over hundreds of tiles, k_grad_sumsq with more than 64 (and at its cap of 256) partial sums.  Each option's own test file
runs it on small nets that never reach these launches.

Shapes.  Net R (big_options_reference.NET_R): 784 (Bernoulli) / 147 (Gaussian), hidden [64, 48], n_z = 37, weights [5, 1],
assoc_lambda 0.5, softplus, batch 2817 = 11 x 256 + 1 -- the smallest batch at which the planner takes this plan (asserted through
the plan dump: 2817 is on it, 2561 is not), with one live row and 255 padding rows in the last loss tile.  C2 (784-500-500 /
147-200-200, n_z 20, B 100, relu, weights [50, 1], lambda 8): P_int 1531488, G = 187 norm partials, chain 8.  SET_A of
tests/test_gpu_big_ragged.py (B 3999, tanh): P_int 4252416, G = 256 (the cap), chain 17.

What the plan dump shows, and the tests assert: the latent item's own launch is planned like any launch of one non-GEMM item, on
the 4-wave 64x64 configuration (0) -- it runs latent_item<4, ...>, the instance the small nets' k_grouped routes run, fed by a
launch of its own (its HyperEntry and presence pointers are set per launch by the host).  The 8-wave instance of that item is
compiled for the 256x64 loss kernel but no training plan puts the latent item into that launch: whenever the planner picks
configuration 6 it also splits the latent item off.

Tolerances are the project's own (tests/test_gpu_masked.py, tests/test_gpu_parity.py): fp32 against the fp64 reference cost 1e-5
relative and gradients 1e-4 of each tensor's maximum, bf16 against the quant='bf16' reference 5e-5 and 3e-3; the KL multiplier in
bf16 against the unquantised torch restatement 1e-3 on the cost (tests/test_gpu_schedule.py); Adam by check_adam_step on the
device's own gradient and recorded norm; the average by tests/test_gpu_ema.py::check_ema_step (2^-23 max(|e|, |theta|)); the norm by
the derived bound of tests/test_gpu_clip.py::test_norm_accuracy_and_determinism at this G and chain; everything else bitwise.

Measured 2026-10-20, worst over the cases (cost / worst gradient tensor, beside the bounds above).  Masked steps, four variants:
fp32 1.4e-7 / 5.6e-6, bf16 1.3e-7 / 9.4e-5 (one_row and last_row_only in bf16: gradients equal to the last bit -- one row's outer
products of bf16 operands are exact).  KL multiplier 0, 0.5, 1: fp32 9.7e-8 / 2.5e-6, bf16 cost 5.6e-5, 2.7e-4, 3.8e-4 of 1e-3.
Explicit inputs: fp32 1.8e-8 / 2.5e-6, bf16 1.3e-7 / 9.8e-5; on-device corruption: fp32 4.1e-8 / 2.2e-6, bf16 1.8e-7 / 6.7e-5; under
the mask, fp32 1.3e-7 / 8.1e-6; staged normals off by 4.2e-7 of the allowed 1e-4 (2e-4 sigma).  A loss charged against the
encoder's rows would move the cost by 6.0e-2 - 7.7e-2 relative: 60 x the required margin of 100 x the fp32 tolerance.  Norm: C2
7.9e-9 (fp32), 4.4e-8 (bf16) of 9.24e-7; SET_A 2.0e-8 of 1.19e-6.  Every option at once: fp32 1.7e-9 / 4.6e-6, bf16 7.9e-8 / 1.7e-4;
the recorded norm within 3.5e-7 of the reference's.  Average: worst error 7.5e-9 (C2, SET_A) and 1.5e-8 (net R) at elements whose
bound is 1.5e-8 - 3.1e-8."""
import math

import numpy as np
import pytest
import torch

import plan_dump
import test_gpu_clip as TC
import test_gpu_denoise as TD
import test_gpu_ema as TE
import test_gpu_masked as TM
from big_options_reference import NET_R, composed_step, wrong_buffer_margin
from conftest import make_arch, shadow_err, synth_batch
from denoise_reference import corrupt
from oracle import vae_assoc_oracle as O
from plan_dump import K_FWD_HEAD, K_FWD_OUT_LOSS, K_LATENT
from schedule_reference import hyper, scheduled_cost_and_grads
from test_gpu_big_ragged import B_A, SET_A
from test_gpu_parity import build_pair, check_adam_step, opt_snapshot, per_tensor_err
from test_gpu_plan_switches import first_masked_step

pytestmark = pytest.mark.gpu

R = NET_R
ARCHS, BIN, W, LAM, B = R["archs"], R["binary"], R["weights"], R["lam"], R["B"]
ACT, LR, NZ, SEED = "softplus", 1e-3, 37, 11
F32 = np.float32
TOL = TD.TOL
DTYPES = ["fp32", "bf16"]
LOSS8, HEAD64x128, TILE64x64 = 6, 4, 0      # TileCfg::k256x64Loss, k64x128, k64x64 (tests/plan_dump.py)
EDGE_ROWS = [0, 63, 64, 2815, 2816]         # the staging tiles' first / last rows and the live row of the last loss tile


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_CACHE = {}


def rdata(steps):
    """the first `steps` of 4 batches of net R (computed once, shared, never written to) -> ([X0, X1], eps)"""
    if "R" not in _CACHE:
        rng = np.random.default_rng(101)
        _CACHE["R"] = (synth_batch(rng, 4 * B, [784, 147], BIN), rng.standard_normal((4 * B, NZ)).astype(np.float32))
    X, eps = _CACHE["R"]
    return [x[:steps * B] for x in X], eps[:steps * B]


def rows(X, eps, i, n=B):
    return [x[i * n:(i + 1) * n] for x in X], eps[i * n:(i + 1) * n]


def p0():
    if "p0" not in _CACHE:
        _CACHE["p0"] = TM._p0(R, 3)
    return _CACHE["p0"]


def model(V, dtype, lam=LAM, lr=LR, ema=None, **kw):
    m = V.AssocVariationalAutoEncoder(ARCHS, binary=BIN, transfer_fct=ACT, weights=W, assoc_lambda=lam, learning_rate=lr,
                                      batch_size=B, compute_dtype=dtype, seed=SEED, **kw)
    m.set_params(p0())
    if ema is not None:
        m.set_ema(**ema)                     # (after set_params: the average starts at the parameters of the moment)
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_state(a, b):
    sa, sb = opt_snapshot(a), opt_snapshot(b)
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(sa[:3], sb[:3])) and sa[3] == sb[3]


def random_mask(seed, steps=1):
    """tests/test_gpu_masked.py's random variant per batch; the live row of the last loss tile carries the image alone"""
    rng = np.random.default_rng(seed)
    P = np.concatenate([TM._masks(rng, B, 2)["random"] for _ in range(steps)])
    P[B - 1::B] = (True, False)
    return P


def check_cost_and_grads(tag, dtype, c, g, c_ref, g_ref, ctol, gtol):
    """cost within ctol (relative), every gradient tensor within gtol of its maximum (None: printed, not bounded)"""
    rel = abs(c - c_ref) / abs(c_ref)
    errs = per_tensor_err(ARCHS, np.asarray(g, np.float64), g_ref)
    worst = max(errs, key=lambda kv: kv[1])
    print("%s %s: cost %.7g reference %.7g rel %.2e (bound %.0e); worst gradient tensor %s %.2e (bound %s)" %
          ((tag, dtype, c, c_ref, rel, ctol) + worst + ("none" if gtol is None else "%.0e" % gtol,)))
    assert rel <= ctol, (tag, c, c_ref)
    bad = [(n, e) for n, e in errs if gtol is not None and e > gtol]
    assert not bad, (tag, bad)


# ----------------------------------------------------------------------------- 0. the plan
def _on_big_plan(plan):
    c, items = plan_dump.launch(plan, "fwd_out_loss")
    return c == LOSS8 and [(k, M, N) for k, M, N, _K in items] == [(K_FWD_OUT_LOSS, B, 784), (K_FWD_OUT_LOSS, B, 147)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_net_r_runs_the_big_plan(V, monkeypatch, capfd, dtype):
    """fwd_out_loss on the 8-wave 256x64 loss tiles, the latent item in a launch of its own, the heads on 64x128 tiles -- plain and
    masked -- and B = 2817 is the smallest batch = 1 mod 256 that gets there"""
    X, eps = rdata(1)
    kw = dict(binary=BIN, transfer_fct=ACT, weights=W, assoc_lambda=LAM, seed=SEED)
    plan = plan_dump.step_plan(V, monkeypatch, capfd, ARCHS, B, dtype, X, eps, **kw)
    assert _on_big_plan(plan), plan_dump.launch(plan, "fwd_out_loss")
    c, items = plan_dump.launch(plan, "latent")
    assert [(k, M) for k, M, _N, _K in items] == [(K_LATENT, B)], items
    assert c == TILE64x64, "the latent item's own launch runs on the 4-wave 64x64 configuration (see the module docstring)"
    c, items = plan_dump.launch(plan, "fwd_head")
    assert c == HEAD64x128 and [(k, M, N) for k, M, N, _K in items] == [(K_FWD_HEAD, B, 2 * NZ)] * 2, (c, items)
    assert "wgrad+adam" not in plan_dump.cfgs(plan), "net R's optimiser is k_adam"
    assert (B - 1) % 256 == 0 and -(-B // 256) * (13 + 3) == 192
    small = plan_dump.step_plan(V, monkeypatch, capfd, ARCHS, B - 256, dtype, [x[:B - 256] for x in X], eps[:B - 256], **kw)
    assert plan_dump.launch(small, "fwd_out_loss")[0] != LOSS8 and "latent" not in plan_dump.cfgs(small)
    # the masked twin of the step
    m = plan_dump.with_switches(monkeypatch, {"AVAE_DEBUG_SYNC": "1"},
                                lambda: V.AssocVariationalAutoEncoder(ARCHS, batch_size=B, compute_dtype=dtype, **kw))
    _, _, masked = first_masked_step(m, capfd, (X, eps, random_mask(1)))
    assert _on_big_plan(masked), plan_dump.launch(masked, "fwd_out_loss")
    c, items = plan_dump.launch(masked, "latent")
    assert c == TILE64x64 and [(k, M) for k, M, _N, _K in items] == [(K_LATENT, B)], (c, items)


# ----------------------------------------------------------------------------- 1. random masks
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_step_against_reference(V, dtype):
    """cost, every gradient tensor of a live modality, exact zeros and untouched parameters for an absent one; last_row_only: the
    single live row of the last 256-row tile is the only row present"""
    last = np.zeros((B, 2), bool)
    last[B - 1] = True
    TM.check_against_reference(V, R, dtype, ACT, variants=("random", "absent_col", "one_row", "last_row_only"),
                               extra={"last_row_only": last})


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_present_mask_is_the_unmasked_step(V, dtype):
    TM.check_all_present_bitwise(V, R, dtype, ACT, steps=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_content_and_source_padding_are_never_read(V, dtype):
    """NaN in every absent entry of X and of inputs=, and in the columns of the caller's matrix that lie between and behind the
    modalities' column views (the padding of the rows the staging launch reads), changes no output bit."""
    X, eps = rdata(2)
    P = random_mask(7, 2)
    a, b = slice(0, B), slice(B, 2 * B)
    runs = []
    for fill in (0.0, np.nan):
        wide = np.full((2 * B, 784 + 3 + 147 + 5), fill, np.float32)
        wide[:, :784], wide[:, 787:934] = X[0], X[1]
        wide[:, :784][~P[:, 0]] = fill
        wide[:, 787:934][~P[:, 1]] = fill
        t = torch.as_tensor(wide).cuda()
        Xs = lambda r: [t[r, :784], t[r, 787:934]]
        m = model(V, dtype)
        costs = [m.partial_fit(Xs(a), eps[a], present=P[a]), m.partial_fit_steps(Xs(b), 1, eps[b], present=P[b]),
                 m.partial_fit(Xs(a), eps[a], present=P[a], inputs=Xs(a)), m.evaluate_cost(Xs(b), eps[b], present=P[b])]
        runs.append((costs, TM._state(m)))
        assert shadow_err(m)[:2] == (0.0, 0.0)
        del m
    assert np.all(np.isfinite(runs[0][0])) and bits(runs[0][0]).tolist() == bits(runs[1][0]).tolist(), (runs[0][0], runs[1][0])
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y)


# ----------------------------------------------------------------------------- 2. schedules
BETA = dict(knots=[(0, 0), (1, 0.5), (2, 1)])
TWIN = dict(assoc=dict(knots=[(0, 0.25), (4, 1.5)]), lr=dict(decay_rate=0.7, decay_steps=3, staircase=False))
KNOTS = dict(kl=dict(knots=[(0, 0.2), (1, 1.0), (4, 0.4)]), assoc=dict(knots=[(0, 0), (1, 1), (2, 0.5)]),
             lr=dict(knots=[(0, 1), (1, 0.5), (3, 1)]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kl_multiplier_against_fp64(V, dtype):
    """steps 1-3 (kl_t = 0, 0.5, 1) at the handle's own weights of each step against the torch fp64 restatement: fp32 cost 1e-5 and
    gradients 1e-4; bf16 the cost within 1e-3 (the restatement does not quantise), as tests/test_gpu_schedule.py"""
    X, eps = rdata(3)
    m = model(V, dtype, schedule=dict(kl=BETA))
    for s, kl in enumerate((0.0, 0.5, 1.0)):
        x, e = rows(X, eps, s)
        th = m.get_params().astype(np.float64)
        cost = m.partial_fit(x, e)
        h = m.hyper_history(1)[0][0]
        assert h[0] == F32(kl) and h[1] == F32(LAM) and h[2] == F32(LR)
        c_ref, g_ref = scheduled_cost_and_grads(ARCHS, th, x, e, BIN, W, LAM, ACT, kl=kl)
        ctol, gtol = (1e-5, 1e-4) if dtype == "fp32" else (1e-3, None)
        check_cost_and_grads("kl %.1f" % kl, dtype, cost, m.get_grads(), c_ref, g_ref, ctol, gtol)
        assert shadow_err(m)[:2] == (0.0, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scheduled_lambda_and_lr_equal_configured_ones_bitwise(V, dtype):
    """step t of a scheduled handle = an unscheduled handle built with assoc_lambda = lambda_t and learning_rate = lr_eff_t (the
    device's own history) on the same theta, m, v and counter"""
    X, eps = rdata(2)
    sch = model(V, dtype, schedule=TWIN)
    for t in (1, 2):
        before = opt_snapshot(sch)
        x, e = rows(X, eps, t - 1)
        c_s = sch.partial_fit(x, e)
        g_s, after = sch.get_grads(), opt_snapshot(sch)
        (kl_t, lam_t, lr_t), last = sch.hyper_history(1)[0][0], sch.hyper_history(1)[1]
        assert last == t and kl_t == 1
        wl = hyper(None, TWIN["assoc"], None, LAM, LR, t)[1]
        assert lam_t.tobytes() == wl.tobytes() and lam_t != F32(LAM) and (t == 1 or lr_t != F32(LR))
        plain = model(V, dtype, lam=float(lam_t), lr=float(lr_t))
        plain.set_params(before[0])
        plain.set_opt_state(before[1], before[2], before[3])
        c_p = plain.partial_fit(x, e)
        assert F32(c_s).tobytes() == F32(c_p).tobytes(), (t, c_s, c_p)
        assert np.array_equal(g_s, plain.get_grads()), "gradient, step %d" % t
        assert same_state(sch, plain), "theta / m / v / counter, step %d" % t
        assert shadow_err(sch)[:2] == (0.0, 0.0) and shadow_err(plain)[:2] == (0.0, 0.0)
        check_adam_step(before, after, g_s, float(lr_t))
        del plain


@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_multipliers_are_the_plain_step_bitwise(V, dtype):
    X, eps = rdata(2)
    flat = dict(knots=[(0, 1), (10, 1), (20, 0)])

    def run(m):
        out = []
        for s in range(2):
            out.append((m.partial_fit(*rows(X, eps, s)), m.get_grads()))
        return out

    plain = model(V, dtype)
    want = run(plain)
    for what, spec in (("constant 1", dict(kl=1.0, assoc=1.0, lr=1.0)), ("piecewise, 1 at the tested steps", dict(kl=flat, assoc=flat, lr=flat))):
        m = model(V, dtype, schedule=spec)
        for s, ((c0, g0), (c1, g1)) in enumerate(zip(want, run(m))):
            assert c0 == c1 and np.array_equal(g0, g1), "%s: step %d" % (what, s)
        assert same_state(plain, m) and shadow_err(m)[:2] == (0.0, 0.0), what
        assert np.array_equal(m.hyper_history(2)[0], np.tile(np.array([1.0, LAM, LR], F32), (2, 1)))
        del m


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_step_replay_across_a_knot_is_three_single_steps(V, dtype):
    X, eps = rdata(3)
    run, single = model(V, dtype, schedule=KNOTS), model(V, dtype, schedule=KNOTS)
    run.partial_fit_steps(X, 3, eps)
    costs = [single.partial_fit(*rows(X, eps, s)) for s in range(3)]
    assert same_state(run, single) and opt_snapshot(run)[3] == 3
    assert np.array_equal(run.cost_history(3), np.asarray(costs, F32))
    ha, hb = run.hyper_history(3), single.hyper_history(3)
    assert ha[0].tobytes() == hb[0].tobytes() and ha[1] == hb[1] == 3
    for t in (1, 2, 3):                                      # every column changes at every step: the knots at u = 1 are crossed
        want = hyper(KNOTS["kl"], KNOTS["assoc"], KNOTS["lr"], LAM, LR, t)
        assert all(ha[0][t - 1, k].tobytes() == want[k].tobytes() for k in range(3)), (t, ha[0][t - 1], want)
    assert all(len(set(ha[0][:, k].tolist())) == 3 for k in range(3))
    assert shadow_err(run)[:2] == (0.0, 0.0)


# ----------------------------------------------------------------------------- 3. denoising
CORR = dict(drop=[0.5, 0.1], noise=[0.0, 0.5], drop_value=[0.0, -1.0])


def explicit_inputs(X):
    """half of the image dropped, sigma 0.5 on the joint, drawn on the host with the reference's stream under another seed"""
    return [corrupt(X[0], 99, 21, 0, drop=0.5)[0].astype(np.float32), corrupt(X[1], 99, 21, 1, noise=0.5)[0].astype(np.float32)]


def check_margin(p, X, xin, eps, dtype, present=None):
    """a loss item that read the encoder's rows would miss the cost bound by more than two orders of magnitude"""
    for k in range(2):
        rows_ = slice(None) if present is None else present[:, k]
        assert np.mean(np.asarray(xin[k])[rows_] != X[k][rows_]) >= 0.1, k
    true, wrong = wrong_buffer_margin(ARCHS, p, X, xin, eps, BIN, W, LAM, ACT, present=present)
    print("cost charged against the clean rows %.7g, against the corrupted rows %.7g: %.1e relative" % (true, wrong, abs(wrong - true) / abs(true)))
    assert abs(wrong - true) > 100 * TOL[dtype][0] * abs(true), (true, wrong)


@pytest.mark.parametrize("dtype", DTYPES)
def test_explicit_inputs_against_reference(V, dtype):
    X, eps = rdata(1)
    xin = explicit_inputs(X)
    m = model(V, dtype)
    p = m.get_params()
    c = m.partial_fit(X, eps, inputs=xin)
    TD.check_step(m, R, dtype, ACT, p, c, X, xin, eps, tag="explicit inputs")
    check_margin(p, X, xin, eps, dtype)


def test_on_device_corruption_is_the_documented_stream(V):
    """Steps 0 and 1: the targets are the clean rows, the encoders' rows the documented draw -- every row and column, so the rows
    around the 64-row staging tiles' edges, the last two rows (2816: the live row of the last loss tile) and the last column quad
    of either width (147 = 36 x 4 + 3: a partial quad) among them; then each step against the reference fed the staged rows."""
    X, eps = rdata(2)
    f32, b16 = model(V, "fp32", corruption=CORR), model(V, "bf16", corruption=CORR)
    for s in range(2):
        x, e = rows(X, eps, s)
        p32, p16 = f32.get_params(), b16.get_params()
        c32, c16 = f32.partial_fit(x, e), b16.partial_fit(x, e)
        xs, ts = TD.staged(f32, B)
        x16, t16 = TD.staged(b16, B)
        for k, w in enumerate((784, 147)):
            assert np.array_equal(ts[k], x[k]) and np.array_equal(t16[k], x[k]), "T%d is the exact target" % k
            want, dropped = corrupt(x[k], SEED, s, k, CORR["drop"][k], CORR["noise"][k], CORR["drop_value"][k])
            edge = np.zeros(dropped.shape, bool)
            edge[EDGE_ROWS] = True
            edge[:, w - (w % 4 or 4):] = True
            assert dropped[edge].any() and not dropped[edge].all()
            for sel, what in ((edge, "edge rows and the last quad"), (np.ones_like(edge), "all")):
                d = dropped & sel
                assert np.all(xs[k][d] == F32(CORR["drop_value"][k])), (what, "dropped elements are exactly drop_value")
                err = np.abs(xs[k][~dropped & sel] - want[~dropped & sel]).max()
                print("step %d modality %d, %s: kept elements off by %.2e (sigma %.1f)" % (s, k, what, err, CORR["noise"][k]))
                assert err <= 2e-4 * CORR["noise"][k], what
            assert np.array_equal(x16[k], O.bf16_round(xs[k]).astype(np.float32)), "the bf16 copy is the fp32 x~ rounded once"
        TD.check_step(f32, R, "fp32", ACT, p32, c32, x, xs, e, tag="corrupted step %d" % s)
        TD.check_step(b16, R, "bf16", ACT, p16, c16, x, x16, e, tag="corrupted step %d" % s)
        if s == 0:
            check_margin(p32, x, xs, e, "bf16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_corrupted_steps_equal_a_twin_fed_the_staged_inputs(V, dtype):
    X, eps = rdata(2)
    a, b = model(V, dtype, corruption=CORR), model(V, dtype)
    for s in range(2):
        x, e = rows(X, eps, s)
        ca = a.partial_fit(x, e)
        cb = b.partial_fit(x, e, inputs=TD.staged(a, B)[0])
        assert ca == cb, (s, ca, cb)
    TD._same_state(a, b)


def test_masked_denoising_step(V):
    """fp32 (where the clean target and the encoder's copy are two buffers of one type): on-device corruption under a random mask"""
    X, eps = rdata(1)
    P = random_mask(5)
    m = model(V, "fp32", corruption=CORR)
    p = m.get_params()
    c = m.partial_fit(X, eps, present=P)
    xs, ts = TD.staged(m, B)
    for k in range(2):
        want, dropped = corrupt(X[k], SEED, 0, k, CORR["drop"][k], CORR["noise"][k], CORR["drop_value"][k])
        on = P[:, k]
        assert not xs[k][~on].any() and not ts[k][~on].any() and np.array_equal(ts[k][on], X[k][on])
        assert np.all(xs[k][on][dropped[on]] == F32(CORR["drop_value"][k]))
        assert np.abs(xs[k][on] - want[on])[~dropped[on]].max() <= 2e-4 * CORR["noise"][k]
    TD.check_step(m, R, "fp32", ACT, p, c, X, xs, eps, present=P, tag="masked corrupted")
    check_margin(p, X, xs, eps, "fp32", present=P)


# ----------------------------------------------------------------------------- 4. clipping and averaging at G > 64
C2 = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
NETS4 = {"C2": dict(archs=C2, B=100, act="relu", w=[50, 1], lam=8.0),
         "SET_A": dict(archs=SET_A, B=B_A, act="tanh", w=[5.0, 1.0], lam=0.5)}
CASES4 = [("C2", "fp32"), ("C2", "bf16"), ("SET_A", "bf16")]
EMA = dict(decay=0.9, warmup=True)                        # d_t = 2/11, 3/12, 4/13 at steps 1..3: every step has its own factor


def make4(V, name, dtype, **kw):
    n = NETS4[name]
    return build_pair(V, n["archs"], BIN, n["w"], n["lam"], n["act"], n["B"], dtype, lr=LR, **kw)[0]


def data4(name, steps):
    """the first `steps` of 3 batches (computed once per net, shared, never written to)"""
    n = NETS4[name]
    if name not in _CACHE:
        rng = np.random.default_rng(31)
        _CACHE[name] = (synth_batch(rng, 3 * n["B"], [784, 147], BIN), rng.standard_normal((3 * n["B"], n["archs"][0]["n_z"])).astype(np.float32))
    X, eps = _CACHE[name]
    return [x[:steps * n["B"]] for x in X], eps[:steps * n["B"]], n["B"]


def handle(V, name, dtype, clip=None, ema=None):
    """C2: a fresh handle.  SET_A (4.6 M parameters): the module's one handle, put back to its initial parameters, zero moments,
    step 0 and no option, then given `clip` / `ema`."""
    if name != "SET_A":
        m = make4(V, name, dtype)
    else:
        if "seta" not in _CACHE:
            m = make4(V, name, dtype)
            _CACHE["seta"] = dict(m=m, p0=m.get_params(), ema=False)
        c = _CACHE["seta"]
        m = c["m"]
        if c["ema"]:
            m.set_ema(None)
        m.set_grad_clip(0.0, False)
        m.set_params(c["p0"])
        z = np.zeros(m.n_params, np.float32)
        m.set_opt_state(z, z, 0)
        c["ema"] = ema is not None
    if clip is not None:
        m.set_grad_clip(**clip)
    if ema is not None:
        m.set_ema(**ema)
    return m


def first_norm(V, name, dtype):
    """(norm, raw gradient) of the first step on data4(name, ...), measured once on a monitoring handle"""
    if ("n0", name, dtype) not in _CACHE:
        m = handle(V, name, dtype, clip=dict(max_norm=float("inf")))
        X, eps, _ = data4(name, 1)
        m.partial_fit(X, eps)
        _CACHE[("n0", name, dtype)] = (float(m.grad_norm_history(1)[0][0]), m.get_grads())
    return _CACHE[("n0", name, dtype)]


@pytest.mark.parametrize("name,dtype", CASES4)
def test_norm_over_more_than_64_partials(V, name, dtype):
    """k_adam's wave 0 sums the partials four per lane: lanes' second to fourth terms are live from G = 65 (C2) and all 256 slots at
    the cap (SET_A, where every thread of k_grad_sumsq also chains more than 8 quads).  The bound is the derived one of
    tests/test_gpu_clip.py::test_norm_accuracy_and_determinism at this G and chain."""
    X, eps, _ = data4(name, 1)
    norms = []
    for fresh in (False, True):
        m = make4(V, name, dtype) if fresh else handle(V, name, dtype)
        m.set_grad_clip(max_norm=float("inf"))
        m.partial_fit(X, eps)
        h, last, skipped = m.grad_norm_history(1)
        assert last == 1 and skipped == 0 and h.dtype == np.float32
        norms.append(h[0])
    assert norms[0].tobytes() == norms[1].tobytes(), "the norm differs between two handles on the same inputs"
    p_int = m._grad_tensor().numel() - 1
    G, chain = TC.sumsq_shape(p_int)
    if name == "C2":
        assert 64 < G < TC.SUMSQ_MAX_BLOCKS, (p_int, G)
    else:
        assert G == TC.SUMSQ_MAX_BLOCKS and chain > TC.SUMSQ_QUADS, (p_int, G, chain)
    bound_s = (chain + 2 + math.ceil(math.log2(TC.SUMSQ_THREADS * G)) + 3) * 2.0 ** -24
    want = float(np.sqrt(np.sum(m.get_grads().astype(np.float64) ** 2)))
    rel = abs(float(norms[0]) - want) / want
    print("%s %s: P_int %d G %d chain %d norm %.9g fp64 %.9g rel %.3e bound %.3e" % (name, dtype, p_int, G, chain, norms[0], want, rel,
                                                                                    0.5 * bound_s + 2.0 ** -24))
    assert want > 0 and rel <= 0.5 * bound_s + 2.0 ** -24


def _two_steps(m, X, eps, B_):
    return [(m.partial_fit(*rows(X, eps, s, B_)), m.get_grads()) for s in range(2)]


@pytest.mark.parametrize("name,dtype", CASES4)
def test_monitor_only_is_bitwise_the_plain_step(V, monkeypatch, capfd, name, dtype):
    """max_norm = inf: c == 1 on every step, so the clip-aware k_adam must give the plain k_adam's bits.  C2's default plan applies
    Adam in the weight-gradient epilogue; its plain twin is planned with AVAE_NO_ADAM_FUSE=1 so that both sides run k_adam."""
    X, eps, B_ = data4(name, 2)
    if name == "C2":
        n = NETS4[name]
        kw = dict(binary=BIN, transfer_fct=n["act"], weights=n["w"], assoc_lambda=n["lam"], seed=5)
        dump = lambda **more: plan_dump.cfgs(plan_dump.step_plan(V, monkeypatch, capfd, n["archs"], B_, dtype, *rows(X, eps, 0, B_), **kw, **more))
        clipped, unfused = dump(grad_clip=dict(max_norm=float("inf"))), dump(env={"AVAE_NO_ADAM_FUSE": "1"})
        assert "wgrad+adam" not in clipped and 12 not in clipped.values(), clipped
        assert "wgrad+adam" not in unfused and 12 not in unfused.values(), unfused
        if dtype == "bf16":
            assert dump().get("wgrad+adam") == 12, "the default plan of C2 is the fused launch"
        plain = plan_dump.with_switches(monkeypatch, {"AVAE_NO_ADAM_FUSE": "1"}, lambda: make4(V, name, dtype))
    else:
        plain = handle(V, name, dtype)
    want = _two_steps(plain, X, eps, B_)
    st = opt_snapshot(plain)
    mon = handle(V, name, dtype, clip=dict(max_norm=float("inf")))
    got = _two_steps(mon, X, eps, B_)
    for s, ((c0, g0), (c1, g1)) in enumerate(zip(want, got)):
        assert c0 == c1 and np.array_equal(g0, g1), "step %d" % s
    now = opt_snapshot(mon)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(st[:3], now[:3])) and st[3] == now[3] == 2
    norms = mon.grad_norm_history(2)[0]
    assert np.all(np.isfinite(norms)) and np.all(norms > 0)
    assert shadow_err(mon)[:2] == (0.0, 0.0)


@pytest.mark.parametrize("name,dtype", CASES4)
def test_active_clipping(V, name, dtype):
    """max_norm = half the first norm: Adam consumed f32(g) * f32(c), c from the device's recorded norm; the buffer keeps g"""
    n0, g_twin = first_norm(V, name, dtype)
    mx = 0.5 * n0
    X, eps, B_ = data4(name, 1)
    m = handle(V, name, dtype, clip=dict(max_norm=mx))
    TC.clipped_steps(m, X, eps, B_, mx, 1, g_first=g_twin)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_step_is_skipped_and_keeps_the_average(V, dtype):
    name = "C2"
    X, eps, B_ = data4(name, 3)
    bad = [X[0], X[1].copy()]
    bad[1][B_ + 3, 7] = np.inf                               # one inf in the joint modality of batch 1
    m = handle(V, name, dtype, clip=dict(max_norm=0.5 * first_norm(V, name, dtype)[0], skip_nonfinite=True), ema=EMA)
    m.partial_fit(*rows(X, eps, 0, B_))
    before, e_before, raw_before = opt_snapshot(m), m.get_ema_params(), TE.master(m)
    c = m.partial_fit(*rows(bad, eps, 1, B_))
    after = opt_snapshot(m)
    assert not np.isfinite(c) and after[3] == before[3] + 1 == 2
    norms, last, skipped = m.grad_norm_history(2)
    assert last == 2 and skipped == 1 and np.isfinite(norms[0]) and not np.isfinite(norms[1])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[:3], after[:3])), "a skipped step wrote parameters or moments"
    assert np.array_equal(bits(TE.master(m)), bits(raw_before)), "a skipped step wrote the average"
    assert shadow_err(m)[:2] == (0.0, 0.0)
    m.partial_fit(*rows(X, eps, 2, B_))
    assert m.get_opt_state()[2] == 3 and m.grad_norm_history(1)[2] == 1
    TE.check_ema_step(e_before, m.get_params(), m.get_ema_params(), EMA["decay"], True, 3)      # the skipped step consumed number 2


@pytest.mark.parametrize("name,dtype", CASES4)
def test_average_under_clipping(V, name, dtype):
    """k_adam<.., CLIP, EMA>: three clipped steps, the average after each against ema_reference on the handle's own parameters; and
    theta, m, v and the costs bit for bit those of a twin without averaging under the same clip"""
    mx = 0.5 * first_norm(V, name, dtype)[0]
    X, eps, B_ = data4(name, 3)
    on = handle(V, name, dtype, clip=dict(max_norm=mx), ema=EMA)
    assert TE.same(on.get_ema_params(), on.get_params())
    for s in range(3):
        e_prev = on.get_ema_params()
        on.partial_fit(*rows(X, eps, s, B_))
        TE.check_ema_step(e_prev, on.get_params(), on.get_ema_params(), EMA["decay"], True, s + 1)
    st, costs, norms = opt_snapshot(on), on.cost_history(3), on.grad_norm_history(3)[0]
    assert norms[0] > F32(mx), "the run must hold a clipped step"
    assert shadow_err(on)[:2] == (0.0, 0.0)
    off = handle(V, name, dtype, clip=dict(max_norm=mx))
    for s in range(3):
        off.partial_fit(*rows(X, eps, s, B_))
    now = opt_snapshot(off)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(st[:3], now[:3])) and st[3] == now[3] == 3
    assert np.array_equal(costs, off.cost_history(3)) and np.array_equal(norms, off.grad_norm_history(3)[0])


# ----------------------------------------------------------------------------- 5. k_adam's row-tile edges under clip + EMA
def first_norm_r(V, dtype):
    """the norm of net R's first plain step, measured once on a monitoring handle"""
    if ("n0R", dtype) not in _CACHE:
        m = model(V, dtype, grad_clip=dict(max_norm=float("inf")))
        m.partial_fit(*rdata(1))
        _CACHE[("n0R", dtype)] = float(m.grad_norm_history(1)[0][0])
    return _CACHE[("n0R", dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_adam_row_tile_edges_under_clip_and_ema(V, dtype):
    """Net R's layers have 785, 148, 65, 49 and 38 rows (fan-in + the bias row): none a multiple of k_adam's 16-row tile."""
    fan = {int(shp[0]) + 1 for na in ARCHS for _, shp in O.layer_shapes(na) if len(shp) == 2}
    assert fan == {785, 148, 65, 49, 38} and all(r % 16 for r in fan)
    mx = 0.5 * first_norm_r(V, dtype)
    X, eps = rdata(3)
    m = model(V, dtype, grad_clip=dict(max_norm=mx), ema=EMA)
    for s in range(3):
        before, e_prev = opt_snapshot(m), m.get_ema_params()
        m.partial_fit(*rows(X, eps, s))
        g, norm = m.get_grads(), m.grad_norm_history(1)[0][0]
        c = TC.factor(mx, norm)
        assert s > 0 or c < 1.0, (norm, mx)
        after = opt_snapshot(m)
        check_adam_step(before, after, g.astype(F32) * c, LR)
        TE.check_ema_step(e_prev, after[0], m.get_ema_params(), EMA["decay"], True, s + 1)
        assert shadow_err(m)[:2] == (0.0, 0.0)
    avg = m.get_ema_params()
    x70 = [x[:70] for x in X]
    live = m.transform(x70)
    with m.averaged():
        got = m.transform(x70)
    fresh = model(V, dtype)
    fresh.set_params(avg)
    want = fresh.transform(x70)
    assert all(TE.same(a, b) for a, b in zip(got, want))
    assert any(not TE.same(a, b) for a, b in zip(got, live)), "the averaged encoders must differ from the live ones"
    assert shadow_err(m)[:2] == (0.0, 0.0)


# ----------------------------------------------------------------------------- 6. everything at once
CORR6 = dict(drop=[0.5, 0.2], noise=0.0, drop_value=[0.0, 3.0])          # drops alone: the reference's draw is the device's, exactly
SCHED6 = dict(assoc=dict(knots=[(0, 0.25), (2, 1.5), (6, 1.0)]), lr=dict(knots=[(0, 1.0), (2, 0.5), (5, 1.0)]))


def handle6(V, dtype, max_norm):
    return model(V, dtype, corruption=CORR6, schedule=SCHED6, grad_clip=dict(max_norm=max_norm), ema=EMA)


def first_norm6(V, dtype, X, eps, P):
    if ("n06", dtype) not in _CACHE:
        m = handle6(V, dtype, float("inf"))
        m.partial_fit(X, eps, present=P)
        _CACHE[("n06", dtype)] = float(m.grad_norm_history(1)[0][0])
    return _CACHE[("n06", dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_option_at_once_against_the_composed_reference(V, dtype):
    """mask + on-device corruption + assoc and lr schedules + clip at half the first norm + averaging with warm-up on one handle:
    step 1 against big_options_reference.composed_step"""
    X, eps = rdata(1)
    P = random_mask(9)
    mx = 0.5 * first_norm6(V, dtype, X, eps, P)
    m = handle6(V, dtype, mx)
    before, e_prev = opt_snapshot(m), m.get_ema_params()
    c = m.partial_fit(X, eps, present=P)
    g, norm, after, e = m.get_grads(), m.grad_norm_history(1)[0][0], opt_snapshot(m), m.get_ema_params()
    (kl_t, lam_t, lr_t), last = m.hyper_history(1)[0][0], m.hyper_history(1)[1]
    z = np.zeros(before[0].size)
    r = composed_step(ARCHS, before[0], z, z, 0, X, eps, BIN, W, LAM, ACT, LR, present=P, corruption=dict(seed=SEED, **CORR6),
                      assoc=SCHED6["assoc"], lr_schedule=SCHED6["lr"], max_norm=mx, ema=dict(e=e_prev, **EMA),
                      quant=None if dtype == "fp32" else "bf16")
    assert last == 1 and kl_t == 1 and lam_t.tobytes() == F32(r["lambda_t"]).tobytes() and lr_t.tobytes() == F32(r["lr_t"]).tobytes()
    assert lam_t != F32(LAM)
    xs, ts = TD.staged(m, B)
    for k in range(2):                                       # the staged rows are the reference's draw, and differ from the clean ones
        on = P[:, k]
        want = r["X_in"][k].astype(np.float32)
        assert np.array_equal(xs[k][on], want[on] if dtype == "fp32" else O.bf16_round(want[on]).astype(np.float32))
        assert np.array_equal(ts[k][on], X[k][on]) and np.mean(want[on] != X[k][on]) >= 0.1
    check_cost_and_grads("all options", dtype, c, g, r["cost"], r["g"], *TOL[dtype])
    cd = TC.factor(mx, norm)
    print("norm %.7g (reference %.7g, rel %.1e), c %.6f (reference %.6f)" % (norm, r["norm"], abs(norm - r["norm"]) / r["norm"], cd, r["c"]))
    assert cd < 1.0 and r["c"] < 1.0
    check_adam_step(before, after, g.astype(F32) * cd, float(lr_t))
    TE.check_ema_step(e_prev, after[0], e, EMA["decay"], True, 1)
    assert shadow_err(m)[:2] == (0.0, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_option_at_once_replay_is_single_steps(V, dtype):
    """four batches through one partial_fit_steps(.., 4, present=) = four single masked steps, bitwise"""
    X, eps = rdata(4)
    P = random_mask(9, 4)
    mx = 0.5 * first_norm6(V, dtype, *rows(X, eps, 0), P[:B])
    run, single = handle6(V, dtype, mx), handle6(V, dtype, mx)
    run.partial_fit_steps(X, 4, eps, present=P)
    costs = [single.partial_fit(*rows(X, eps, s), present=P[s * B:(s + 1) * B]) for s in range(4)]
    assert same_state(run, single) and opt_snapshot(run)[3] == 4
    assert TE.same(run.get_ema_params(), single.get_ema_params()) and not TE.same(run.get_ema_params(), run.get_params())
    assert np.array_equal(run.cost_history(4), np.asarray(costs, F32))
    na, nb = run.grad_norm_history(4), single.grad_norm_history(4)
    assert na[0].tobytes() == nb[0].tobytes() and na[1:] == nb[1:] == (4, 0) and na[0][0] > F32(mx)
    ha, hb = run.hyper_history(4), single.hyper_history(4)
    assert ha[0].tobytes() == hb[0].tobytes() and ha[1] == hb[1] == 4
    assert len(set(ha[0][:, 1].tolist())) == 4, "lambda_t changes at every step"
    assert shadow_err(run)[:2] == (0.0, 0.0) and shadow_err(single)[:2] == (0.0, 0.0)
