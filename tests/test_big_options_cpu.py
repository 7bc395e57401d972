"""CPU checks of the composed reference of tests/big_options_reference.py (the step with masks, corruption, schedules, clipping
and averaging set at once, which tests/test_gpu_big_options.py holds the big nets' plan to): with options off it must BE the
reference each option already has -- the oracle's step, the masked step, the clipped step -- and a loss charged against the
encoder's corrupted rows must move net R's cost by far more than the GPU tests' cost tolerance."""
import numpy as np
import pytest

from big_options_reference import NET_R, composed_step, corrupted_inputs, wrong_buffer_margin
from clip_reference import clipped_step
from conftest import synth_batch
from ema_reference import ema_step
from masked_reference import masked_cost_and_grads
from oracle import vae_assoc_oracle as O
from schedule_reference import hyper

ARCHS, BIN, W, LAM = NET_R["archs"], NET_R["binary"], NET_R["weights"], NET_R["lam"]
ACT, LR, B, NZ = "softplus", 1e-3, 64, 37


@pytest.fixture(scope="module")
def setup():
    """a 64-row slice of net R: parameters, one batch, eps, a mask with an empty row, a full row and both single-modality rows"""
    rng = np.random.default_rng(5)
    p0 = O.flatten_params(ARCHS, O.init_params(ARCHS, rng))
    X = synth_batch(rng, B, [784, 147], BIN)
    eps = rng.standard_normal((B, NZ))
    P = rng.random((B, 2)) < 0.6
    P[0], P[1], P[2], P[3] = False, True, (True, False), (False, True)
    return p0, X, eps, P


def _zeros():
    return np.zeros(O.param_count(ARCHS))


def test_every_option_off_is_the_oracle_step(setup):
    p0, X, eps, _ = setup
    ref = O.OracleAssocVAE(ARCHS, BIN, ACT, W, LAM, LR, B, params_flat=p0.copy())
    cost, g, _ = ref.cost_and_grads(X, eps)
    th, m, v = O.adam_step(p0, _zeros(), _zeros(), g, 1, LR)
    r = composed_step(ARCHS, p0, _zeros(), _zeros(), 0, X, eps, BIN, W, LAM, ACT, LR)
    assert r["cost"] == cost and r["c"] == 1.0 and r["t"] == 1 and r["ema"] is None
    assert r["lambda_t"] == LAM and r["lr_t"] == LR
    for a, b in ((r["g"], g), (r["theta"], th), (r["m"], m), (r["v"], v)):
        assert np.array_equal(a, b)
    # ... and a second step from there is the oracle's second step
    ref.apply_gradients(g)
    cost2, g2, _ = ref.cost_and_grads(X, eps)
    ref.apply_gradients(g2)
    r2 = composed_step(ARCHS, r["theta"], r["m"], r["v"], r["t"], X, eps, BIN, W, LAM, ACT, LR)
    assert r2["cost"] == cost2 and np.array_equal(r2["theta"], ref.get_params()) and r2["t"] == ref.t == 2


def test_mask_only_is_the_masked_reference(setup):
    p0, X, eps, P = setup
    cost, g = masked_cost_and_grads(ARCHS, p0, X, eps, P, BIN, W, LAM, ACT)
    r = composed_step(ARCHS, p0, _zeros(), _zeros(), 0, X, eps, BIN, W, LAM, ACT, LR, present=P)
    assert r["cost"] == cost and np.array_equal(r["g"], g) and r["c"] == 1.0
    th, _, _ = O.adam_step(p0, _zeros(), _zeros(), g, 1, LR)
    assert np.array_equal(r["theta"], th)
    # the quantised reference is handed through alike
    cost, g = masked_cost_and_grads(ARCHS, p0, X, eps, P, BIN, W, LAM, ACT, quant="bf16")
    r = composed_step(ARCHS, p0, _zeros(), _zeros(), 0, X, eps, BIN, W, LAM, ACT, LR, present=P, quant="bf16")
    assert r["cost"] == cost and np.array_equal(r["g"], g)


def test_clip_only_is_the_clipped_step(setup):
    p0, X, eps, _ = setup
    probe = clipped_step(O.OracleAssocVAE(ARCHS, BIN, ACT, W, LAM, LR, B, params_flat=p0.copy()), X, eps)
    for mx in (0.5 * probe["norm"], 4.0 * probe["norm"], float("inf")):
        ref = O.OracleAssocVAE(ARCHS, BIN, ACT, W, LAM, LR, B, params_flat=p0.copy())
        want = clipped_step(ref, X, eps, max_norm=mx)
        r = composed_step(ARCHS, p0, _zeros(), _zeros(), 0, X, eps, BIN, W, LAM, ACT, LR, max_norm=mx)
        assert r["cost"] == want["cost"] and r["norm"] == want["norm"] and r["c"] == want["c"]
        assert (r["c"] < 1.0) == (mx < probe["norm"])
        assert np.array_equal(r["theta"], ref.get_params()) and np.array_equal(r["m"], ref.m) and np.array_equal(r["v"], ref.v)


def test_schedules_corruption_and_average_enter_where_documented(setup):
    """The remaining stages, each against its own reference: lambda_t / lr_eff_t are schedule_reference.hyper's fp32 products of
    the step's number, the draw is keyed by the counter before the step, the average follows the updated parameters."""
    p0, X, eps, P = setup
    assoc, lrs = dict(knots=[(0, 0.25), (4, 1.5)]), dict(knots=[(0, 1.0), (3, 0.25)])
    corr = dict(seed=11, drop=[0.5, 0.2], noise=0.0, drop_value=[0.0, 3.0])
    e0 = p0 + 0.01
    r = composed_step(ARCHS, p0, _zeros(), _zeros(), 2, X, eps, BIN, W, LAM, ACT, LR, present=P, corruption=corr, assoc=assoc,
                      lr_schedule=lrs, max_norm=1e-3, ema=dict(e=e0, decay=0.9, warmup=True))
    _, lam3, lr3 = hyper(None, assoc, lrs, LAM, LR, 3)
    assert r["t"] == 3 and r["lambda_t"] == float(lam3) and r["lr_t"] == float(lr3) and lam3 != np.float32(LAM) and lr3 != np.float32(LR)
    xin = corrupted_inputs(X, 11, 2, corr["drop"], 0.0, corr["drop_value"])
    assert all(np.array_equal(a, b) for a, b in zip(r["X_in"], xin))
    assert not np.array_equal(xin[0], corrupted_inputs(X, 11, 3, corr["drop"], 0.0, corr["drop_value"])[0])
    assert r["c"] < 1.0 and np.array_equal(r["ema"], ema_step(e0, r["theta"], 0.9, True, 3))
    th, _, _ = O.adam_step(p0, _zeros(), _zeros(), r["g"] * r["c"], 3, float(lr3))
    assert np.array_equal(r["theta"], th)


@pytest.mark.parametrize("corr", [dict(drop=[0.5, 0.1], noise=[0.0, 0.5], drop_value=[0.0, -1.0]),
                                  dict(drop=[0.5, 0.2], noise=0.0, drop_value=[0.0, 3.0])])
def test_a_loss_against_the_wrong_buffer_is_far_outside_the_tolerance(setup, corr):
    """The corruptions tests/test_gpu_big_options.py uses: at least a tenth of the elements of either modality differ between the
    clean and the corrupted rows, and the cost charged against the corrupted rows is more than 100 x the bf16 cost tolerance
    (5e-5, the wider of the two) away from the true one -- unmasked and under the mask."""
    p0, X, eps, P = setup
    xin = corrupted_inputs(X, 11, 0, corr["drop"], corr["noise"], corr["drop_value"])
    for k in range(2):
        assert np.mean(xin[k] != X[k]) >= 0.1, k
    for present in (None, P):
        true, wrong = wrong_buffer_margin(ARCHS, p0, X, xin, eps, BIN, W, LAM, ACT, present=present)
        assert abs(wrong - true) > 100 * 5e-5 * abs(true), (true, wrong)
