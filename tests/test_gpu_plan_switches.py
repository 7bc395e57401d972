"""The planner's environment switches are read once per handle, by avae_create (avae_host.hip: PlanSwitches, read_switches): the
plans a handle builds on a later first call -- the serve plan of generate(), the masked twin of the step -- follow the switches
the handle was created under, not the environment of that call.

Net: 784-24-24 / 147-12-12, n_z 4, batch 32 (the fused small-net plan of tests/test_gpu_schedule.py, model A): its default serve
plan takes the lean staging launch (k_serve_in, lean_in=1) and its default output + loss launch is the lean one (tile
configuration 9) -- both asserted first, on a handle created with no planner switch set, so that a planner change cannot turn
these tests vacuous.  Everything compared between handles is compared bitwise: same seed, same inputs, same plan."""
import numpy as np
import pytest
import torch

import plan_dump
from conftest import make_arch, synth_batch
from plan_dump import with_switches

pytestmark = pytest.mark.gpu

ARCHS = [make_arch("image", 784, 24, 24, 4), make_arch("joint", 147, 12, 12, 4)]
B, NZ = 32, 4
KW = dict(binary=[True, False], transfer_fct="relu", batch_size=B, compute_dtype="bf16", seed=5)
LEAN_LOSS = 9          # TileCfg::kLeanLoss (avae_device.h)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def new(V):
    return V.AssocVariationalAutoEncoder(ARCHS, **KW)


Z1 = np.random.default_rng(3).standard_normal((1, NZ)).astype(np.float32)


def first_generate(m, capfd):
    """(outputs, serve plans) of the handle's first generate() of one row (the handle prints: created under AVAE_PLAN_DUMP=1)"""
    capfd.readouterr()
    out = m.generate(Z1)
    m.synchronize()
    plans = plan_dump.parse_serve(capfd.readouterr().err)
    assert len(plans) == 1, plans
    return [np.asarray(o) for o in out], next(iter(plans.values()))


def same_outputs(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(8)
    X = synth_batch(rng, B, [784, 147], [True, False])
    eps = rng.standard_normal((B, NZ)).astype(np.float32)
    P = rng.random((B, 2)) < 0.6
    P[0] = [True, False]                     # at least one absent entry, and every column both ways
    P[1] = [False, True]
    return X, eps, P


def test_serve_plan_follows_the_switches_of_creation(V, monkeypatch, capfd):
    default = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"}, lambda: new(V))
    out_d, sv_d = first_generate(default, capfd)
    assert sv_d["fused_in"] and sv_d["lean_in"], sv_d          # the precondition: the default plan takes the lean staging launch
    env = {"AVAE_NO_LEAN": "1", "AVAE_PLAN_DUMP": "1"}
    out_a, sv_a = with_switches(monkeypatch, env, lambda: first_generate(new(V), capfd))      # set from creation through the call
    assert sv_a["fused_in"] and not sv_a["lean_in"] and sv_a != sv_d, sv_a
    b = with_switches(monkeypatch, env, lambda: new(V))         # set during creation only
    out_b, sv_b = first_generate(b, capfd)
    assert sv_b == sv_a, (sv_b, sv_a)
    assert same_outputs(out_b, out_a)


def test_serve_plan_ignores_a_switch_set_after_creation(V, monkeypatch, capfd):
    default = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"}, lambda: new(V))
    out_d, sv_d = first_generate(default, capfd)
    assert sv_d["lean_in"], sv_d
    late = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"}, lambda: new(V))
    out_l, sv_l = with_switches(monkeypatch, {"AVAE_NO_LEAN": "1"}, lambda: first_generate(late, capfd))
    assert sv_l == sv_d, (sv_l, sv_d)
    assert same_outputs(out_l, out_d)


def first_masked_step(m, capfd, batch):
    """(cost, parameters, step plan) of the handle's first masked partial_fit (the handle prints: created under AVAE_DEBUG_SYNC=1)"""
    X, eps, P = batch
    capfd.readouterr()
    cost = m.partial_fit(X, eps, present=P)
    m.synchronize()
    plan = plan_dump.parse(capfd.readouterr().err)
    assert plan, "no launch dump under AVAE_DEBUG_SYNC=1"
    return cost, m.get_params(), plan


def test_masked_plan_follows_the_switches_of_creation(V, monkeypatch, capfd, batch):
    default = with_switches(monkeypatch, {"AVAE_DEBUG_SYNC": "1"}, lambda: new(V))
    _, _, plan_d = first_masked_step(default, capfd, batch)
    assert plan_dump.launch(plan_d, "fwd_out_loss")[0] == LEAN_LOSS, plan_d      # the precondition: the lean output + loss launch
    env = {"AVAE_NO_LEAN_LOSS": "1", "AVAE_DEBUG_SYNC": "1"}
    cost_a, theta_a, plan_a = with_switches(monkeypatch, env, lambda: first_masked_step(new(V), capfd, batch))
    b = with_switches(monkeypatch, env, lambda: new(V))
    cost_b, theta_b, plan_b = first_masked_step(b, capfd, batch)
    cfg_a, cfg_b = plan_dump.launch(plan_a, "fwd_out_loss")[0], plan_dump.launch(plan_b, "fwd_out_loss")[0]
    assert cfg_b == cfg_a and cfg_a != LEAN_LOSS, (cfg_a, cfg_b)
    assert plan_b == plan_a
    assert np.float32(cost_b).tobytes() == np.float32(cost_a).tobytes(), (cost_a, cost_b)
    assert theta_b.tobytes() == theta_a.tobytes()
