"""The record kernels of the output + loss launch and the two fused head launches (k_loss_rec, k_head_rec, k_latb_rec) against the
by-value kernels.

A default handle runs fwd_head+fwd_dec1, fwd_out_loss and bwd_dec1_latent+bwd_head of its plain training step on two-line records
that the host resolved per workgroup (avae_device.h: LossRec, HeadRec); a handle created under AVAE_NO_DESC=1 runs the same plan on
the by-value kernels.  The tile bodies are shared, so everything compared here is compared bitwise."""
import numpy as np
import pytest
import torch

from conftest import make_arch
from plan_dump import with_switches
from test_gpu_descriptors import V, assert_same, batches, run_twins, state, twins  # noqa: F401  (V: the module's fixture)

pytestmark = pytest.mark.gpu

HEADS = ["fwd_head+fwd_dec1", "fwd_out_loss", "bwd_dec1_latent+bwd_head"]
OLD = ["fwd_enc1", "fwd_enc2", "fwd_dec2", "bwd_out", "bwd_dec2", "bwd_enc2", "wgrad+adam"]
KW = dict(transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0)


def labels(text):
    """(launches that printed records=, launches that printed descriptors=) of an AVAE_DEBUG_SYNC dump, in the order they ran"""
    lines = text.splitlines()
    def named(key):
        return [lines[i - 1].split()[2] for i, ln in enumerate(lines) if ln.strip().startswith(key)]
    return named("records="), named("descriptors=")


def dumped_step(V, monkeypatch, capfd, env, archs, B, nz, dtype="bf16", fit_kw=None):
    """one step of a handle created under `env` + AVAE_DEBUG_SYNC=1: (the handle, its labels)"""
    widths = [int(a["n_input"]) for a in archs]
    X, eps = batches(1, 1, B, widths, [True, False], nz)
    m = with_switches(monkeypatch, dict(env, AVAE_DEBUG_SYNC="1"),
                      lambda: V.AssocVariationalAutoEncoder(archs, binary=[True, False], batch_size=B, compute_dtype=dtype, seed=3, **KW))
    capfd.readouterr()
    m.partial_fit(X, eps, **(fit_kw or {}))
    m.synchronize()
    return m, labels(capfd.readouterr().err)


def test_dump_labels(V, monkeypatch, capfd):
    archs = [make_arch("image", 70, 65, 65, 5), make_arch("joint", 33, 33, 33, 5)]
    _, (recs, descs) = dumped_step(V, monkeypatch, capfd, {}, archs, 48, 5)
    assert recs == HEADS, recs
    assert descs == OLD, descs
    _, (recs, descs) = dumped_step(V, monkeypatch, capfd, {"AVAE_NO_DESC": "1"}, archs, 48, 5)
    assert recs == [] and descs == [], (recs, descs)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B", [48, 32])
@pytest.mark.parametrize("nz", [5, 16, 17, 31, 32])
def test_nz_classes_of_the_head_tile(V, monkeypatch, nz, B, dtype):
    """n_z below / at / above one fp32 K tile of [dmu | dlv] (tail_kt = 2 above 16) and at the 64-column limit of the head tile; widths
    off the tile and off the quad; B = 48: a partial second row block"""
    archs = [make_arch("image", 70, 65, 65, nz), make_arch("joint", 33, 33, 33, nz)]
    run_twins(V, monkeypatch, archs, [True, False], B, n=2, compute_dtype=dtype, **KW)


def test_nz_33_leaves_the_lean_head_launches(V, monkeypatch, capfd):
    """2 n_z > 64: the head launches run on the general kernel -- no records for them, and the step still equals its twin"""
    archs = [make_arch("image", 70, 65, 65, 33), make_arch("joint", 33, 33, 33, 33)]
    _, (recs, _descs) = dumped_step(V, monkeypatch, capfd, {}, archs, 48, 33)
    assert not any("head" in r for r in recs), recs
    run_twins(V, monkeypatch, archs, [True, False], 48, n=2, compute_dtype="bf16", **KW)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_tail_slices(V, monkeypatch, dtype):
    """decoder first layer of 130 units: three 64-column tail slices, the last partial; encoder last layer of 65 units: two slices of
    the heads' input gradient, the second of one column"""
    archs = [make_arch("image", 70, 130, 65, 12), make_arch("joint", 33, 130, 65, 12)]      # (the decoder reuses the encoder's widths, in order)
    run_twins(V, monkeypatch, archs, [True, False], 48, n=2, compute_dtype=dtype, **KW)


def test_three_modalities_fp32(V, monkeypatch):
    archs = [make_arch("a", 96, 80, 64, 12), make_arch("b", 50, 48, 40, 12), make_arch("c", 21, 32, 24, 12)]
    run_twins(V, monkeypatch, archs, [True, False, False], 40, transfer_fct="relu", weights=[50, 1, 1], assoc_lambda=4.0, compute_dtype="fp32")


def test_four_modalities_eight_hidden_layers(V, monkeypatch):
    """the latent item's largest n_mod, the most records"""
    hs = [16, 24, 40, 32, 20, 36, 28, 16]
    archs = [make_arch("m%d" % i, n, 0, 0, 6, n_hidden=hs[i:] + hs[:i]) for i, n in enumerate([44, 30, 17, 9])]
    run_twins(V, monkeypatch, archs, [True, False, False, True], 32, transfer_fct="tanh", weights=[10, 1, 1, 5], assoc_lambda=2.0,
              compute_dtype="bf16")


ARCHS_OPT = [make_arch("image", 70, 65, 40, 7), make_arch("joint", 33, 33, 24, 7)]


def test_schedule_on(V, monkeypatch):
    """a KL ramp and an LR factor: the latent and cost items are patched per step and read by value, beside the records"""
    run_twins(V, monkeypatch, ARCHS_OPT, [True, False], 32, n=3, compute_dtype="bf16",
              prepare=lambda m: m.set_schedule(kl=dict(knots=[(0, 0.0), (4, 1.0)]), lr=0.5), **KW)


def _present(B):
    p = np.ones((B, 2), np.uint8)
    p[::3, 0] = 0
    p[1::4, 1] = 0
    p[p.sum(1) == 0, 0] = 1
    return dict(present=p)


def test_masked_steps_stay_by_value(V, monkeypatch, capfd):
    _, (recs, _descs) = dumped_step(V, monkeypatch, capfd, {}, ARCHS_OPT, 32, 7, fit_kw=_present(32))
    assert recs == [], recs
    run_twins(V, monkeypatch, ARCHS_OPT, [True, False], 32, n=3, fit_kw=_present, compute_dtype="bf16", **KW)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_runs_of_steps_equal_single_steps(V, monkeypatch, dtype):
    """16 + 4 steps per replay (the records of staging sets 0..15) against the same 20 single steps, and both against the twin"""
    n, B = 20, 32
    X, eps = batches(4, n, B, [70, 33], [True, False], 7)
    Xd, ed = [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()
    kw = dict(binary=[True, False], batch_size=B, seed=3, compute_dtype=dtype, **KW)
    on, off = twins(V, monkeypatch, ARCHS_OPT, **kw)
    single = with_switches(monkeypatch, {}, lambda: V.AssocVariationalAutoEncoder(ARCHS_OPT, **kw))
    single.set_params(on.get_params())
    on.partial_fit_steps(Xd, n, ed)
    off.partial_fit_steps(Xd, n, ed)
    for i in range(n):
        single.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B])
    ref = state(single, n)
    assert len(set(ref["costs"].tolist())) == n
    assert_same(state(on, n), ref, "runs vs single steps")
    assert_same(state(off, n), ref, "by-value runs vs single steps")


def test_back_to_back_steps_equal_synchronised_steps(V):
    """Three single steps back to back, 10 times, against the same steps with a host synchronisation after each: the warm-up loads
    are scalar loads and must not move a counted wait of the head kernels (kExtra in the backward one)."""
    archs = [make_arch("image", 784, 500, 500, 32), make_arch("joint", 147, 200, 200, 32)]
    B, n = 64, 3
    X, eps = batches(5, n, B, [784, 147], [True, False], 32)
    Xd, ed = [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()
    p0 = None

    def run(sync):
        nonlocal p0
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[1.0, 50.0], assoc_lambda=0.0, batch_size=B,
                                          compute_dtype="fp32", seed=7)
        if p0 is None:
            p0 = m.get_params()
        m.set_params(p0)
        for i in range(n):
            m.partial_fit([x[i * B:(i + 1) * B] for x in Xd], ed[i * B:(i + 1) * B], return_cost=False)
            if sync:
                torch.cuda.synchronize()
        return m.get_params()
    truth = run(True)
    differing = sum(1 for _ in range(10) if not np.array_equal(run(False), truth))
    assert differing == 0, "%d of 10 back-to-back runs differ from the synchronised run" % differing
