"""Per-workgroup launch descriptors of the small-net training plan (k_small_desc, k_small_tn_desc) against the by-value kernels.

A default handle runs the hidden forward / hidden dgrad launches and the weight-gradient + Adam launch of its step on records that
the host resolved per workgroup (avae_device.h: SmallDesc, TnDesc); a handle created under AVAE_NO_DESC=1 runs the same plan on
the by-value kernels.  Same tiles, same K order, same addresses: everything compared here is compared bitwise."""
import numpy as np
import pytest
import torch

from conftest import make_arch, synth_batch, shadow_err
from plan_dump import with_switches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def twins(V, monkeypatch, archs, **kw):
    """(default handle, AVAE_NO_DESC=1 handle) of one model; the switch is read when the plan is built"""
    monkeypatch.delenv("AVAE_NO_DESC", raising=False)
    on = V.AssocVariationalAutoEncoder(archs, **kw)
    off = with_switches(monkeypatch, {"AVAE_NO_DESC": "1"}, lambda: V.AssocVariationalAutoEncoder(archs, **kw))
    off.set_params(on.get_params())
    return on, off


def state(m, n_costs):
    mo, vo, step = m.get_opt_state()
    return dict(theta=m.get_params(), m=mo, v=vo, g=m.get_grads(), costs=m.cost_history(n_costs).copy(), step=step,
                shadow=shadow_err(m)[:2])


def assert_same(a, b, what=""):
    for k in a:
        if k == "shadow":
            assert a[k] == (0.0, 0.0) and b[k] == (0.0, 0.0), (what, k, a[k], b[k])
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def batches(seed, n, B, widths, binary, nz):
    rng = np.random.default_rng(seed)
    X = synth_batch(rng, n * B, widths, binary)
    eps = rng.standard_normal((n * B, nz)).astype(np.float32)
    return X, eps


def steps(m, X, eps, n, B, **kw):
    for i in range(n):
        m.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B], **kw)


def run_twins(V, monkeypatch, archs, binary, B, n=3, prepare=None, fit_kw=None, seed=11, **kw):
    nz = int(archs[0]["n_z"])
    widths = [int(a["n_input"]) for a in archs]
    X, eps = batches(seed, n, B, widths, binary, nz)
    on, off = twins(V, monkeypatch, archs, binary=binary, batch_size=B, seed=3, **kw)
    out = []
    for m in (on, off):
        if prepare:
            prepare(m)
        steps(m, X, eps, n, B, **(fit_kw(B) if fit_kw else {}))
        out.append(state(m, n))
    assert_same(out[0], out[1])
    return on, off, X, eps


def test_default_plan_runs_on_descriptors(V, monkeypatch, capfd):
    """The comparison below is one of two different kernels: the default handle's k_small and wgrad+adam launches print their record
    counts in the AVAE_DEBUG_SYNC dump, the AVAE_NO_DESC=1 handle's print none."""
    archs = [make_arch("image", 70, 65, 65, 5), make_arch("joint", 33, 33, 33, 5)]
    X, eps = batches(1, 1, 48, [70, 33], [True, False], 5)
    seen = {}
    for env in ({}, {"AVAE_NO_DESC": "1"}):
        m = with_switches(monkeypatch, dict(env, AVAE_DEBUG_SYNC="1"),
                          lambda: V.AssocVariationalAutoEncoder(archs, binary=[True, False], batch_size=48, compute_dtype="bf16", seed=3))
        capfd.readouterr()
        m.partial_fit(X, eps)
        m.synchronize()
        text = capfd.readouterr().err.splitlines()
        seen[bool(env)] = [text[i - 1].split()[2] for i, ln in enumerate(text) if ln.strip().startswith("descriptors=")]
    assert seen[True] == []
    # 2 hidden layers a side: fwd_enc1, fwd_enc2, fwd_dec2 (fwd_dec1 rides in the head launch), bwd_out, bwd_dec2, bwd_enc2, wgrad+adam
    assert seen[False] == ["fwd_enc1", "fwd_enc2", "fwd_dec2", "bwd_out", "bwd_dec2", "bwd_enc2", "wgrad+adam"], seen[False]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_single_k_tile_every_tile_an_edge(V, monkeypatch, dtype):
    archs = [make_arch("image", 40, 24, 24, 5), make_arch("joint", 12, 16, 16, 5)]
    run_twins(V, monkeypatch, archs, [True, False], 32, transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, compute_dtype=dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("act", ["relu", "softplus", "sigmoid", "tanh", "identity"])
def test_widths_off_tile_and_quad(V, monkeypatch, act, dtype):
    """n_in 70 / 33, hidden 65 / 33, n_z 31, B 48: store_row's partial arm and the partial-quad arm of the Adam epilogue"""
    archs = [make_arch("image", 70, 65, 65, 31), make_arch("joint", 33, 33, 33, 31)]
    run_twins(V, monkeypatch, archs, [True, False], 48, transfer_fct=act, weights=[50, 1], assoc_lambda=8.0, compute_dtype=dtype)


def test_three_modalities_fp32(V, monkeypatch):
    archs = [make_arch("a", 96, 80, 64, 12), make_arch("b", 50, 48, 40, 12), make_arch("c", 21, 32, 24, 12)]
    run_twins(V, monkeypatch, archs, [True, False, False], 40, transfer_fct="relu", weights=[50, 1, 1], assoc_lambda=4.0, compute_dtype="fp32")


def test_four_modalities_eight_hidden_layers(V, monkeypatch):
    """the ABI maxima: most items per launch, most records"""
    hs = [16, 24, 40, 32, 20, 36, 28, 16]
    archs = [make_arch("m%d" % i, n, 0, 0, 6, n_hidden=hs[i:] + hs[:i]) for i, n in enumerate([44, 30, 17, 9])]
    run_twins(V, monkeypatch, archs, [True, False, False, True], 32, transfer_fct="tanh", weights=[10, 1, 1, 5], assoc_lambda=2.0,
              compute_dtype="bf16")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_runs_of_steps_equal_single_steps(V, monkeypatch, dtype):
    """16 + 4 steps per replay (the records of staging sets 0..15, each step's last launch warming the next step's first) against
    the same 20 single steps, and both against the by-value twin"""
    archs = [make_arch("image", 70, 65, 40, 7), make_arch("joint", 33, 33, 24, 7)]
    n, B = 20, 32
    X, eps = batches(4, n, B, [70, 33], [True, False], 7)
    Xd, ed = [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()
    on, off = twins(V, monkeypatch, archs, binary=[True, False], batch_size=B, seed=3, transfer_fct="relu", weights=[50, 1],
                    assoc_lambda=8.0, compute_dtype=dtype)
    single = with_switches(monkeypatch, {}, lambda: V.AssocVariationalAutoEncoder(
        archs, binary=[True, False], batch_size=B, seed=3, transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, compute_dtype=dtype))
    single.set_params(on.get_params())
    on.partial_fit_steps(Xd, n, ed)
    off.partial_fit_steps(Xd, n, ed)
    steps(single, X, eps, n, B)
    ref = state(single, n)
    assert len(set(ref["costs"].tolist())) == n
    assert_same(state(on, n), ref, "runs vs single steps")
    assert_same(state(off, n), ref, "by-value runs vs single steps")


@pytest.mark.parametrize("act", ["identity", "relu"])
def test_back_to_back_steps_equal_synchronised_steps(V, act):
    """Three single steps back to back, 25 times, against the same steps with a host synchronisation after each: the warm-up loads
    are scalar loads and must not move a counted wait of the K loops (the pattern of test_gpu_parity's test of the same name)."""
    archs = [make_arch("image", 784, 500, 500, 32), make_arch("joint", 147, 200, 200, 32)]
    B, n = 64, 3
    X, eps = batches(5, n, B, [784, 147], [True, False], 32)
    Xd, ed = [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()
    p0 = None

    def run(sync):
        nonlocal p0
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct=act, weights=[1.0, 50.0], assoc_lambda=0.0, batch_size=B,
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
    differing = sum(1 for _ in range(25) if not np.array_equal(run(False), truth))
    assert differing == 0, "%d of 25 back-to-back runs differ from the synchronised run" % differing


ARCHS_OPT = [make_arch("image", 70, 65, 40, 7), make_arch("joint", 33, 33, 24, 7)]


def _present(B):
    p = np.ones((B, 2), np.uint8)
    p[::3, 0] = 0
    p[1::4, 1] = 0
    p[p.sum(1) == 0, 0] = 1
    return dict(present=p)


@pytest.mark.parametrize("option", ["masks", "denoising", "clipping", "schedule", "ema"])
def test_plan_options(V, monkeypatch, option):
    """the options that change launch arguments or the step's tail"""
    prepare = {"masks": None,
               "denoising": lambda m: m.set_corruption(drop=0.2, noise=0.1),
               "clipping": lambda m: m.set_grad_clip(max_norm=0.5),
               "schedule": lambda m: m.set_schedule(kl=dict(knots=[(0, 0.0), (4, 1.0)]), lr=0.5),
               "ema": lambda m: m.set_ema(0.9)}[option]
    on, off, _X, _eps = run_twins(V, monkeypatch, ARCHS_OPT, [True, False], 32, prepare=prepare,
                                  fit_kw=_present if option == "masks" else None, transfer_fct="relu", weights=[50, 1],
                                  assoc_lambda=8.0, compute_dtype="bf16")
    if option == "ema":
        assert np.array_equal(on.get_ema_params(), off.get_ema_params())


def test_two_handles_stepping_alternately(V, monkeypatch):
    archs = ARCHS_OPT
    B, n = 32, 3
    X, eps = batches(8, n, B, [70, 33], [True, False], 7)
    kw = dict(binary=[True, False], batch_size=B, seed=3, transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, compute_dtype="bf16")
    a, ref = twins(V, monkeypatch, archs, **kw)
    b = V.AssocVariationalAutoEncoder(archs, **kw)
    b.set_params(a.get_params())
    for i in range(n):
        for m in (a, b):
            m.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B], return_cost=False)
    steps(ref, X, eps, n, B)
    want = state(ref, n)
    assert_same(state(a, n), want, "first handle")
    assert_same(state(b, n), want, "second handle")


def test_set_params_and_restore_then_step(V, monkeypatch, tmp_path, capsys):
    B = 32
    X, eps = batches(9, 3, B, [70, 33], [True, False], 7)
    on, off = twins(V, monkeypatch, ARCHS_OPT, binary=[True, False], batch_size=B, seed=3, transfer_fct="relu", weights=[50, 1],
                    assoc_lambda=8.0, compute_dtype="bf16")
    for m in (on, off):
        steps(m, X, eps, 2, B)
    on.save_model(str(tmp_path / "d.ckpt"))
    p = on.get_params() * np.float32(0.5)
    for m in (on, off):
        m.set_params(p)
        steps(m, X, eps, 1, B)
    assert_same(state(on, 3), state(off, 3), "after set_params")
    for m in (on, off):
        m.restore_model(str(tmp_path), "d.ckpt")
        m.partial_fit([x[2 * B:] for x in X], eps[2 * B:])
    assert_same(state(on, 1), state(off, 1), "after restore_model")
    capsys.readouterr()


def test_inference_after_training(V, monkeypatch):
    on, off, X, eps = run_twins(V, monkeypatch, ARCHS_OPT, [True, False], 32, transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                compute_dtype="bf16")
    z = eps[:32]
    for a, b in zip(on.generate(z), off.generate(z)):
        assert np.array_equal(a, b)
    assert np.array_equal(np.asarray(on.transform([x[:32] for x in X])), np.asarray(off.transform([x[:32] for x in X])))
