"""Runs of steps store the gradient only on a replay's last step (k_small_tn_nograd) -- against handles that store it every step.

In the small nets' fused step nothing on the device reads the gradient buffer, and inside a replayed graph of 16 or 4 steps step
j + 1 overwrites step j's gradient before the host can ask for it (avae_host.hip: step_body).  So a default handle runs the
non-storing instance of the wgrad+adam launch for every step but a graph's last; a handle created under AVAE_KEEP_GRADS=1 runs the
storing one everywhere, and so does a handle that takes the same batches as single steps.  Same tiles, same K order, same
arithmetic: everything compared here -- theta, m, v, the gradient, the cost history, the step counter -- is compared bitwise, and
both weight shadows must be the parameters after every run."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_arch, shadow_err
from plan_dump import with_switches
from test_gpu_descriptors import assert_same, batches, state, steps

pytestmark = pytest.mark.gpu

# every tile an edge tile (the partial-quad arm runs) / interior `full` tiles beside both edge arms
NETS = {"edge": ([make_arch("image", 70, 65, 40, 7), make_arch("joint", 33, 33, 24, 7)], 32),
        "interior": ([make_arch("image", 191, 129, 128, 7), make_arch("joint", 70, 65, 64, 7)], 64)}
RUNS = [1, 2, 4, 5, 16, 17, 20, 21, 36]
KW = dict(binary=[True, False], seed=3, transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0)
DEFAULT_FLAGS = [0] * 15 + [1] + [0, 0, 0, 1] + [1]


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def make(V, monkeypatch, net, dtype, keep, **kw):
    """a handle of NETS[net]; keep: created under AVAE_KEEP_GRADS=1 (read once by avae_create)"""
    archs, B = NETS[net]
    monkeypatch.delenv("AVAE_KEEP_GRADS", raising=False)
    return with_switches(monkeypatch, {"AVAE_KEEP_GRADS": "1"} if keep else {},
                         lambda: V.AssocVariationalAutoEncoder(archs, batch_size=B, compute_dtype=dtype, **dict(KW, **kw)))


def grad_keep(m, key=b"grad_keep"):
    buf = np.full(32, -1.0, np.float32)
    cnt = C.c_size_t(0)
    rc = m._L.avae_debug_fetch(m._h, key, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt))
    assert rc == 0, m._L.avae_last_error(m._h)
    return [int(x) for x in buf[:cnt.value]]


def data(net, n, seed=4):
    archs, B = NETS[net]
    widths = [int(a["n_input"]) for a in archs]
    X, eps = batches(seed, n, B, widths, KW["binary"], int(archs[0]["n_z"]))
    return X, eps, [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()


_SINGLE = {}


def single_steps(V, monkeypatch, net, dtype):
    """(initial parameters, {n: state after n single steps}) of one handle that takes the 36 batches one partial_fit at a time:
    computed once per net and dtype, shared by the run lengths"""
    if (net, dtype) not in _SINGLE:
        X, eps, _Xd, _ed = data(net, max(RUNS))
        B = NETS[net][1]
        m = make(V, monkeypatch, net, dtype, False)
        p0 = m.get_params()
        snaps = {}
        for i in range(max(RUNS)):
            m.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B], return_cost=False)
            if i + 1 in RUNS:
                snaps[i + 1] = state(m, i + 1)
        assert len(set(snaps[max(RUNS)]["costs"].tolist())) == max(RUNS)
        _SINGLE[(net, dtype)] = (p0, snaps)
    return _SINGLE[(net, dtype)]


def test_keep_flags(V, monkeypatch):
    """the last step of every captured graph stores, the others do not; everything stores under the switch and with an unfused tail"""
    m = make(V, monkeypatch, "edge", "bf16", False)
    assert grad_keep(m) == DEFAULT_FLAGS
    assert grad_keep(make(V, monkeypatch, "edge", "bf16", True)) == [1] * 21
    m.set_grad_clip(max_norm=0.5)
    assert grad_keep(m) == [1] * 21
    m.set_grad_clip(max_norm=0.0)
    assert grad_keep(m) == DEFAULT_FLAGS
    m.set_ema(0.9)
    assert grad_keep(m) == [1] * 21
    # the masked plan is built by the first masked call and shares step_body
    B = NETS["edge"][1]
    X, eps, _Xd, _ed = data("edge", 1)
    d = make(V, monkeypatch, "edge", "fp32", False)
    d.partial_fit(X, eps, present=np.ones((B, 2), np.uint8))
    assert grad_keep(d, b"grad_keep_masked") == DEFAULT_FLAGS
    assert grad_keep(d) == DEFAULT_FLAGS


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("n", RUNS)
def test_runs_equal_keeping_twin_and_single_steps(V, monkeypatch, n, net, dtype):
    p0, snaps = single_steps(V, monkeypatch, net, dtype)
    _X, _eps, Xd, ed = data(net, max(RUNS))
    rows = n * NETS[net][1]
    Xd, ed = [x[:rows] for x in Xd], ed[:rows]
    out = []
    for keep in (False, True):
        m = make(V, monkeypatch, net, dtype, keep)
        m.set_params(p0)
        m.partial_fit_steps(Xd, n, ed)
        out.append(state(m, n))
    assert_same(out[0], out[1], "default vs AVAE_KEEP_GRADS=1")
    assert_same(out[0], snaps[n], "runs vs single steps")


def _present(n, B):
    p = np.ones((n * B, 2), np.uint8)
    p[::3, 0] = 0
    p[1::4, 1] = 0
    p[p.sum(1) == 0, 0] = 1
    return p


@pytest.mark.parametrize("option", ["masks", "denoising", "schedule", "clipping+ema"])
def test_options(V, monkeypatch, option):
    n, net = 20, "edge"
    B = NETS[net][1]
    _X, _eps, Xd, ed = data(net, n, seed=6)
    prepare = {"masks": lambda m: None,
               "denoising": lambda m: m.set_corruption(drop=0.2, noise=0.1),
               "schedule": lambda m: m.set_schedule(kl=dict(knots=[(0, 0.0), (4, 1.0)]), lr=0.5),
               "clipping+ema": lambda m: (m.set_grad_clip(max_norm=0.5), m.set_ema(0.9))}[option]
    fit_kw = dict(present=_present(n, B)) if option == "masks" else {}
    ms, out = [], []
    for keep in (False, True):
        m = make(V, monkeypatch, net, "bf16", keep)
        if keep:
            m.set_params(ms[0].get_params())
        ms.append(m)
    for m in ms:
        prepare(m)
        m.partial_fit_steps(Xd, n, ed, **fit_kw)
        out.append(state(m, n))
    assert_same(out[0], out[1], option)
    assert len(set(out[0]["costs"].tolist())) == n
    if option == "clipping+ema":
        assert np.array_equal(ms[0].get_ema_params(), ms[1].get_ema_params())


def test_interleaved_with_reads_and_inference(V, monkeypatch):
    net = "interior"
    B = NETS[net][1]
    X, eps, Xd, ed = data(net, 21, seed=8)
    a, b = make(V, monkeypatch, net, "bf16", False), make(V, monkeypatch, net, "bf16", True)
    b.set_params(a.get_params())

    def both(what, f):
        ra, rb = f(a), f(b)
        for x, y in zip(ra, rb):
            assert np.array_equal(np.asarray(x), np.asarray(y)), what
    cut = lambda lo, hi: ([x[lo * B:hi * B] for x in Xd], ed[lo * B:hi * B])
    for m in (a, b):
        m.partial_fit_steps(cut(0, 16)[0], 16, cut(0, 16)[1])
    both("get_grads after 16", lambda m: [m.get_grads()])
    both("transform", lambda m: [m.transform([x[:B] for x in X])])
    both("generate", lambda m: m.generate(eps[:B]))
    for m in (a, b):
        m.partial_fit_steps(cut(16, 20)[0], 4, cut(16, 20)[1])
    both("get_grads after 16 + 4", lambda m: [m.get_grads()])
    assert_same(state(a, 20), state(b, 20), "after 16 + 4")
    for m in (a, b):
        m.partial_fit(*cut(20, 21))
    assert_same(state(a, 21), state(b, 21), "after 16 + 4 + 1")


def test_repeated_runs_are_deterministic(V):
    """One 20-step run (a 16-step and a 4-step replay), 25 times from the same weights at the benchmark's layer sizes: the
    non-storing instance issues one store fewer per quad, and no counted wait of the launch may come to depend on it."""
    archs = [make_arch("image", 784, 500, 500, 32), make_arch("joint", 147, 200, 200, 32)]
    B, n = 64, 20
    X, eps = batches(5, n, B, [784, 147], [True, False], 32)
    Xd, ed = [torch.as_tensor(x).cuda() for x in X], torch.as_tensor(eps).cuda()
    p0 = None

    def run():
        nonlocal p0
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[1.0, 50.0], assoc_lambda=0.0,
                                          batch_size=B, compute_dtype="fp32", seed=7)
        if p0 is None:
            p0 = m.get_params()
            assert grad_keep(m) == DEFAULT_FLAGS
        m.set_params(p0)
        m.partial_fit_steps(Xd, n, ed, return_cost=False)
        return state(m, n)
    first = run()
    assert first["shadow"] == (0.0, 0.0)
    differing = sum(1 for _ in range(25) if any(not np.array_equal(v, first[k]) for k, v in run().items() if k != "shadow"))
    assert differing == 0, "%d of 25 runs differ from the first" % differing
