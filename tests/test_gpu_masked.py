"""Partially paired training on a real MI355X (include/avae.h: avae_train_steps_masked / avae_eval_cost_masked; DESIGN.md
section 10): an all-present mask is bit for bit the unmasked step, a random mask matches the pattern-composed oracle of
tests/masked_reference.py, absent entries are never read, an absent modality gets exact zeros, every planner route honours the
mask, the masked evaluation is the per-row formula on score_samples' columns, and multi-step replays are the single steps.

Tolerances as tests/test_gpu_parity.py: fp32 against the fp64 reference (cost 1e-5 relative, gradients 1e-4 of each tensor's
maximum), bf16 against the reference run with quant='bf16' and the kernels' relu decisions (cost 5e-5, gradients 3e-3)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import hip_relu_masks, make_arch, shadow_err, synth_batch
from masked_reference import masked_cost_and_grads, masked_cost_from_rows
from oracle import vae_assoc_oracle as O

pytestmark = pytest.mark.gpu

C2 = dict(archs=[make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)], binary=[True, False],
          weights=[50.0, 1.0], lam=8.0, B=100)
THREE = dict(archs=[make_arch("a", 60, 32, 24, 8), make_arch("b", 21, 16, 16, 8), make_arch("c", 33, 24, 16, 8)],
             binary=[True, False, False], weights=[2.0, 1.0, 0.5], lam=0.7, B=64)
CONV = dict(archs=[dict(make_arch("image", 784, 8, 24, 6), hidden_conv=True, n_hidden_gener_1=24, n_hidden_gener_2=8),
                   make_arch("joint", 147, 40, 30, 6)], binary=[True, False], weights=[5.0, 1.0], lam=0.5, B=32)
# the big nets' plan: 256x64 8-wave loss tiles (register epilogue) and the latent item in a launch of its own
BIG = dict(archs=[make_arch("a", 784, 0, 0, 16, n_hidden=[64, 48]), make_arch("b", 147, 0, 0, 16, n_hidden=[64, 48])],
           binary=[True, False], weights=[5.0, 1.0], lam=0.5, B=4096)
NETS = {"c2": C2, "three": THREE, "conv": CONV}


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _p0(net, seed):
    rng = np.random.default_rng(seed)
    flat = O.flatten_params(net["archs"], O.init_params(net["archs"], rng)).astype(np.float32)
    off = 0
    for na in net["archs"]:                    # non-zero biases
        for _, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            if len(shp) == 1:
                flat[off:off + n] = 0.05 * rng.standard_normal(n)
            off += n
    return flat


def _model(V, net, dtype, act, p0, seed=11):
    m = V.AssocVariationalAutoEncoder(net["archs"], binary=net["binary"], transfer_fct=act, weights=net["weights"],
                                      assoc_lambda=net["lam"], learning_rate=1e-3, batch_size=net["B"], compute_dtype=dtype,
                                      seed=seed)
    m.set_params(p0)
    return m


def _data(net, seed, steps=1):
    rng = np.random.default_rng(seed)
    B, M = net["B"] * steps, len(net["archs"])
    X = synth_batch(rng, B, [na["n_input"] for na in net["archs"]], net["binary"])
    eps = rng.standard_normal((B, net["archs"][0]["n_z"])).astype(np.float32)
    return rng, X, eps


def _masks(rng, B, M):
    """mask variants: random with an empty row, a full row and every single-modality pattern; the last modality absent on every
    row; a single present row"""
    a = rng.random((B, M)) < 0.6
    a[0] = False
    a[1] = True
    for m in range(M):
        a[2 + m] = False
        a[2 + m, m] = True
    b = rng.random((B, M)) < 0.7
    b[:, M - 1] = False
    c = np.zeros((B, M), bool)
    c[5] = True
    return {"random": a, "absent_col": b, "one_row": c}


def _state(m):
    mm, vv, st = m.get_opt_state()
    return m.get_params(), mm, vv, st, m.get_grads()


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    for x, y, what in zip(sa, sb, ("params", "adam m", "adam v", "step", "grads")):
        assert np.array_equal(x, y), what


def _slices(archs):
    out, off = [], 0
    for na in archs:
        n = sum(int(np.prod(s)) for _, s in O.layer_shapes(na))
        out.append(slice(off, off + n))
        off += n
    return out


def _rel_errs(archs, got, ref):
    out, off = [], 0
    for m, na in enumerate(archs):
        for name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            a, b = got[off:off + n], ref[off:off + n]
            out.append(("m%d.%s" % (m, name), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))))
            off += n
    return out


def check_all_present_bitwise(V, net, dtype, act, steps=3):
    """masked steps with an all-present mask on one handle == unmasked steps on a twin handle: caller eps, then internal eps"""
    p0 = _p0(net, 3)
    a, b = _model(V, net, dtype, act, p0), _model(V, net, dtype, act, p0)
    _, X, eps = _data(net, 4, steps)
    B, M = net["B"], len(net["archs"])
    ones = np.ones((B, M), bool)
    for s in range(steps):
        Xs = [x[s * B:(s + 1) * B] for x in X]
        ca = a.partial_fit(Xs, eps[s * B:(s + 1) * B], present=ones)
        cb = b.partial_fit(Xs, eps[s * B:(s + 1) * B])
        assert ca == cb, (s, ca, cb)
    _same_state(a, b)
    for s in range(steps):                      # internal eps: keyed by (seed, step, row) alike
        Xs = [x[s * B:(s + 1) * B] for x in X]
        assert a.partial_fit(Xs, present=ones) == b.partial_fit(Xs), s
    _same_state(a, b)
    Xs = [x[:B] for x in X]
    assert a.evaluate_cost(Xs, eps[:B], present=ones) == b.evaluate_cost(Xs, eps[:B])
    assert a.evaluate_cost(Xs, present=ones) == b.evaluate_cost(Xs)        # the same draw counter
    _same_state(a, b)
    return a, b


def check_against_reference(V, net, dtype, act, variants=None, seed=7, extra=None):
    """one masked step per mask variant on a fresh handle: cost, every gradient tensor and the Adam update against the reference.
    ``extra``: {name: [B, M] mask}, further variants of the caller's"""
    fp32 = dtype == "fp32"
    p0 = _p0(net, seed)
    rng, X, eps = _data(net, seed + 1)
    B, M, archs = net["B"], len(net["archs"]), net["archs"]
    sl = _slices(archs)
    for name, P in dict(_masks(rng, B, M), **(extra or {})).items():
        if variants and name not in variants:
            continue
        m = _model(V, net, dtype, act, p0)
        c = m.partial_fit(X, eps, present=P)
        g = m.get_grads().astype(np.float64)
        masks = hip_relu_masks(m, archs) if act == "relu" and not any(na.get("hidden_conv") for na in archs) else None
        c_ref, g_ref = masked_cost_and_grads(archs, p0, X, eps, P, net["binary"], net["weights"], net["lam"], act,
                                             quant=None if fp32 else "bf16", masks=masks)
        ctol, gtol = (1e-5, 1e-4) if fp32 else (5e-5, 3e-3)
        assert abs(c - c_ref) <= ctol * max(abs(c_ref), 1e-3), (name, c, c_ref)
        live = [k for k in range(M) if P[:, k].any()]
        bad = [(n, e) for n, e in _rel_errs(archs, g, g_ref) if e > gtol and int(n[1]) in live]
        assert not bad, (name, bad)
        th1, _, _ = O.adam_step(p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size), g, 1, 1e-3)
        assert np.all(np.abs(m.get_params() - th1) <= 6e-8 * np.maximum(1.0, np.abs(th1))), name
        for k in range(M):
            if not P[:, k].any():               # fresh Adam state: exact zeros in, bitwise unchanged parameters out
                assert np.all(g[sl[k]] == 0), (name, k)
                assert np.array_equal(m.get_params()[sl[k]], p0[sl[k]]), (name, k)
        assert shadow_err(m)[:2] == (0.0, 0.0)
        del m


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_all_present_mask_is_the_unmasked_step(V, net, dtype, act):
    check_all_present_bitwise(V, NETS[net], dtype, act)


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_step_against_reference(V, net, dtype):
    check_against_reference(V, NETS[net], dtype, "softplus" if net == "conv" else "relu")


@pytest.mark.parametrize("env", [{}, {"AVAE_NO_LOSS8": "1"}])
def test_big_net_loss_tiles(V, monkeypatch, env):
    """256x64 8-wave loss tiles + the latent launch of its own (default), and the 128x128 4-wave route (AVAE_NO_LOSS8)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_all_present_bitwise(V, BIG, "bf16", "softplus", steps=1)
    check_against_reference(V, BIG, "fp32", "softplus", variants=("random",))


@pytest.mark.parametrize("env", [{"AVAE_NO_LEAN": "1"}, {"AVAE_NO_LEAN_LOSS": "1"}, {"AVAE_NO_TAIL": "1"}, {"AVAE_NO_32": "1"},
                                 {"AVAE_NO_32x32": "1"}, {"AVAE_NO_LEAN_HEAD": "1"}, {"AVAE_CHAIN2": "1"}])
def test_planner_switches_honour_the_mask(V, monkeypatch, env):
    """every route that moves the loss or latent item to another kernel honours the mask (or would refuse the call)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_all_present_bitwise(V, C2, "bf16", "relu", steps=2)
    check_against_reference(V, C2, "bf16", "relu", variants=("random",))
    check_against_reference(V, THREE, "fp32", "relu", variants=("absent_col",))


@pytest.mark.parametrize("net", ["three", "conv"])
def test_absent_content_is_never_read(V, net):
    net = NETS[net]
    p0 = _p0(net, 21)
    rng, X, eps = _data(net, 22, 2)
    B, M = net["B"], len(net["archs"])
    P = rng.random((2 * B, M)) < 0.6
    P[:, M - 1] = False
    runs = []
    for fill in ("nan", "inf", "big", "zeros", "none"):
        Xf = [x.copy() for x in X]
        for k in range(M):
            bad = {"nan": np.nan, "inf": np.inf if k % 2 else -np.inf, "big": 1e30, "zeros": 0.0, "none": 0.0}[fill]
            Xf[k][~P[:, k]] = bad
        if fill == "none":
            Xf[M - 1] = None
        m = _model(V, net, "bf16", "relu", p0)
        costs = [m.partial_fit([x[:B] if x is not None else None for x in Xf], eps[:B], present=P[:B]),
                 m.partial_fit_steps([x[B:] if x is not None else None for x in Xf], 1, eps[B:], present=P[B:]),
                 m.evaluate_cost([x[:B] if x is not None else None for x in Xf], eps[:B], present=P[:B])]
        runs.append((fill, costs, _state(m)))
        del m
    for fill, costs, st in runs[1:]:
        assert costs == runs[0][1], fill
        for x, y in zip(st, runs[0][2]):
            assert np.array_equal(x, y), fill
    assert all(np.isfinite(runs[0][1]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_eval_is_the_per_row_formula(V, dtype):
    net = THREE
    p0 = _p0(net, 31)
    rng, X, eps = _data(net, 32)
    B, M = net["B"], len(net["archs"])
    m = _model(V, net, dtype, "relu", p0)
    P = _masks(rng, B, M)["random"]
    m.partial_fit(X, eps, present=P)
    m.partial_fit(X, present=P)
    assert shadow_err(m)[:2] == (0.0, 0.0)
    before, hist = _state(m), m.cost_history(2)
    c = m.evaluate_cost(X, eps, present=P)
    sc = m.score_samples(X, eps)
    want = masked_cost_from_rows(sc["recon"], sc["latent"], sc["assoc"], P, net["binary"], net["weights"], net["lam"], B)
    assert abs(c - want) <= 1e-5 * abs(want), (c, want)
    for x, y in zip(_state(m), before):
        assert np.array_equal(x, y)
    assert np.array_equal(m.cost_history(2), hist)
    m.evaluate_cost(X, present=P)               # internal eps
    assert _state(m)[3] == before[3]


@pytest.mark.parametrize("net", ["c2", "conv"])
def test_multi_step_replay_is_single_steps(V, net):
    net = NETS[net]
    p0 = _p0(net, 41)
    rng, X, eps = _data(net, 42, 20)
    B, M = net["B"], len(net["archs"])
    P = rng.random((20 * B, M)) < 0.6
    a, b = _model(V, net, "bf16", "relu", p0), _model(V, net, "bf16", "relu", p0)
    a.partial_fit_steps(X, 20, eps, present=P)                 # one 16-step and one 4-step replay
    costs = [b.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B], present=P[i * B:(i + 1) * B]) for i in range(20)]
    _same_state(a, b)
    assert np.array_equal(a.cost_history(20), np.asarray(costs, np.float32))
    a.partial_fit_steps(X, 20, present=P)                      # internal eps
    for i in range(20):
        b.partial_fit([x[i * B:(i + 1) * B] for x in X], present=P[i * B:(i + 1) * B])
    _same_state(a, b)


def test_interleaved_masked_and_unmasked_steps_follow_the_reference(V):
    net = THREE
    p0 = _p0(net, 51)
    rng, X, eps = _data(net, 52, 4)
    B, M, archs = net["B"], len(net["archs"]), net["archs"]
    m = _model(V, net, "fp32", "softplus", p0)
    ref = O.OracleAssocVAE(archs, net["binary"], "softplus", net["weights"], net["lam"], 1e-3, B, params_flat=p0.astype(np.float64))
    for s, masked in enumerate((True, False, True, False)):
        Xs, es = [x[s * B:(s + 1) * B] for x in X], eps[s * B:(s + 1) * B]
        if masked:
            P = _masks(rng, B, M)["random"]
            c = m.partial_fit(Xs, es, present=P)
            c_ref, g_ref = masked_cost_and_grads(archs, ref.get_params(), Xs, es, P, net["binary"], net["weights"], net["lam"], "softplus")
        else:
            c = m.partial_fit(Xs, es)
            c_ref, g_ref, _ = ref.cost_and_grads(Xs, es)
        ref.apply_gradients(g_ref)
        # (later steps start from weights that differ in the Adam-ill-conditioned elements: test_gpu_parity's 2e-5)
        assert abs(c - c_ref) <= (1e-5 if s == 0 else 2e-5) * abs(c_ref), (s, c, c_ref)
        assert m.cost_history(1)[0] == np.float32(c)
    assert m.get_opt_state()[2] == 4


def test_masked_call_errors(V):
    net = THREE
    p0 = _p0(net, 61)
    _, X, eps = _data(net, 62)
    B, M = net["B"], len(net["archs"])
    m = _model(V, net, "fp32", "relu", p0)
    for bad in (np.ones((B + 1, M), bool), np.ones((B, M - 1), bool), np.ones((B,), bool)):
        with pytest.raises(ValueError):
            m.partial_fit(X, eps, present=bad)
        with pytest.raises(ValueError):
            m.evaluate_cost(X, eps, present=bad)
    with pytest.raises(ValueError):
        m.partial_fit_steps(X, 2, present=np.ones((B, M), bool))
    # NULL present_dev straight through the C ABI: an error with a message, not a fault
    ts = [torch.as_tensor(x).cuda() for x in X]
    ptrs = (C.c_void_p * M)(*[t.data_ptr() for t in ts])
    cost = C.c_float(0.0)
    for rc in (m._L.avae_train_steps_masked(m._h, 1, ptrs, None, None, None, C.byref(cost), m._stream()),
               m._L.avae_eval_cost_masked(m._h, ptrs, None, None, None, C.byref(cost), m._stream())):
        assert rc != 0 and b"present_dev" in m._L.avae_last_error(m._h)
    assert m.get_opt_state()[2] == 0
    # a data-parallel model: refused in Python whatever the comm route, and in the library (one-rank communicator)
    real = m._sync
    m._sync = types.SimpleNamespace(world_size=2)
    with pytest.raises(RuntimeError, match="one replica"):
        m.partial_fit(X, eps, present=np.ones((B, M), bool))
    m._sync = real
    dp = V.AssocVariationalAutoEncoder(net["archs"], binary=net["binary"], transfer_fct="relu", weights=net["weights"],
                                       assoc_lambda=net["lam"], batch_size=B, compute_dtype="fp32", comm="ipc")
    with pytest.raises(RuntimeError, match="one replica"):
        dp.partial_fit(X, eps, present=np.ones((B, M), bool))
    with pytest.raises(RuntimeError, match="one replica"):
        dp.evaluate_cost(X, eps, present=np.ones((B, M), bool))
