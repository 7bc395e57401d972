"""Denoising training on a real MI355X (include/avae.h: avae_set_corruption, avae_train_steps_in, avae_eval_cost_in,
avae_stage_batches_in): the encoders read a corrupted copy of the batch -- the caller's ``inputs`` or the
on-device Philox corruption -- while every loss term is charged against the clean batch.

Shapes: image 784-24-16 and joint 147-20-12, n_z 6; B = 80 is two 64-row tiles, the second ragged, 147 = 36 quads + 3; ``X`` and
``inputs`` are column views of two [rows, 931] matrices, so every source is strided and unaligned.  Tolerances are the project's
plain ones (tests/test_gpu_parity.py): fp32 against the fp64 reference of tests/denoise_reference.py 1e-5
for the cost and 1e-4 of each tensor's maximum for the gradients, bf16 against the reference run with quant='bf16' and the
kernels' relu decisions 5e-5 and 3e-3.  The staged normals are held to the internal eps test's 2e-4 (the hardware sin / cos)."""
import ctypes as C
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import hip_relu_masks, make_arch, shadow_err, synth_batch
from denoise_reference import corrupt, denoise_cost_and_grads
from oracle import vae_assoc_oracle as O

pytestmark = pytest.mark.gpu

NET = dict(archs=[make_arch("image", 784, 24, 16, 6), make_arch("joint", 147, 20, 12, 6)], binary=[True, False],
           weights=[5.0, 1.0], lam=0.5)
CONV = dict(archs=[dict(make_arch("image", 784, 8, 24, 6), hidden_conv=True, n_hidden_gener_1=24, n_hidden_gener_2=8),
                   make_arch("joint", 147, 40, 30, 6)], binary=[True, False], weights=[5.0, 1.0], lam=0.5)
SEED = 11
CORR = dict(drop=[0.3, 0.1], noise=[0.0, 0.5], drop_value=[0.0, -1.0])
TOL = {"fp32": (1e-5, 1e-4), "bf16": (5e-5, 3e-3)}


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _p0(net, seed=3):
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


def _model(V, net, B, dtype, act="relu", corruption=None, p0=None, **kw):
    m = V.AssocVariationalAutoEncoder(net["archs"], binary=net["binary"], transfer_fct=act, weights=net["weights"],
                                      assoc_lambda=net["lam"], learning_rate=1e-3, batch_size=B, compute_dtype=dtype, seed=SEED,
                                      corruption=corruption, **kw)
    m.set_params(_p0(net) if p0 is None else p0)
    return m


class Data:
    """``rows`` rows of clean data and of explicit corrupted inputs (30 % of the image dropped, sigma 0.5 on the joint, drawn on
    the host with the reference's stream under another seed), each ONE [rows, 931] device matrix: ``X`` / ``IN`` are its column
    views, ``x`` / ``xin`` the NumPy copies, ``eps`` [rows, 6]."""

    def __init__(self, rows, seed):
        rng = np.random.default_rng(seed)
        self.x = synth_batch(rng, rows, [784, 147], [True, False])
        self.xin = [corrupt(self.x[0], 99, seed, 0, drop=0.3)[0].astype(np.float32),
                    corrupt(self.x[1], 99, seed, 1, noise=0.5)[0].astype(np.float32)]
        self.eps = rng.standard_normal((rows, 6)).astype(np.float32)
        self.wide = torch.as_tensor(np.concatenate(self.x, axis=1)).cuda()
        self.wide_in = torch.as_tensor(np.concatenate(self.xin, axis=1)).cuda()
        self.X = [self.wide[:, :784], self.wide[:, 784:]]
        self.IN = [self.wide_in[:, :784], self.wide_in[:, 784:]]
        assert self.X[1].stride(0) == 931 and self.X[0][1:].data_ptr() % 16 != 0      # strided; rows 1.. not 16-byte aligned

    def at(self, s, B):
        """batch s: (X views, IN views, x, xin, eps)"""
        r = slice(s * B, (s + 1) * B)
        return [t[r] for t in self.X], [t[r] for t in self.IN], [a[r] for a in self.x], [a[r] for a in self.xin], self.eps[r]


def fetch(m, name, shape):
    buf = np.empty(int(np.prod(shape)), dtype=np.float32)
    cnt = C.c_size_t(0)
    rc = m._L.avae_debug_fetch(m._h, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt))
    assert rc == 0 and cnt.value == buf.size, m._L.avae_last_error(m._h)
    return buf.reshape(shape)


def staged(m, B):
    """([X0, X1], [T0, T1]) of staging set 0"""
    return [fetch(m, "X%d" % k, (B, w)) for k, w in enumerate((784, 147))], [fetch(m, "T%d" % k, (B, w)) for k, w in enumerate((784, 147))]


def _state(m):
    mm, vv, st = m.get_opt_state()
    return m.get_params(), mm, vv, st, m.get_grads()


def _same_state(a, b):
    for x, y, what in zip(_state(a), _state(b), ("params", "adam m", "adam v", "step", "grads")):
        assert np.array_equal(x, y), what


def _rel_errs(archs, got, ref):
    out, off = [], 0
    for m, na in enumerate(archs):
        for name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            a, b = got[off:off + n], ref[off:off + n]
            out.append(("m%d.%s" % (m, name), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))))
            off += n
    return out


def check_step(m, net, dtype, act, p, c, x, xin, eps, present=None, tag=""):
    """cost ``c`` and the gradient of the step ``m`` just ran from parameters ``p`` against the reference"""
    archs = net["archs"]
    mlp = not any(na.get("hidden_conv") for na in archs)
    masks = hip_relu_masks(m, archs) if act == "relu" and mlp else None
    c_ref, g_ref = denoise_cost_and_grads(archs, p, x, xin, eps, net["binary"], net["weights"], net["lam"], act, present=present,
                                          quant=None if dtype == "fp32" else "bf16", masks=masks)
    ctol, gtol = TOL[dtype]
    errs = _rel_errs(archs, m.get_grads().astype(np.float64), g_ref)
    print("%s %s: cost rel %.2e, worst gradient tensor %.2e" % (tag, dtype, abs(c - c_ref) / abs(c_ref), max(e for _, e in errs)))
    assert abs(c - c_ref) <= ctol * abs(c_ref), (tag, c, c_ref)
    bad = [(n, e) for n, e in errs if e > gtol]
    assert not bad, (tag, bad)
    assert shadow_err(m)[:2] == (0.0, 0.0)
    return c_ref


# ------------------------------------------------------------------------------------------------ 1. explicit inputs
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("net,B,act", [("mlp", 80, "relu"), ("conv", 16, "softplus")])
def test_explicit_inputs_against_reference(V, dtype, net, B, act):
    """three steps, the reference restarted from the kernels' weights before each; then evaluate_cost(inputs=).  (The conv model
    runs softplus: its stored conv activations have no relu decisions to hand over.)"""
    net = NET if net == "mlp" else CONV
    m = _model(V, net, B, dtype, act)
    d = Data(3 * B, 21)
    for s in range(3):
        X, IN, x, xin, eps = d.at(s, B)
        p = m.get_params()
        c = m.partial_fit(X, eps, inputs=IN)
        check_step(m, net, dtype, act, p, c, x, xin, eps, tag="step %d" % s)
        if s == 0:      # a step that staged one array into both copies is another step: its gradient is far outside the tolerance
            _, g_plain = denoise_cost_and_grads(net["archs"], p, x, x, eps, net["binary"], net["weights"], net["lam"], act)
            assert max(e for _, e in _rel_errs(net["archs"], m.get_grads().astype(np.float64), g_plain)) > 10 * TOL[dtype][1]
    X, IN, x, xin, eps = d.at(0, B)
    p, before = m.get_params(), _state(m)
    c_ref, _ = denoise_cost_and_grads(net["archs"], p, x, xin, eps, net["binary"], net["weights"], net["lam"], act,
                                      quant=None if dtype == "fp32" else "bf16")
    c = m.evaluate_cost(X, eps, inputs=IN)
    assert abs(c - c_ref) <= TOL[dtype][0] * abs(c_ref), (c, c_ref)
    for a, b in zip(_state(m), before):
        assert np.array_equal(a, b)
    # one modality with an explicit input, the other without: the other's encoder reads the clean rows
    c = m.evaluate_cost(X, eps, inputs=[None, IN[1]])
    c_ref, _ = denoise_cost_and_grads(net["archs"], p, x, [x[0], xin[1]], eps, net["binary"], net["weights"], net["lam"], act,
                                      quant=None if dtype == "fp32" else "bf16")
    assert abs(c - c_ref) <= TOL[dtype][0] * abs(c_ref), (c, c_ref)


# ------------------------------------------------------------------------------------------------ 2. on-device corruption
def test_on_device_corruption_is_the_documented_stream(V):
    B = 80
    d = Data(2 * B, 22)
    f32, b16 = _model(V, NET, B, "fp32", corruption=CORR), _model(V, NET, B, "bf16", corruption=CORR)
    for s in range(2):                                   # step 0 and step 1: the step counter keys the draw
        X, _, x, _, eps = d.at(s, B)
        p32, p16 = f32.get_params(), b16.get_params()
        c32, c16 = f32.partial_fit(X, eps), b16.partial_fit(X, eps)
        xs, ts = staged(f32, B)
        for k in range(2):
            assert np.array_equal(ts[k], x[k]), "T%d is the exact target" % k
            want, dropped = corrupt(x[k], SEED, s, k, CORR["drop"][k], CORR["noise"][k], CORR["drop_value"][k])
            assert 0.5 * CORR["drop"][k] < dropped.mean() < 1.5 * CORR["drop"][k]
            assert np.all(xs[k][dropped] == np.float32(CORR["drop_value"][k])), "dropped elements are exactly drop_value"
            err = np.abs(xs[k][~dropped] - want[~dropped]).max()
            print("step %d modality %d: kept elements off by %.2e (sigma %.1f)" % (s, k, err, CORR["noise"][k]))
            assert err <= 2e-4 * CORR["noise"][k]
        x16, t16 = staged(b16, B)
        for k in range(2):
            assert np.array_equal(t16[k], x[k])
            assert np.array_equal(x16[k], O.bf16_round(xs[k]).astype(np.float32)), "the bf16 copy is the fp32 x~ rounded once"
        check_step(f32, NET, "fp32", "relu", p32, c32, x, xs, eps, tag="corrupted step %d" % s)
        check_step(b16, NET, "bf16", "relu", p16, c16, x, x16, eps, tag="corrupted step %d" % s)


def test_zero_parameters_leave_a_modality_alone_and_inputs_win(V):
    B = 20
    d = Data(B, 23)
    X, IN, x, xin, eps = d.at(0, B)
    m = _model(V, NET, B, "fp32", corruption=dict(drop=[0.3, 0.0], noise=0.0, drop_value=[0.5, 7.0]))
    m.partial_fit(X, eps)
    xs, ts = staged(m, B)
    assert np.array_equal(xs[1].view(np.uint32), ts[1].view(np.uint32)) and np.array_equal(ts[1], x[1])
    assert np.all(xs[0][corrupt(x[0], SEED, 0, 0, 0.3)[1]] == 0.5)
    m.set_corruption(**CORR)
    m.partial_fit(X, eps, inputs=[None, IN[1]])          # step 1: modality 0 corrupted on the device, modality 1 explicit
    xs, ts = staged(m, B)
    assert np.array_equal(xs[1], xin[1]) and np.array_equal(ts[1], x[1])
    assert np.array_equal(xs[0], corrupt(x[0], SEED, 1, 0, 0.3)[0].astype(np.float32)) and np.array_equal(ts[0], x[0])
    # a NaN under a drop does not reach the encoder's copy; it reaches the target
    xn = d.wide.clone()
    where = corrupt(x[0], SEED, 2, 0, 0.3)[1]
    r, c = np.argwhere(where)[0]
    xn[r, c] = float("nan")
    m.partial_fit([xn[:, :784], xn[:, 784:]], eps, return_cost=False)
    xs, ts = staged(m, B)
    assert xs[0][r, c] == 0.0 and np.isnan(ts[0][r, c]) and np.isfinite(xs[0]).all()


# ------------------------------------------------------------------------------------------------ 3. twin
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_corrupted_steps_equal_a_twin_fed_the_staged_inputs(V, dtype):
    B = 80
    d = Data(3 * B, 24)
    a, b = _model(V, NET, B, dtype, corruption=CORR), _model(V, NET, B, dtype)
    for s in range(3):
        X, _, _, _, eps = d.at(s, B)
        ca = a.partial_fit(X, eps)
        cb = b.partial_fit(X, eps, inputs=staged(a, B)[0])
        assert ca == cb, (s, ca, cb)
    _same_state(a, b)


# ------------------------------------------------------------------------------------------------ 4. replay
@pytest.mark.parametrize("how", ["corruption", "inputs"])
def test_replays_are_single_steps(V, how):
    """21 steps = one 16-step replay, one 4-step replay and one single step"""
    B, n = 20, 21
    d = Data(n * B, 25)
    corr = CORR if how == "corruption" else None
    a, b = _model(V, NET, B, "bf16", corruption=corr), _model(V, NET, B, "bf16", corruption=corr)
    a.partial_fit_steps(d.X, n, d.eps, inputs=d.IN if how == "inputs" else None)
    costs = []
    for s in range(n):
        X, IN, _, _, eps = d.at(s, B)
        costs.append(b.partial_fit(X, eps, inputs=IN if how == "inputs" else None))
    _same_state(a, b)
    assert np.array_equal(a.cost_history(n), np.asarray(costs, np.float32))
    if how == "corruption":                              # (and the run did corrupt)
        c = _model(V, NET, B, "bf16")
        c.partial_fit_steps(d.X, n, d.eps)
        assert not np.array_equal(c.get_params(), a.get_params())


# ------------------------------------------------------------------------------------------------ 5. off is off
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_off_is_off(V, dtype):
    B = 20
    d = Data(3 * B, 26)
    plain = _model(V, NET, B, dtype)
    off = {"none": _model(V, NET, B, dtype), "zeros": _model(V, NET, B, dtype), "was_on": _model(V, NET, B, dtype, corruption=CORR),
           "inputs_none": _model(V, NET, B, dtype), "capi": _model(V, NET, B, dtype)}
    off["none"].set_corruption(None)
    off["zeros"].set_corruption(0.0, 0.0, drop_value=3.0)
    off["was_on"].set_corruption(None)
    for s in range(3):
        X, _, _, _, eps = d.at(s, B)
        c = plain.partial_fit(X, eps)
        for name, m in off.items():
            if name == "capi":       # the _in call with every optional argument NULL, straight through the C ABI
                e = torch.as_tensor(eps).cuda()
                ptrs, lds = (C.c_void_p * 2)(*[t.data_ptr() for t in X]), (C.c_int32 * 2)(931, 931)
                cost = C.c_float(0.0)
                rc = m._L.avae_train_steps_in(m._h, 1, ptrs, lds, None, None, None, e.data_ptr(), C.byref(cost), m._stream())
                assert rc == 0, m._L.avae_last_error(m._h)
                assert cost.value == c, name
            else:
                assert m.partial_fit(X, eps, inputs=None if name != "inputs_none" else [None, None]) == c, (name, s)
    for name, m in off.items():
        _same_state(m, plain)
    # evaluation never corrupts: a handle with a corruption set evaluates what a plain one does, caller's eps and internal draw
    X, _, _, _, eps = d.at(0, B)
    on = _model(V, NET, B, dtype, corruption=CORR, p0=plain.get_params())
    ref = _model(V, NET, B, dtype, p0=plain.get_params())
    assert on.evaluate_cost(X, eps) == ref.evaluate_cost(X, eps)
    assert on.evaluate_cost(X) == ref.evaluate_cost(X)
    mask = np.ones((B, 2), bool)
    assert on.evaluate_cost(X, eps, present=mask) == ref.evaluate_cost(X, eps, present=mask)
    assert np.array_equal(on.transform(X)[0].cpu().numpy(), ref.transform(X)[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------ 6. masked
def _mask(rng, B):
    p = rng.random((B, 2)) < 0.6
    p[0], p[1], p[2], p[3] = False, True, (True, False), (False, True)
    return p


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_denoising_steps(V, dtype):
    B = 80
    d = Data(B, 27)
    X, IN, x, xin, eps = d.at(0, B)
    rng = np.random.default_rng(5)
    ones, P = np.ones((B, 2), bool), _mask(rng, B)
    # an all-present mask is the unmasked corrupted step, bit for bit (on-device corruption, then explicit inputs)
    a, b = _model(V, NET, B, dtype, corruption=CORR), _model(V, NET, B, dtype, corruption=CORR)
    assert a.partial_fit(X, eps, present=ones) == b.partial_fit(X, eps)
    assert a.partial_fit(X, eps, present=ones, inputs=IN) == b.partial_fit(X, eps, inputs=IN)
    assert a.evaluate_cost(X, eps, present=ones, inputs=IN) == b.evaluate_cost(X, eps, inputs=IN)
    _same_state(a, b)
    # explicit inputs under a random mask: parity, zeros where absent, and absent content of X and inputs is never read
    m = _model(V, NET, B, dtype)
    p = m.get_params()
    c = m.partial_fit(X, eps, present=P, inputs=IN)
    xs, ts = staged(m, B)
    for k in range(2):
        assert not xs[k][~P[:, k]].any() and not ts[k][~P[:, k]].any()
        assert np.array_equal(ts[k][P[:, k]], x[k][P[:, k]])
    check_step(m, NET, dtype, "relu", p, c, x, xin, eps, present=P, tag="masked explicit")
    wn, wn_in = d.wide.clone(), d.wide_in.clone()
    for k, cols in enumerate((slice(0, 784), slice(784, 931))):
        gone = torch.as_tensor(~P[:, k]).cuda()
        wn[:, cols][gone] = float("nan")
        wn_in[:, cols][gone] = float("nan")
    n = _model(V, NET, B, dtype)
    assert n.partial_fit([wn[:, :784], wn[:, 784:]], eps, present=P, inputs=[wn_in[:, :784], wn_in[:, 784:]]) == c
    _same_state(n, m)
    # on-device corruption under the mask: the staged rows are the unmasked draw where present, and the step follows them
    k_ = _model(V, NET, B, dtype, corruption=CORR)
    p = k_.get_params()
    c = k_.partial_fit(X, eps, present=P)
    xs, ts = staged(k_, B)
    full = staged(_step(_model(V, NET, B, dtype, corruption=CORR), X, eps), B)[0]
    for k in range(2):
        assert np.array_equal(xs[k][P[:, k]], full[k][P[:, k]]) and not xs[k][~P[:, k]].any() and not ts[k][~P[:, k]].any()
    check_step(k_, NET, dtype, "relu", p, c, x, xs, eps, present=P, tag="masked corrupted")


def _step(m, X, eps):
    m.partial_fit(X, eps, return_cost=False)
    return m


# ------------------------------------------------------------------------------------------------ 7. shards
def test_a_shard_stages_its_rows_of_the_global_draw(V):
    from vae_assoc_amd import _capi
    d = Data(80, 28)
    full = _model(V, NET, 80, "fp32", corruption=CORR)
    half = _model(V, NET, 40, "fp32")
    half._L.avae_destroy(half._h)
    half._cfg.row_offset, half._cfg.batch_global = 40, 80
    h = C.c_void_p()
    _capi.check(None, half._L.avae_create(C.byref(half._cfg), C.byref(h)), "avae_create")
    half._h = h
    half.set_params(full.get_params())
    half.set_corruption(**CORR)
    for s in range(2):
        full.partial_fit(d.X, d.eps, return_cost=False)
        half.partial_fit([t[40:] for t in d.X], d.eps[40:], return_cost=False)
        for k, w in enumerate((784, 147)):
            assert np.array_equal(fetch(half, "X%d" % k, (40, w)), fetch(full, "X%d" % k, (80, w))[40:]), (s, k)
            assert np.array_equal(fetch(half, "T%d" % k, (40, w)), d.x[k][40:])


B_LOC, WORLD, STEPS = 32, 2, 3


def _dp_data():
    rng = np.random.default_rng(17)
    X = synth_batch(rng, B_LOC * WORLD, [784, 147], [True, False])
    eps = rng.standard_normal((STEPS, B_LOC * WORLD, 6)).astype(np.float32)
    return X, eps


def _dp_model(B, **kw):
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    return AssocVariationalAutoEncoder(NET["archs"], binary=NET["binary"], transfer_fct="relu", weights=NET["weights"],
                                       assoc_lambda=NET["lam"], batch_size=B, compute_dtype="fp32", device=0, seed=SEED,
                                       corruption=CORR, **kw)


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        import __graft_entry__ as g
        g.build()
        X, eps = _dp_data()
        m = _dp_model(B_LOC, data_parallel=True)
        lo, hi = rank * B_LOC, (rank + 1) * B_LOC
        costs = [m.partial_fit([x[lo:hi] for x in X], eps[s][lo:hi]) for s in range(STEPS)]
        staged0 = fetch(m, "X0", (B_LOC, 784))
        # the same steps as one staged run (avae_stage_batches(n)): bitwise the same
        m2 = _dp_model(B_LOC, data_parallel=True)
        last = m2.partial_fit_steps([np.concatenate([x[lo:hi]] * STEPS) for x in X], STEPS, np.concatenate([eps[s][lo:hi] for s in range(STEPS)]))
        assert last == costs[-1] and np.array_equal(m2.get_params(), m.get_params())
        np.savez(os.path.join(out_dir, "r%d.npz" % rank), costs=np.array(costs), params=m.get_params(), staged0=staged0)
    finally:
        dist.destroy_process_group()


def test_two_replicas_with_corruption_track_the_global_batch(V, tmp_path):
    """two gloo ranks on the one GPU (the pattern and tolerances of tests/test_gpu_dataparallel.py), corruption on"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)
    X, eps = _dp_data()
    full = _dp_model(B_LOC * WORLD)
    ref_costs = [full.partial_fit(X, eps[s]) for s in range(STEPS)]
    r = [np.load(os.path.join(str(tmp_path), "r%d.npz" % k)) for k in range(WORLD)]
    assert np.array_equal(r[0]["params"], r[1]["params"]) and np.array_equal(r[0]["costs"], r[1]["costs"])
    want = fetch(full, "X0", (B_LOC * WORLD, 784))       # the last step's staged image rows: each rank drew its own rows of them
    assert np.array_equal(np.concatenate([r[0]["staged0"], r[1]["staged0"]]), want)
    assert np.allclose(r[0]["costs"], ref_costs, rtol=1e-5)
    assert np.abs(r[0]["params"] - full.get_params()).max() <= 2e-4
    plain = _dp_model(B_LOC * WORLD)
    plain.set_corruption(None)
    assert abs(plain.partial_fit(X, eps[0]) - ref_costs[0]) > 1e-3 * abs(ref_costs[0])     # (and the runs did corrupt)


def test_one_rank_library_pipeline_is_the_plain_corrupted_step(V):
    """comm='ipc' with one rank (the library-owned bucketed pipeline and its captured 16- and 4-step graphs): 3 single steps and
    a run of 21 are bitwise the plain corrupted run's"""
    B, n = 20, 21
    d = Data((3 + n) * B, 29)
    a, b = _model(V, NET, B, "bf16", corruption=CORR, comm="ipc"), _model(V, NET, B, "bf16", corruption=CORR)
    for s in range(3):
        X, _, _, _, eps = d.at(s, B)
        assert a.partial_fit(X, eps) == b.partial_fit(X, eps), s
    rest = slice(3 * B, None)
    for m in (a, b):
        m.partial_fit_steps([t[rest] for t in d.X], n, d.eps[rest], inputs=[None, d.IN[1][rest]])
    _same_state(a, b)
    assert np.array_equal(a.cost_history(n), b.cost_history(n))


# ------------------------------------------------------------------------------------------------ 8. errors
def test_denoise_call_errors(V):
    from vae_assoc_amd import _capi
    B = 20
    d = Data(B, 30)
    X, IN, _, _, eps = d.at(0, B)
    m = _model(V, NET, B, "fp32")
    L, h = m._L, m._h

    def corr(**kw):
        c = _capi.Corruption()
        for name, (k, v) in kw.items():
            getattr(c, name)[k] = v
        return c
    for c, needle in ((corr(drop_prob=(0, 1.0)), b"drop_prob"), (corr(drop_prob=(1, -0.25)), b"drop_prob"),
                      (corr(drop_prob=(0, float("nan"))), b"drop_prob"), (corr(noise_std=(1, -1.0)), b"noise_std"),
                      (corr(noise_std=(0, float("inf"))), b"noise_std"), (corr(drop_value=(1, float("nan"))), b"drop_value"),
                      (corr(drop_value=(0, float("inf"))), b"drop_value")):
        assert L.avae_set_corruption(h, C.byref(c)) != 0
        assert needle in L.avae_last_error(h), L.avae_last_error(h)
    ptrs, lds = (C.c_void_p * 2)(*[t.data_ptr() for t in X]), (C.c_int32 * 2)(931, 931)
    ins = (C.c_void_p * 2)(*[t.data_ptr() for t in IN])
    e, cost, st = torch.as_tensor(eps).cuda(), C.c_float(0.0), m._stream()
    short = (C.c_int32 * 2)(931, 146)
    for rc in (L.avae_train_steps_in(h, 1, ptrs, lds, ins, short, None, e.data_ptr(), C.byref(cost), st),
               L.avae_eval_cost_in(h, ptrs, lds, ins, short, None, e.data_ptr(), C.byref(cost), st),
               L.avae_stage_batches_in(h, 1, ptrs, lds, ins, short, e.data_ptr(), st)):
        assert rc != 0 and b"in_ld[1]" in L.avae_last_error(h), L.avae_last_error(h)
    no_x = (C.c_void_p * 2)(X[0].data_ptr(), None)
    pres = torch.ones((B, 2), dtype=torch.uint8).cuda()
    for rc in (L.avae_train_steps_in(h, 1, no_x, lds, ins, lds, pres.data_ptr(), e.data_ptr(), C.byref(cost), st),
               L.avae_eval_cost_in(h, no_x, lds, ins, lds, pres.data_ptr(), e.data_ptr(), C.byref(cost), st)):
        assert rc != 0 and b"in_dev[1]" in L.avae_last_error(h) and b"x_dev[1]" in L.avae_last_error(h), L.avae_last_error(h)
    assert L.avae_train_steps_in(h, 0, ptrs, lds, ins, lds, None, e.data_ptr(), C.byref(cost), st) != 0
    assert b"n_steps" in L.avae_last_error(h)
    # none of them moved the step counter or left a corruption behind: the next step is the plain one
    assert m.get_opt_state()[2] == 0
    ref = _model(V, NET, B, "fp32")
    assert m.partial_fit(X, eps) == ref.partial_fit(X, eps)
    # the Python surface raises ahead of the library
    with pytest.raises(ValueError, match="drop_prob"):
        m.set_corruption(drop=1.0)
    with pytest.raises(ValueError, match="noise_std"):
        m.set_corruption(noise=[0.1, -0.1])
    with pytest.raises(ValueError, match="rows"):
        m.partial_fit(X, eps, inputs=[IN[0][:B - 1], IN[1]])
    with pytest.raises(ValueError, match=r"inputs\[1\] is given while X\[1\] is None"):
        m.partial_fit([X[0], None], eps, present=np.ones((B, 2), bool), inputs=IN)
    assert m.get_opt_state()[2] == 1
    # present= on a data-parallel model is still refused, with or without inputs, in Python and in the library
    dp = _model(V, NET, B, "fp32", comm="ipc")
    with pytest.raises(RuntimeError, match="one replica"):
        dp.partial_fit(X, eps, present=np.ones((B, 2), bool), inputs=IN)
    with pytest.raises(RuntimeError, match="one replica"):
        dp.evaluate_cost(X, eps, present=np.ones((B, 2), bool), inputs=IN)
    real = m._sync
    m._sync = types.SimpleNamespace(world_size=2)
    with pytest.raises(RuntimeError, match="one replica"):
        m.partial_fit(X, eps, present=np.ones((B, 2), bool), inputs=IN)
    m._sync = real
    assert dp.get_opt_state()[2] == 0
