"""The big-net launches at ragged shapes, and the optimiser from crafted states (MI355X).

The 8-wave 256x128 NT/TN tiles (cfg 2), the 128x128 tiles (cfg 1), the 8-wave 256x64 loss tiles (cfg 6), the latent item's own
launch and the 64x128 head tiles (cfg 4) were only tested at batches of 2048 / 4096 and widths that are multiples of 128.  Here
every one of them runs with a ragged edge: a batch that leaves padding rows in the last 256-row tile (3999 = 15 x 256 + 159), widths
that are multiples of neither the tile nor 8 (1003, 605: the bf16 register epilogue's partial column group), fan-ins that are not
multiples of the K tile, and weight gradients whose K (= batch) is not a multiple of the K tile (333).  Each target is asserted
through the plan dump (plan_dump.step_plan), so a planner change that moves a shape off its target fails here instead of silently
testing something else.  Parity runs use a normal handle, at every step (check_step_parity with grad_every_step).

Adam from crafted states: a checkpoint's m, v and step are rewritten (m ~ N(0, 1) x (sqrt(v) + 1e-6), v log-uniform over
[1e-30, 1e2] with exact zeros, step t0 up to 2^31 + 3) and restored; every step is then checked against the kernel's arithmetic
(check_adam_step), a multi-step replay against single steps bitwise, and the cost ring across its wrap at 4096 entries."""
import numpy as np
import pytest
import torch

from conftest import make_arch, shadow_err, synth_batch
from oracle import vae_assoc_oracle as O
from plan_dump import K_DGRAD_HIDDEN, K_DGRAD_LATENT, K_FWD_HEAD, K_FWD_HIDDEN, K_FWD_OUT_LOSS, K_LATENT, step_plan
from test_gpu_parity import check_adam_step, check_step_parity, opt_snapshot, per_tensor_err

pytestmark = pytest.mark.gpu

# Set A: batch 3999 (97 padding rows in the last 256-row tile), n_z = 40 (2 n_z = 80 > 64: 64x128 head tiles)
B_A, NZ_A = 3999, 40
SET_A = [make_arch("a", 784, 0, 0, NZ_A, n_hidden=[1003, 605]), make_arch("b", 147, 0, 0, NZ_A, n_hidden=[1003, 640])]
# Set B: batch 333, wide layers -- the weight-gradient launch alone reaches the 8-wave TN tiles, with K = 333
B_B, NZ_B = 333, 20
SET_B = [make_arch("a", 784, 0, 0, NZ_B, n_hidden=[1500, 1000]), make_arch("b", 147, 0, 0, NZ_B, n_hidden=[1500, 1000])]
BIN = [True, False]


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _batch(archs, B, seed, n=1):
    rng = np.random.default_rng(seed)
    X = synth_batch(rng, n * B, [a["n_input"] for a in archs], BIN)
    eps = rng.standard_normal((n * B, archs[0]["n_z"])).astype(np.float32)
    return X, eps


def _wide_tn(archs, B):
    """(M, N, K) of the weight-gradient products that go to the wide launch (avae_host.hip: N > 64 and M > 64): every dense layer
    but the heads and the first decoder layer (M = n_z + 1)"""
    out = []
    for na in archs:
        for name, shp in O.layer_shapes(na):
            if len(shp) == 2 and name not in ("enc_Wmu", "enc_Wsig") and shp[0] + 1 > 64 and shp[1] > 64:
                out.append((int(shp[0]) + 1, int(shp[1]), B))
    return out


# ----------------------------------------------------------------------------- the plan each shape reaches
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_a_plan(V, monkeypatch, capfd, dtype):
    X, eps = _batch(SET_A, B_A, 1)
    plan = step_plan(V, monkeypatch, capfd, SET_A, B_A, dtype, X, eps, binary=BIN, transfer_fct="relu", seed=1)
    cf = {n: c for n, c, _i in plan}
    KU = 64 if dtype == "bf16" else 32
    rup = lambda n: (n + KU - 1) // KU * KU
    # cfg 2 NT, hidden forward: M = 3999, N = 1003 (% 128, % 8 != 0)
    c, items = [(c, it) for n, c, it in plan if n == "fwd_enc1"][0]
    assert c == 2 and items == [(K_FWD_HIDDEN, B_A, 1003, rup(785)), (K_FWD_HIDDEN, B_A, 1003, rup(148))], (c, items)
    # cfg 2 NT, hidden dgrad with a ragged N
    dg = [(n, it) for n, c, its in plan if c == 2 for it in its if it[0] == K_DGRAD_HIDDEN and it[1] == B_A and it[2] % 8 != 0]
    assert dg, [(n, c) for n, c, _i in plan]
    # cfg 1 NT: M = 3999, N = 605 / 640, K = 1004 -> K tiles with padding
    c, items = [(c, it) for n, c, it in plan if n == "fwd_enc2"][0]
    assert c == 1 and items == [(K_FWD_HIDDEN, B_A, 605, rup(1004)), (K_FWD_HIDDEN, B_A, 640, rup(1004))], (c, items)
    # cfg 6 loss: Bernoulli item (fan-in 605: bias row as a K row) and Gaussian item with the bias in the epilogue (fan-in 640,
    # a multiple of the K unit: K stops at 640)
    c, items = [(c, it) for n, c, it in plan if n == "fwd_out_loss"][0]
    assert c == 6 and items == [(K_FWD_OUT_LOSS, B_A, 784, rup(606)), (K_FWD_OUT_LOSS, B_A, 147, 640)], (c, items)
    # the latent item as a launch of its own
    c, items = [(c, it) for n, c, it in plan if n == "latent"][0]
    assert [(k, M) for k, M, _N, _K in items] == [(K_LATENT, B_A)], items
    # heads on 64x128 tiles: forward and the latent gradient
    c, items = [(c, it) for n, c, it in plan if n == "fwd_head"][0]
    assert c == 4 and [(k, M, N) for k, M, N, _K in items] == [(K_FWD_HEAD, B_A, 2 * NZ_A)] * 2, (c, items)
    assert any(c == 4 and any(it[0] == K_DGRAD_LATENT and it[1] == B_A for it in its) for _n, c, its in plan), cf
    # TN on 128x128 tiles (279 of them, 147 of 256x128: below cfg 2's 192), K = 3999
    wide = _wide_tn(SET_A, B_A)
    assert sum((M + 127) // 128 * ((N + 127) // 128) for M, N, _K in wide) >= 192
    assert sum((M + 255) // 256 * ((N + 127) // 128) for M, N, _K in wide) < 192
    assert [c for n, c, _i in plan if n.startswith("wgrad")][0] == 1, cf
    # k_adam, not the fused small-net launch: its tiles (16 x 64) end inside a quad on 1003-, 605- and 147-column layers
    assert 12 not in cf.values() and "wgrad+adam" not in cf, cf


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_b_plan(V, monkeypatch, capfd, dtype):
    X, eps = _batch(SET_B, B_B, 2)
    plan = step_plan(V, monkeypatch, capfd, SET_B, B_B, dtype, X, eps, binary=BIN, transfer_fct="relu", seed=2)
    cf = {n: c for n, c, _i in plan}
    wide = _wide_tn(SET_B, B_B)
    assert sum((M + 255) // 256 * ((N + 127) // 128) for M, N, _K in wide) >= 192
    # every wide product: K = 333 (not a multiple of any K tile), M = in + 1 with in % 256 != 0 (bias row inside a partial tile)
    assert all(K % 32 != 0 and (M - 1) % 256 != 0 for M, _N, K in wide), wide
    assert [c for n, c, _i in plan if n.startswith("wgrad")][0] == 2, cf


# ----------------------------------------------------------------------------- parity at every step
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_a_parity(V, dtype, act):
    """fp32 against the fp64 oracle, bf16 against the bf16-rounding oracle; relu with the kernels' own relu decisions, and tanh as
    the smooth transfer function (softplus at these widths drives the Gaussian modality's cost to 1e7 - 1e16 within a step,
    where the comparison measures the conditioning of the cost, not the kernels)."""
    check_step_parity(V, SET_A, BIN, [5.0, 1.0], 0.5, act, B_A, dtype, steps=3, seed=7, grad_every_step=True,
                      relu_masks=act == "relu")


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_b_parity(V, dtype, act):
    # fp32 drift bound as for the conv nets: 333 rows through 1500-wide layers leave many gradients near 1e-8, where Adam turns a
    # 1e-7 relative gradient error into a fraction of lr (the gradients at HIP's weights and the Adam arithmetic are checked at
    # every step); bf16 keeps its default bound
    check_step_parity(V, SET_B, BIN, [5.0, 1.0], 0.5, act, B_B, dtype, steps=3, seed=8, grad_every_step=True,
                      relu_masks=act == "relu", drift_tol=2.5e-3 if dtype == "fp32" else None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_set_a_replay_and_all_present_mask_bitwise(V, dtype):
    """Set A: 5 batches through partial_fit_steps (a 4-step replay and a single step) = 5 single steps, bitwise; and an all-present
    `present=` mask (the masked twin of the cfg-6 loss launch, with padding rows) = the unmasked step, bitwise."""
    n = 5
    X, eps = _batch(SET_A, B_A, 3, n)
    kw = dict(binary=BIN, transfer_fct="relu", weights=[5.0, 1.0], assoc_lambda=0.5, batch_size=B_A, compute_dtype=dtype, seed=3)
    res = []
    for many in (False, True):
        m = V.AssocVariationalAutoEncoder(SET_A, **kw)
        if many:
            m.partial_fit_steps(X, n, eps)
        else:
            for i in range(n):
                m.partial_fit([x[i * B_A:(i + 1) * B_A] for x in X], eps[i * B_A:(i + 1) * B_A])
        res.append((m.cost_history(n).copy(), m.get_params()) + m.get_opt_state()[:2])
        assert shadow_err(m)[:2] == (0.0, 0.0)
        del m
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert len(set(res[0][0].tolist())) == n
    res = []
    for present in (None, np.ones((B_A, 2), np.uint8)):
        m = V.AssocVariationalAutoEncoder(SET_A, **kw)
        c = m.partial_fit([x[:B_A] for x in X], eps[:B_A], present=present)
        res.append((c, m.get_params(), m.get_grads()))
        del m
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


# ----------------------------------------------------------------------------- Adam from crafted states
def _ckpt_layout(path, n_params):
    """byte offsets of (step, theta, m, v) in a checkpoint: "AVAECKPT" | u32 version | u32 n_mod | u32 n_z | per modality
    {n_input, L, hs[L], conv, gener1, gener2} | u64 P | i64 step | theta | m | v (P floats each)"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"AVAECKPT"
    u32 = lambda o: int(np.frombuffer(raw, np.uint32, 1, o)[0])
    off = 8
    assert u32(off) == 2
    n_mod = u32(off + 4)
    off += 12
    for _ in range(n_mod):
        L = u32(off + 4)
        off += 4 * (2 + L + 3)
    P = int(np.frombuffer(raw, np.uint64, 1, off)[0])
    assert P == n_params
    assert len(raw) == off + 16 + 12 * P, "checkpoint size %d != header %d + 16 + 12 P" % (len(raw), off)
    return raw, off + 8, off + 16


def _craft(src, dst, n_params, t0, seed):
    raw, o_step, o_th = _ckpt_layout(src, n_params)
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-30.0, 2.0, n_params)).astype(np.float32)
    v[rng.random(n_params) < 0.1] = 0.0
    assert np.all((v == 0) | (v >= np.finfo(np.float32).tiny))                      # no subnormals
    # |m| ~ sqrt(v): a state a real history can leave (a large m over a tiny v would throw the weights far in one step)
    m = (rng.standard_normal(n_params) * (np.sqrt(v.astype(np.float64)) + 1e-6)).astype(np.float32)
    P4 = 4 * n_params
    out = bytearray(raw)
    out[o_step:o_step + 8] = np.int64(t0).tobytes()
    out[o_th + P4:o_th + 2 * P4] = m.tobytes()
    out[o_th + 2 * P4:o_th + 3 * P4] = v.tobytes()
    with open(dst, "wb") as f:
        f.write(bytes(out))
    return m, v


_C2 = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
_CONV = [dict(make_arch("image", 784, 8, 24, 6), hidden_conv=True, n_hidden_gener_1=24, n_hidden_gener_2=8), make_arch("joint", 147, 40, 32, 6)]
ROUTES = {
    "fused": (_C2, 100, "bf16", {}),                                 # wgrad+adam (cfg 12)
    "unfused": (_C2, 100, "bf16", {"AVAE_NO_ADAM_FUSE": "1"}),       # the same net through k_grouped + k_adam
    "set_a": (SET_A, B_A, "bf16", {}),                               # k_adam, ragged edge tiles
    "conv": (_CONV, 12, "fp32", {}),                                  # k_adam + the conv stages' adjoint shadows (Wadj / Wf)
}
CASES = [(r, t) for r in ("fused", "unfused") for t in (5, 10 ** 6)] + \
        [("set_a", 4094), ("set_a", 2 ** 31 + 3), ("conv", 5), ("conv", 4094)]      # (fused / unfused at 4094, 2^31 + 3: below)


def _crafted_run(V, monkeypatch, tmp_path, route, t0):
    archs, B, dtype, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 16 if t0 == 4094 and route != "set_a" else 3      # from 4094 the cost ring wraps at the third step; 16 = one full replay
    X, eps = _batch(archs, B, 11, n)
    kw = dict(binary=BIN, transfer_fct="tanh", weights=[5.0, 1.0], assoc_lambda=0.5, learning_rate=1e-3, batch_size=B,
              compute_dtype=dtype, seed=4)
    a = V.AssocVariationalAutoEncoder(archs, **kw)
    a.partial_fit([x[:B] for x in X], eps[:B])
    src, dst = str(tmp_path / "src.ckpt"), str(tmp_path / "crafted.ckpt")
    a.save_model(src)
    m0, v0 = _craft(src, dst, a.n_params, t0, seed=t0 % 1000)
    a.restore_model(folder=str(tmp_path), fname="crafted.ckpt")
    b = V.AssocVariationalAutoEncoder(archs, **kw)
    b.restore_model(folder=str(tmp_path), fname="crafted.ckpt")
    mb, vb, tb = b.get_opt_state()
    assert tb == t0 and np.array_equal(mb, m0) and np.array_equal(vb, v0) and np.array_equal(a.get_params(), b.get_params())
    # b: n single steps, each checked against the optimiser arithmetic (conv: and its gradient against the oracle at b's weights)
    costs = []
    for i in range(n):
        Xi, ei = [x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B]
        before = opt_snapshot(b)
        costs.append(b.partial_fit(Xi, ei))
        g = b.get_grads()
        check_adam_step(before, opt_snapshot(b), g, 1e-3)
        if route == "conv":
            at = O.OracleAssocVAE(archs, BIN, "tanh", [5.0, 1.0], 0.5, 1e-3, B, params_flat=before[0].astype(np.float64))
            c_at, g_at, _ = at.cost_and_grads(Xi, ei)
            assert abs(costs[-1] - c_at) <= 1e-5 * abs(c_at), (i, costs[-1], c_at)
            bad = [(nm, e) for nm, e in per_tensor_err(archs, g, g_at) if e > 1e-4]
            assert not bad, (i, bad)
    assert b.get_opt_state()[2] == t0 + n
    hist = b.cost_history(n)
    assert np.array_equal(hist, np.array(costs, np.float32)), (hist, costs)
    # a: the same n batches in one multi-step replay
    a.partial_fit_steps(X, n, eps)
    ma, va, ta = a.get_opt_state()
    mb, vb, tb = b.get_opt_state()
    assert ta == tb == t0 + n
    assert np.array_equal(a.cost_history(n), hist)
    assert np.array_equal(a.get_params(), b.get_params()) and np.array_equal(ma, mb) and np.array_equal(va, vb)
    for h in (a, b):
        assert shadow_err(h)[:2] == (0.0, 0.0)
    return b.get_params(), mb, vb, hist


@pytest.mark.parametrize("route,t0", CASES)
def test_adam_from_crafted_state(V, monkeypatch, tmp_path, route, t0):
    _crafted_run(V, monkeypatch, tmp_path, route, t0)


@pytest.mark.parametrize("t0", [4094, 2 ** 31 + 3])
def test_adam_fused_equals_unfused_from_crafted_state(V, monkeypatch, tmp_path, t0):
    """The fused wgrad+adam launch and the k_grouped + k_adam pair from the same crafted state: bitwise."""
    fused = _crafted_run(V, monkeypatch, tmp_path, "fused", t0)
    unfused = _crafted_run(V, monkeypatch, tmp_path, "unfused", t0)
    for x, y in zip(fused, unfused):
        assert np.array_equal(x, y)


def test_adam_routes_reach_their_launches(V, monkeypatch, capfd):
    """the crafted-state routes run what they are named for: the fused launch (cfg 12) or not"""
    for route, want in (("fused", True), ("unfused", False)):
        archs, B, dtype, env = ROUTES[route]
        X, eps = _batch(archs, B, 11)
        plan = step_plan(V, monkeypatch, capfd, archs, B, dtype, X, eps, env=env, binary=BIN, transfer_fct="tanh", seed=4)
        assert (("wgrad+adam", 12) in [(n, c) for n, c, _i in plan]) == want, (route, [(n, c) for n, c, _i in plan])
