"""Parity of the HIP path (through the C ABI, include/avae.h) with the CPU oracle on a real MI355X.

Tolerances (the oracle is fp64):
  fp32 path : mu / lv / x_hat / cost <= 1e-5 relative, gradients <= 1e-4 of the tensor's max
  bf16 path : cost <= 1e-3 relative (north_star), mu / lv <= 2e-2 absolute
PARITY UNPINNED against the reference itself (it cannot run; see oracle/vae_assoc_oracle.py).
"""
import os
import threading

import numpy as np
import pytest
import torch

from conftest import GOLDEN, hip_relu_masks, make_arch, synth_batch, shadow_err
from oracle import vae_assoc_oracle as O
from plan_dump import step_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def per_tensor_err(archs, got, ref):
    """max |got-ref| / max |ref| per named parameter tensor (flat layout)."""
    out, off = [], 0
    for m, na in enumerate(archs):
        for name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            a, b = got[off:off + n], ref[off:off + n]
            out.append(("m%d.%s" % (m, name), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))))
            off += n
    return out


def build_pair(V, archs, binary, weights, lam, act, B, dtype, lr=1e-3, p0=None, seed=5, **kw):
    model = V.AssocVariationalAutoEncoder(archs, binary=binary, transfer_fct=act, weights=weights, assoc_lambda=lam,
                                          learning_rate=lr, batch_size=B, compute_dtype=dtype, seed=seed, **kw)
    if p0 is None:
        rng = np.random.default_rng(seed)
        p0 = model.get_params()
        off = 0
        for na in archs:                       # non-zero biases: exercise the folded-bias column
            for name, shp in O.layer_shapes(na):
                n = int(np.prod(shp))
                if len(shp) == 1:
                    p0[off:off + n] = 0.05 * rng.standard_normal(n)
                off += n
    model.set_params(p0)
    assert np.array_equal(model.get_params(), p0.astype(np.float32))         # set/get round trip is exact
    ref = O.OracleAssocVAE(archs, binary, act, weights, lam, lr, B, params_flat=np.asarray(p0, dtype=np.float64))
    return model, ref


U32 = 2.0 ** -23            # fp32 spacing at 1: one ulp of x is at most U32 * |x|
TINY32 = 2.0 ** -126        # smallest normal fp32: a subnormal intermediate flushed to zero moves a result by less


def adam_lr_t(lr, t):
    """lr_t as the step's K_COST item forms it (avae_kernels.hip::cost_item): f32 lr and betas widened to double, rounded to f32"""
    b1, b2 = float(np.float32(O.ADAM_BETA1)), float(np.float32(O.ADAM_BETA2))
    return float(np.float32(float(np.float32(lr)) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def check_adam_step(before, after, g, lr):
    """One optimiser step of the HIP path, decoupled from gradient conditioning: `before` / `after` = (theta, m, v, step) read
    from the handle around the step, `g` = the step's gradient.  The kernel's expression (avae_kernels.hip::adam_update) is
    evaluated in fp64 with its fp32 constants, omb = f32(1 - f32(beta)), and the bounds are the kernel's own roundings:
      m_t = m + (g - m) omb1: two roundings, 1/2 ulp of |g - m| <= 2a times omb1 = 0.1 and 1/2 ulp of |m_t| <= a, a = max(|m|, |g|):
          < 0.6 ulp of a                                                                                -> bound U32 * a
      v_t = v + (g^2 - v) omb2: 1/2 ulp of |g^2 - v| <= b times 0.001 and 1/2 ulp of v_t <= b, b = max(v, g^2)  -> bound U32 * b
      theta_t = theta - (m_t lr_t) / (sqrt(v_t) + eps) from HIP's own m_t, v_t: four roundings of 1/2 ulp in the update (product,
          root, sum of non-negative terms, quotient) and 1/2 ulp of |theta_t| in the subtraction  -> U32 * (|theta_t| + 3 |update|)
    plus TINY32 each (flushed subnormal intermediates).  The step counter must advance by one."""
    th0, m0, v0, t0 = before
    th1, m1, v1, t1 = after
    assert t1 == t0 + 1, "step counter %d after a step from %d" % (t1, t0)
    f32 = np.float32
    omb1, omb2 = float(f32(1.0) - f32(O.ADAM_BETA1)), float(f32(1.0) - f32(O.ADAM_BETA2))
    eps = float(f32(O.ADAM_EPS))
    lr_t = adam_lr_t(lr, t1)
    g, m0, v0, th0 = (np.asarray(a, np.float64) for a in (g, m0, v0, th0))
    m1d, v1d = m1.astype(np.float64), v1.astype(np.float64)
    m_want = m0 + (g - m0) * omb1
    err = np.abs(m1d - m_want) - (U32 * np.maximum(np.abs(m0), np.abs(g)) + TINY32)
    assert err.max() <= 0, "Adam m at step %d: worst element %d (m %r g %r -> %r, want %r)" % (
        t1, int(err.argmax()), m0[err.argmax()], g[err.argmax()], m1d[err.argmax()], m_want[err.argmax()])
    v_want = v0 + (g * g - v0) * omb2
    err = np.abs(v1d - v_want) - (U32 * np.maximum(v0, g * g) + TINY32)
    assert err.max() <= 0, "Adam v at step %d: worst element %d (v %r g %r -> %r, want %r)" % (
        t1, int(err.argmax()), v0[err.argmax()], g[err.argmax()], v1d[err.argmax()], v_want[err.argmax()])
    upd = m1d * lr_t / (np.sqrt(v1d) + eps)
    th_want = th0 - upd
    err = np.abs(th1.astype(np.float64) - th_want) - (U32 * (np.abs(th_want) + 3.0 * np.abs(upd)) + TINY32)
    assert err.max() <= 0, "Adam theta at step %d: worst element %d (theta %r update %r -> %r, want %r)" % (
        t1, int(err.argmax()), th0[err.argmax()], upd[err.argmax()], th1[err.argmax()], th_want[err.argmax()])


def opt_snapshot(model):
    m, v, t = model.get_opt_state()
    return model.get_params(), m, v, t


def check_step_parity(V, archs, binary, weights, lam, act, B, dtype, steps=3, seed=5, ref_config=False, drift_tol=None,
                      adam_rel=False, grad_every_step=False, relu_masks=False, **kw):
    """HIP path vs oracle on the same weights / inputs / eps.

    fp32 operands: against the fp64 oracle at the fp32 tolerances of the module docstring.
    bf16 operands: (1) against the oracle run with quant='bf16', which rounds at exactly the points
    the kernels round (same relu decisions), tightly -- this is the correctness check of the bf16
    kernels; (2) against the plain fp64 oracle at the north_star tolerances (cost 1e-3 relative on the
    reference configurations, mu/lv 2e-2 absolute) -- this is the measured price of bf16 operands.
    adam_rel: the Adam arithmetic bound 6e-8 is taken relative to max(1, |theta|) per element (fp32 resolves only ~5e-7 at
    |theta| = 8-16, e.g. the head biases of posteriors far from the prior).
    Every step: the optimiser arithmetic from HIP's own theta / m / v / step before it and gradient after it (check_adam_step).
    grad_every_step: also HIP's gradient of every later step against the like-for-like oracle evaluated at HIP's weights of
    that step (the free-running oracle drifts away from them) -- the gradients that run on shadows the optimiser wrote.
    relu_masks (relu): the oracle takes the relu decisions of HIP's pass of the same step (hip_relu_masks), so a pre-activation
    within rounding of the kink cannot fall on different sides in the two runs."""
    fp32 = dtype == "fp32"
    lr = 1e-3
    rng = np.random.default_rng(seed + 100)
    nz = archs[0]["n_z"]
    blist = binary if isinstance(binary, list) else [binary] * len(archs)
    X = synth_batch(rng, B, [a["n_input"] for a in archs], blist)
    eps = rng.standard_normal((steps, B, nz)).astype(np.float32)
    model, ref = build_pair(V, archs, binary, weights, lam, act, B, dtype, seed=seed, **kw)
    p0 = model.get_params().astype(np.float64)
    emu = ref if fp32 else O.OracleAssocVAE(archs, binary, act, weights, lam, lr, B, params_flat=p0, quant="bf16")
    c_tol0 = 1e-5 if fp32 else 5e-5                    # vs the like-for-like oracle
    g_tol = 1e-4 if fp32 else 3e-3
    # -- encoder outputs
    mus, emu_mu, ref_mu = model.transform(X), emu.transform(X), ref.transform(X)
    for m in range(len(archs)):
        scale = max(1.0, np.abs(emu_mu[m]).max())
        # bf16: fp32 vs fp64 accumulation flips the bf16 rounding of a few hidden activations by one ulp
        assert np.abs(mus[m] - emu_mu[m]).max() <= (1e-5 if fp32 else 2e-3) * scale, "mu[%d] vs like-for-like oracle" % m
        assert np.abs(mus[m] - ref_mu[m]).max() <= (1e-5 * scale if fp32 else 2e-2 * scale), "mu[%d] vs fp64 oracle" % m
    # -- evaluate_cost: parity, and it must not change anything
    p_before = model.get_params()
    c_eval = model.evaluate_cost(X, eps[0])
    e_eval = emu.evaluate_cost(X, eps[0])
    assert abs(c_eval - e_eval) <= c_tol0 * abs(e_eval), "evaluate_cost %.6f vs %.6f" % (c_eval, e_eval)
    assert np.array_equal(model.get_params(), p_before)
    # -- training steps: cost of the pre-update forward pass, gradients, Adam
    for s in range(steps):
        c_ref = ref.partial_fit(X, eps[s]) if not fp32 else None
        before = opt_snapshot(model)
        c = model.partial_fit(X, eps[s])
        g = model.get_grads()
        masks = hip_relu_masks(model, archs) if relu_masks else None
        check_adam_step(before, opt_snapshot(model), g, lr)
        assert before[3] == s, "step counter %d before step %d" % (before[3], s)
        c_emu, g_emu, fw = emu.cost_and_grads(X, eps[s], masks=masks)
        emu.apply_gradients(g_emu)
        if s > 0 and grad_every_step:
            at = O.OracleAssocVAE(archs, binary, act, weights, lam, lr, B, params_flat=before[0].astype(np.float64),
                                  quant=None if fp32 else "bf16")
            c_at, g_at, _ = at.cost_and_grads(X, eps[s], masks=masks)
            assert abs(c - c_at) <= c_tol0 * abs(c_at), "step %d cost %.6f vs oracle at HIP's weights %.6f" % (s, c, c_at)
            bad = [(n, e) for n, e in per_tensor_err(archs, g, g_at) if e > g_tol]
            assert not bad, "step %d gradient vs oracle at HIP's weights (rel to tensor max): %s" % (s, bad)
        # later steps start from weights that differ in the Adam-ill-conditioned elements (|g| ~ 1e-8)
        tol = c_tol0 if s == 0 else (2e-5 if fp32 else 3e-4)
        assert abs(c - c_emu) <= tol * abs(c_emu), "step %d cost %.6f vs like-for-like oracle %.6f (rel %.2e)" % (
            s, c, c_emu, abs(c - c_emu) / abs(c_emu))
        if not fp32:
            ctol = 1e-3 if ref_config else 1e-2
            assert abs(c - c_ref) <= ctol * abs(c_ref), "step %d bf16 cost %.6f vs fp64 oracle %.6f (rel %.2e)" % (
                s, c, c_ref, abs(c - c_ref) / abs(c_ref))
        if s == 0:
            errs = per_tensor_err(archs, g, g_emu)
            bad = [(n, e) for n, e in errs if e > g_tol]
            assert not bad, "gradient mismatch (rel to tensor max): %s" % bad
            # Adam arithmetic, decoupled from gradient conditioning: TF-1 update of p0 with the HIP gradient
            th1, _, _ = O.adam_step(p0, np.zeros_like(p0), np.zeros_like(p0), g.astype(np.float64), 1, lr)
            bound = 6e-8 * (np.maximum(1.0, np.abs(th1)) if adam_rel else 1.0)
            assert np.all(np.abs(model.get_params() - th1) <= bound), "Adam update arithmetic: max err %.3e" % (
                np.abs(model.get_params() - th1).max())
            for m in range(len(archs)):          # mu / lv of the training forward pass
                mulv = fetch(model, "mulv%d" % m, (B, 2 * nz))
                scale = max(1.0, np.abs(fw[m]["lv"]).max(), np.abs(fw[m]["mu"]).max())
                tol_l = (1e-5 if fp32 else 2e-3) * scale
                assert np.abs(mulv[:, :nz] - fw[m]["mu"]).max() <= tol_l
                assert np.abs(mulv[:, nz:] - fw[m]["lv"]).max() <= tol_l
    dp = np.abs(model.get_params() - emu.get_params()).max()
    # Adam normalises the step: an element with |g| ~ 1e-8 turns a 1e-7 relative gradient error into
    # a visible fraction of lr, so the end-to-end drift bound is loose; the arithmetic was checked above
    assert dp <= (drift_tol if drift_tol is not None else 2e-4 if fp32 else 2.5 * steps * lr), "params drift %.3e" % dp
    assert shadow_err(model)[:2] == (0.0, 0.0), "a compute-dtype shadow differs from its parameters"
    return model, emu, X, eps


# ----------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", ["script_nz4_b64", "c1_nz20_b100"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_golden_fixture(V, golden, name, dtype):
    G = golden[name]
    c = G["config"]
    fp32 = dtype == "fp32"
    M = len(c["archs"])
    X = [G["x%d" % m] for m in range(M)]
    model = V.AssocVariationalAutoEncoder(c["archs"], binary=c["binary"], transfer_fct=c["act"], weights=c["weights"],
                                          assoc_lambda=c["assoc_lambda"], learning_rate=c["lr"], batch_size=c["B"],
                                          compute_dtype=dtype)
    model.set_params(G["params0"])
    mus = model.transform(X)
    for m in range(M):
        assert np.abs(mus[m] - G["mu%d" % m]).max() <= (1e-5 * max(1, np.abs(G["mu%d" % m]).max()) if fp32 else 2e-2)
    tol_c = 1e-5 if fp32 else 1e-3                     # fixture = fp64 oracle: bf16 gets the north_star 1e-3
    costs = []
    for s in range(3):
        costs.append(model.partial_fit(X, G["eps"][s]))
        if s == 0:
            if fp32:
                g_want = G["grads0"].astype(np.float64)
            else:   # like-for-like: the oracle with the kernels' bf16 rounding points, on the fixture's inputs
                emu = O.OracleAssocVAE(c["archs"], c["binary"], c["act"], c["weights"], c["assoc_lambda"], c["lr"], c["B"],
                                       params_flat=G["params0"].astype(np.float64), quant="bf16")
                _, g_want, _ = emu.cost_and_grads(X, G["eps"][0])
            errs = per_tensor_err(c["archs"], model.get_grads(), g_want)
            bad = [(n, e) for n, e in errs if e > (1e-4 if fp32 else 3e-3)]
            assert not bad, bad
            if fp32:
                assert np.abs(model.get_params() - G["params1"]).max() <= 1e-5
    assert np.allclose(costs, G["costs"], rtol=tol_c, atol=0), (costs, G["costs"])
    assert np.abs(model.get_params() - G["params3"]).max() <= (2e-4 if fp32 else 7.5e-3)
    assert np.allclose(model.cost_history(3), costs, rtol=1e-6)
    m_, v_, step = model.get_opt_state()
    assert step == 3
    if fp32:
        assert abs(np.linalg.norm(m_.astype(np.float64)) - G["adam_m3_norm"]) <= 1e-4 * G["adam_m3_norm"]
        assert abs(np.linalg.norm(v_.astype(np.float64)) - G["adam_v3_norm"]) <= 1e-4 * G["adam_v3_norm"]
    # inference surface on the trained weights (fp32: weights equal the oracle's to ~1e-6)
    if fp32:
        t = model.transform(X)
        gen = model.generate(G["eps"][1])
        rec = model.reconstruct(X, eps=[G["eps"][1], G["eps"][2]])
        for m in range(M):
            assert np.abs(t[m] - G["t_mu%d" % m]).max() <= 1e-4
            assert np.abs(gen[m][:16] - G["gen%d" % m]).max() <= 1e-4
            assert np.abs(rec[m][:16] - G["rec%d" % m]).max() <= 1e-4
        ce = model.evaluate_cost(X, G["eps"][2])
        assert abs(ce - G["eval_cost3"]) <= 1e-4 * abs(G["eval_cost3"])


def _load_big():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_big", os.path.join(GOLDEN, "make_golden_big.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_sampled(G, tag, got, what, tol, noise=0.0):
    """HIP tensor set `got` (flat) against the fixture's per-tensor maxima / norms / sampled entries of run `tag`.
    `noise` > 0 (bf16 runs of deep relu nets): the bound of a tensor is max(tol, noise x d), d = the distance between the fixture's
    own bf16-rounding and fp64 runs on that tensor -- two runs that round to bf16 at the same points but accumulate differently
    (fp32 MFMA vs fp64) flip the rounding of some activations by one ulp and the relu decision of pre-activations near 0, and what
    that does to a tensor's gradient scales with that tensor's sensitivity to bf16 rounding, which d measures."""
    ptr, idx = G["sample_ptr"], G["sample_idx"]
    bad = []
    for t, name in enumerate(G["names"]):
        sl = slice(int(ptr[t]), int(ptr[t + 1]))
        mx = max(float(G[what + "max_" + tag][t]), 1e-30)
        err = float(np.abs(got[idx[sl]] - G[what + "sample_" + tag][sl]).max()) / mx
        bound = tol
        if noise > 0.0:
            bound = max(tol, noise * float(np.abs(G[what + "sample_bf16"][sl] - G[what + "sample_f64"][sl]).max()) / mx)
        if err > bound:
            bad.append((str(name), "sample", err, bound))
    return bad


def test_c4_full_size_gradients(V):
    """BASELINE C4 at the BENCHMARK size (4 x 1024 hidden, n_z = 64, batch 4096, bf16) against the committed
    fixture of the oracle run at that size (tests/golden/c4_b4096.npz, made by make_golden_big.py): cost, posterior statistics and
    every tensor's gradient -- maxima, L2 norms and 1024 sampled entries per tensor.  This is the plan the bench times: 256x128
    8-wave tiles with the register epilogue, bias folded into the epilogue, 256x64 loss tiles, the 20-item XCD-packed
    weight-gradient launch on producer waves, 64x128 head tiles."""
    big = _load_big()
    G = np.load(os.path.join(GOLDEN, "c4_b4096.npz"), allow_pickle=False)
    c = big.C4
    X, eps, p0 = big.c4_inputs()
    chk = [float(X[0].astype(np.float64).sum()), float(X[1].astype(np.float64).sum()), float(eps.astype(np.float64).sum()), float(p0.astype(np.float64).sum())]
    assert np.allclose(chk, G["checksum"], rtol=1e-12), "the seeded inputs are not the ones the fixture was made from"
    # 1) softplus, strict: the same plan (tile shapes, launch tables, XCD packing; the transfer function changes no launch) without
    # relu's kink -- with relu and 33 M hidden pre-activations per pass a few land within rounding of 0 and flip their derivative
    # between two arithmetic types: measured on the fp32 kernels against the fp64 run, ONE of 1024 sampled entries of dec_b4 /
    # dec_b3 off by 1e-3 of the tensor maximum (one sample's contribution), the rest at 1e-6 (tools/c4_grad_diag.py).
    # fp32 operands on the exact-fp32 MFMA kernels against the fp64 run, bf16 operands against the bf16-rounding run.
    for dtype, tag, ctol, gtol in (("fp32", "f64_softplus", 1e-5, 1e-4), ("bf16", "bf16_softplus", 5e-5, 3e-3)):
        m = V.AssocVariationalAutoEncoder(c["archs"], binary=c["binary"], transfer_fct="softplus", weights=c["weights"],
                                          assoc_lambda=c["assoc_lambda"], learning_rate=c["lr"], batch_size=c["B"], compute_dtype=dtype)
        m.set_params(p0)
        cost = m.partial_fit(X, eps)
        assert abs(cost - float(G["cost_" + tag])) <= ctol * abs(cost), (dtype, cost, float(G["cost_" + tag]))
        bad = _check_sampled(G, tag, m.get_grads().astype(np.float64), "g", gtol)
        assert not bad, (dtype, bad)
        del m
    # 2) relu = the benchmark configuration itself, bf16: cost at both tolerances, gradients within the noise-aware bound
    m = V.AssocVariationalAutoEncoder(c["archs"], binary=c["binary"], transfer_fct=c["act"], weights=c["weights"], assoc_lambda=c["assoc_lambda"],
                                      learning_rate=c["lr"], batch_size=c["B"], compute_dtype="bf16")
    assert m.n_params == 14900387
    m.set_params(p0)
    cost = m.partial_fit(X, eps)
    assert abs(cost - float(G["cost_bf16"])) <= 5e-5 * abs(cost), (cost, float(G["cost_bf16"]))        # like-for-like oracle
    assert abs(cost - float(G["cost_f64"])) <= 1e-3 * abs(cost), (cost, float(G["cost_f64"]))           # north_star: 1e-3 of the fp64 run
    g = m.get_grads().astype(np.float64)
    bad = _check_sampled(G, "bf16", g, "g", 3e-3, noise=0.5)        # the committed fixture: noise-aware (relu kink flips, see _check_sampled)
    assert not bad, bad
    # the plain 3e-3 bound on the BENCHMARK transfer function.  The oracle (rounding where the kernels round) is run
    # here with the kernels' own relu decisions -- the stored activations of the pass above -- so no pre-activation within rounding
    # of 0 can fall on different sides in the two runs, and EVERY entry of every tensor is compared, not a sample.
    emu = O.OracleAssocVAE(c["archs"], c["binary"], c["act"], c["weights"], c["assoc_lambda"], c["lr"], c["B"],
                           params_flat=p0.astype(np.float64), quant="bf16")
    c_emu, g_emu, _ = emu.cost_and_grads(X, eps, masks=hip_relu_masks(m, c["archs"]))
    assert abs(c_emu - float(G["cost_bf16"])) <= 1e-9 * abs(c_emu)
    bad = [(n, e) for n, e in per_tensor_err(c["archs"], g, g_emu) if e > 3e-3]
    assert not bad, bad
    off = 0
    for t, (name, shp) in enumerate([(n, s) for na in c["archs"] for n, s in O.layer_shapes(na)]):
        n = int(np.prod(shp))
        l2, want = float(np.linalg.norm(g[off:off + n])), float(G["gl2_bf16"][t])
        assert abs(l2 - want) <= 5e-3 * want, (name, l2, want)
        assert abs(float(np.abs(g[off:off + n]).max()) - float(G["gmax_bf16"][t])) <= 1e-2 * float(G["gmax_bf16"][t]), name
        off += n
    for k in range(2):
        mulv = fetch(m, "mulv%d" % k, (c["B"], 128))[:64]
        assert np.abs(mulv[:, :64] - G["mu%d_bf16" % k]).max() <= 2e-3 * max(1.0, np.abs(G["mu%d_bf16" % k]).max())
        assert np.abs(mulv[:, 64:] - G["lv%d_bf16" % k]).max() <= 2e-3 * max(1.0, np.abs(G["lv%d_bf16" % k]).max())
        assert np.abs(mulv[:, :64] - G["mu%d_f64" % k]).max() <= 2e-2 * max(1.0, np.abs(G["mu%d_f64" % k]).max())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["conv_small", "c5_small"])
def test_round2_small_fixtures(V, name, dtype):
    """Committed fixtures for the conv/deconv branch and for the 3-modality (C5) net: cost, gradients (sampled entries of every
    tensor) and two Adam steps against the oracle outputs stored in tests/golden/."""
    big = _load_big()
    G = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    c, X, eps, p0 = big.small_inputs(name)
    fp32 = dtype == "fp32"
    tag = "f64" if fp32 else "bf16"
    m = V.AssocVariationalAutoEncoder(c["archs"], binary=c["binary"], transfer_fct=c["act"], weights=c["weights"], assoc_lambda=c["assoc_lambda"],
                                      learning_rate=c["lr"], batch_size=c["B"], compute_dtype=dtype)
    m.set_params(p0)
    costs = [m.partial_fit(X, eps[0])]
    assert abs(costs[0] - float(G["cost0_" + tag])) <= (1e-5 if fp32 else 5e-5) * abs(costs[0])
    bad = _check_sampled(G, tag, m.get_grads().astype(np.float64), "g", 1e-4 if fp32 else 3e-3)
    assert not bad, bad
    costs.append(m.partial_fit(X, eps[1]))
    assert np.allclose(costs, G["costs_" + tag], rtol=2e-5 if fp32 else 3e-4)
    if not fp32:
        assert np.allclose(costs, G["costs_f64"], rtol=1e-2)       # (small nets, few terms: the 1e-3 bound is for the reference configs)
    p2 = m.get_params().astype(np.float64)
    assert np.abs(p2[G["sample_idx"]] - G["p2sample_" + tag]).max() <= (2e-4 if fp32 else 5e-3)


# ----------------------------------------------------------------------------- full reference sizes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_reference_default_architecture(V, dtype):
    """784-500-500 / 147-200-200 (vae_assoc_ujichar_img_jnt.py:53-71), n_z=20, B=100 (BASELINE C1)."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", 100, dtype, ref_config=True)


def test_bench_config_c2_bf16(V):
    """BASELINE C2: same nets, n_z=20, B=256, bf16."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", 256, "bf16", ref_config=True)


# ----------------------------------------------------------------------------- shapes / options
@pytest.mark.parametrize("lam", [0.0, 1e-5, 1e-2, 1.0, 8.0, 50.0])
def test_config_c5_three_modalities_lambda_sweep(V, lam):
    """BASELINE.json configs[4]: img + jnt + 256-d aux, fp32, association weight swept over the values the reference's
    callers use (train default 1e-5 vae_assoc.py:498, script 8, robot app 50) -- per-GPU shard of 256 rows."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20), make_arch("aux", 256, 200, 200, 20)]
    check_step_parity(V, archs, [True, False, False], [50.0, 1.0, 1.0], lam, "relu", 256, "fp32", steps=1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [
    dict(archs=[make_arch("a", 60, 20, 16, 5), make_arch("b", 21, 12, 10, 5)], binary=[True, False], w=[50.0, 1.0], lam=8.0, act="relu", B=9),
    dict(archs=[make_arch("a", 60, 20, 16, 3), make_arch("b", 21, 12, 10, 3), make_arch("c", 256, 40, 40, 3)],
         binary=[True, False, False], w=[2.0, 1.0, 0.5], lam=0.7, act="softplus", B=37),
    dict(archs=[make_arch("a", 130, 0, 0, 4, n_hidden=[70, 65, 33]), make_arch("b", 11, 0, 0, 4, n_hidden=[7])],
         binary=[False, True], w=[1.0, 3.0], lam=1e-2, act="tanh", B=64),
    dict(archs=[make_arch("solo", 25, 9, 7, 1)], binary=True, w=1.0, lam=3.0, act="sigmoid", B=130),
    dict(archs=[make_arch("a", 200, 0, 0, 64, n_hidden=[96]), make_arch("b", 70, 0, 0, 64, n_hidden=[80, 72])],
         binary=[True, False], w=[1.0, 1.0], lam=0.05, act="relu", B=200),          # n_z=64: 128x128 head tile
    dict(archs=[make_arch("a", 40, 24, 24, 6), make_arch("b", 30, 24, 24, 6), make_arch("c", 20, 16, 16, 6), make_arch("d", 10, 8, 8, 6)],
         binary=[True, False, True, False], w=[1.0, 2.0, 3.0, 4.0], lam=0.3, act="identity", B=33),
    dict(archs=[make_arch("a", 128, 0, 0, 16, n_hidden=[64, 128]), make_arch("b", 64, 0, 0, 16, n_hidden=[192])],
         binary=[True, False], w=[1.0, 1.0], lam=0.2, act="softplus", B=96),        # fan-ins of k*64: bias gradient from the ones MFMA
    dict(archs=[make_arch("a", 50, 0, 0, 7, n_hidden=[40, 36, 32, 28, 24, 20, 16, 12]), make_arch("b", 33, 0, 0, 7, n_hidden=[30, 28, 26, 24, 22, 20, 18, 16]),
                make_arch("c", 21, 0, 0, 7, n_hidden=[20, 19, 18, 17, 16, 15, 14, 13]), make_arch("d", 9, 0, 0, 7, n_hidden=[12, 12, 12, 12, 12, 12, 12, 12])],
         binary=[True, False, True, False], w=[1.0, 0.5, 2.0, 1.5], lam=0.4, act="softplus", B=20),   # the ABI's maxima: 4 modalities x 8 hidden layers
])
def test_shapes_and_options(V, case, dtype):
    check_step_parity(V, case["archs"], case["binary"], case["w"], case["lam"], case["act"], case["B"], dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_random_shapes(V, dtype):
    """25 seeded random models (1-4 modalities, 1-3 hidden layers, widths 1-150, n_z 1-64, batch 1-200, every activation,
    mixed Bernoulli / Gaussian): one train step each against the oracle at the tolerances of check_step_parity.  Odd sizes are
    where a tiling mistake would read or write out of range."""
    rng = np.random.default_rng(2026)
    acts = ["relu", "softplus", "tanh", "sigmoid", "identity"]
    for case in range(25):
        M = int(rng.integers(1, 5))
        nz = int(rng.choice([1, 2, 3, 5, 8, 20, 31, 33, 64]))
        B = int(rng.choice([1, 2, 7, 31, 32, 33, 63, 65, 100, 129, 200]))
        archs, binary, w = [], [], []
        for m in range(M):
            hs = [int(rng.integers(1, 151)) for _ in range(int(rng.integers(1, 4)))]
            archs.append(make_arch("m%d" % m, int(rng.integers(1, 301)), 0, 0, nz, n_hidden=hs))
            binary.append(bool(rng.integers(0, 2)))
            w.append(float(rng.choice([0.5, 1.0, 3.0, 50.0])))
        lam = float(rng.choice([0.0, 1e-5, 0.3, 8.0]))
        act = acts[case % len(acts)]
        try:
            check_step_parity(V, archs, binary, w, lam, act, B, dtype, steps=1, seed=100 + case)
        except AssertionError as e:
            raise AssertionError("case %d: M=%d nz=%d B=%d act=%s archs=%s: %s" % (
                case, M, nz, B, act, [(a["n_input"], a["n_hidden"]) for a in archs], e))


def test_random_conv_shapes(V):
    """Random conv / deconv depths (1..80 channels: below and above the 64-channel limit of the adjoint-frame route,
    multiples of 4 and not, different per modality), 1-3 modalities of which at least one is conv, random batch and
    latent width, fp32 (tight tolerance: a routing or indexing mistake shows)."""
    rng = np.random.default_rng(77)
    for case in range(24):
        M = int(rng.integers(1, 4))
        nz = int(rng.choice([2, 5, 8, 20]))
        B = int(rng.choice([3, 8, 17, 32]))
        conv = [True] + [bool(rng.integers(0, 2)) for _ in range(M - 1)]
        rng.shuffle(conv)
        archs, binary, w = [], [], []
        for m in range(M):
            if conv[m]:
                r1, r2 = int(rng.integers(1, 25)), int(rng.integers(1, 81))
                g1, g2 = int(rng.choice([2, 6, 20, 64, 130, 160])), int(rng.integers(1, 21))
                archs.append(dict(make_arch("c%d" % m, 784, r1, r2, nz), hidden_conv=True, n_hidden_gener_1=g1, n_hidden_gener_2=g2))
                binary.append(True)
            else:
                archs.append(make_arch("m%d" % m, int(rng.integers(1, 200)), int(rng.integers(1, 90)), int(rng.integers(1, 90)), nz))
                binary.append(bool(rng.integers(0, 2)))
            w.append(float(rng.choice([0.5, 1.0, 3.0])))
        lam = float(rng.choice([0.0, 0.3, 8.0]))
        try:
            # drift bound of the bf16 runs: one-channel sigmoid maps (G1 = 2) leave many gradients near 1e-8, where Adam turns
            # a 1e-7 relative gradient error into a fraction of lr (the gradients and the Adam arithmetic are checked tightly)
            check_step_parity(V, archs, binary, w, lam, "relu", B, "fp32", steps=1, seed=300 + case, drift_tol=2.5e-3)
        except AssertionError as e:
            raise AssertionError("case %d: nz=%d B=%d conv=%s archs=%s: %s" % (
                case, nz, B, conv, [(a.get("n_hidden_recog_1"), a.get("n_hidden_recog_2"), a.get("n_hidden_gener_1"), a.get("n_hidden_gener_2")) for a in archs], e))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_deconv_branch(V, dtype):
    """hidden_conv=True image modality (vae_assoc.py:169-210,249-291; deconv.py) paired with the MLP joint
    modality: the commented-out configuration of vae_assoc_ujichar_img_jnt.py:72-80 (depths 16/64, 64/16)."""
    img = dict(make_arch("image", 784, 16, 64, 20), hidden_conv=True, n_hidden_gener_1=64, n_hidden_gener_2=16)
    jnt = make_arch("joint", 147, 200, 200, 20)
    model, emu, X, eps = check_step_parity(V, [img, jnt], [True, False], [50.0, 1.0], 8.0, "relu", 24, dtype, steps=2, grad_every_step=True)
    # inference surface of the conv modality, any row count
    rng = np.random.default_rng(9)
    for rows in (1, 24, 31):
        Xr = synth_batch(rng, rows, [784, 147], [True, False])
        z = rng.standard_normal((rows, 20)).astype(np.float32)
        e = [rng.standard_normal((rows, 20)).astype(np.float32) for _ in range(2)]
        tol = 2e-5 if dtype == "fp32" else 3e-3
        assert np.abs(model.transform(Xr)[0] - emu.transform(Xr)[0]).max() <= tol * 5
        assert np.abs(model.generate(z)[0] - emu.generate(z)[0]).max() <= tol
        assert np.abs(model.reconstruct(Xr, eps=e)[0] - emu.reconstruct(Xr, eps=e)[0]).max() <= tol


@pytest.mark.parametrize("policy", [None, "E:fwb,H:fwb,D1:fwb,DT:fwb", "E:fw,H:fwb,D1:fwb,DT:wb"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_branch_at_bench_size(V, monkeypatch, dtype, policy):
    """`bench.py --config c2conv` (depths 16/64, 64/16; batch 256): at this size the decoder's stages take the direct
    (one output channel) and adjoint-frame routes with split reductions over 256 images x 49..784 pixels; the conv stages, the
    heads and the first decoder stage are implicit GEMMs (default policy), or every stage is (the other two policies)."""
    if policy:
        monkeypatch.setenv("AVAE_IMPL_POLICY", policy)
    img = dict(make_arch("image", 784, 16, 64, 20), hidden_conv=True, n_hidden_gener_1=64, n_hidden_gener_2=16)
    jnt = make_arch("joint", 147, 200, 200, 20)
    check_step_parity(V, [img, jnt], [True, False], [50.0, 1.0], 8.0, "relu", 256, dtype, steps=1)


def test_conv_plan_is_implicit_gemm(V, monkeypatch):
    """with every product implicit (AVAE_IMPL_POLICY below) every conv / transposed-conv stage of the bench
    configuration but the one-channel ends (the first conv reads a one-channel image: no 16-byte chunk of channels to stage; the last
    transposed conv writes one: direct kernel) is an implicit GEMM -- no im2col, col2im, overlap-add or scatter launch is left in
    the step, which has at most 24 launches (38 in round 2).  The DEFAULT policy keeps the transposed direction on round 2's routes,
    where they do a quarter of the work (29 launches, faster: avae_host.hip::plan_memory); both are parity-tested below."""
    import ctypes as C
    monkeypatch.setenv("AVAE_IMPL_POLICY", "E:fwb,H:fwb,D1:fwb,DT:fwb")
    img = dict(make_arch("image", 784, 16, 64, 20), hidden_conv=True, n_hidden_gener_1=64, n_hidden_gener_2=16)
    jnt = make_arch("joint", 147, 200, 200, 20)
    rng = np.random.default_rng(2)
    X = synth_batch(rng, 256, [784, 147], [True, False])
    m = V.AssocVariationalAutoEncoder([img, jnt], binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, batch_size=256,
                                      compute_dtype="bf16", seed=1)
    m._L.avae_timing_enable(m._h, 1)
    m.partial_fit(X, return_cost=False)
    buf = C.create_string_buffer(1 << 16)
    m._L.avae_timing_report(m._h, buf, len(buf))
    m._L.avae_timing_enable(m._h, 0)
    names = [ln.split()[0] for ln in buf.value.decode().splitlines() if not ln.startswith("_null")]
    helpers = [n for n in names if any(k in n for k in ("col2im", "overlap", "scatter", "rowsum")) or (n.endswith("_im2col") and n != "conv_enc1_im2col")]
    assert not helpers, helpers
    assert len(names) <= 24, (len(names), names)


@pytest.mark.parametrize("nz", [33, 64])
@pytest.mark.parametrize("policy", ["", "E:fwb,H:fwb,D1:fwb,DT:fwb"])
def test_conv_branch_with_wide_latents(V, monkeypatch, nz, policy):
    """2 n_z > 64: the head and latent-dgrad launches run on the 128-column tiles, which carry no implicit-GEMM gather; the planner
    has to keep the conv heads' forward and the first decoder stage's latent gradient on their explicit routes there (it threw
    "an implicit patch matrix on a tile configuration without the gather" -- found by tools/fuzz_parity.py conv)."""
    if policy:
        monkeypatch.setenv("AVAE_IMPL_POLICY", policy)
    archs = [dict(make_arch("image", 784, 16, 64, nz), hidden_conv=True, n_hidden_gener_1=64, n_hidden_gener_2=16),
             make_arch("joint", 147, 60, 40, nz)]
    check_step_parity(V, archs, [True, False], [3.0, 1.0], 0.3, "relu", 17, "fp32", steps=2, drift_tol=2.5e-3, grad_every_step=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_conv_only_model(V, dtype):
    """A single conv modality (no MLP modality at all, no association term)."""
    img = dict(make_arch("image", 784, 8, 12, 6), hidden_conv=True, n_hidden_gener_1=12, n_hidden_gener_2=6)
    check_step_parity(V, [img], True, 1.0, 1.0, "relu", 10, dtype, steps=2, grad_every_step=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_conv_modalities_mixed_paths(V, dtype):
    """Two conv modalities in one model (every conv helper launch carries two segments) with depths that take
    different routes: generator depths 144/8 give a 72-channel transposed conv (patch-matrix path: more than 64
    output channels) next to adjoint-frame and direct one-channel stages; 20/12 keeps channel counts that are
    not multiples of 4 on one stage (scalar gather paths) and multiples on the others."""
    a = dict(make_arch("img_a", 784, 8, 24, 5), hidden_conv=True, n_hidden_gener_1=144, n_hidden_gener_2=8)
    b = dict(make_arch("img_b", 784, 4, 16, 5), hidden_conv=True, n_hidden_gener_1=20, n_hidden_gener_2=12)
    check_step_parity(V, [a, b], [True, True], [2.0, 1.0], 0.5, "relu", 12, dtype, steps=2, grad_every_step=True)


def _plan(V, monkeypatch, capfd, archs, binary, act, B, dtype, seed=5):
    rng = np.random.default_rng(seed)
    X = synth_batch(rng, B, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((B, archs[0]["n_z"])).astype(np.float32)
    return step_plan(V, monkeypatch, capfd, archs, B, dtype, X, eps, binary=binary, transfer_fct=act, seed=seed)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_large_tile_path(V, monkeypatch, capfd, dtype):
    """Wide-ish layers at a large batch.  softplus, not relu: with 2048 x 384 hidden units some pre-activation lands within fp32
    rounding of the relu kink and flips its derivative between the fp32 kernel and the fp64 oracle, which is not a kernel error.
    The plan dump shows that this shape does NOT reach the 128x128 tiles it was written for (its largest launch, fwd_out_loss,
    has 144 of the 192 tiles cfg 1 needs): every GEMM launch runs on 64x64 or smaller tiles.  test_large_tile_path_128 is the
    shape that does."""
    archs = [make_arch("a", 784, 0, 0, 32, n_hidden=[512, 384]), make_arch("b", 147, 0, 0, 32, n_hidden=[384, 256])]
    plan = _plan(V, monkeypatch, capfd, archs, [True, False], "softplus", 2048, dtype)
    assert all(c in (0, 3, 5, 7, 9, 10, 11, 12) for _n, c, _i in plan), [(n, c) for n, c, _i in plan]
    check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", 2048, dtype, steps=2, grad_every_step=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_large_tile_path_128(V, monkeypatch, capfd, dtype):
    """The 128x128 tiles (cfg 1) on NT launches (forward into and dgrad of the 768-wide layers: 2 x 16 x 6 = 192 tiles of 128x128,
    96 of 256x128) at
    a batch that is not a multiple of any tile height (2000 = 15 x 128 + 80) and fan-ins that are not multiples of the K tile
    (785, 148): the plan is asserted, then parity at every step."""
    archs = [make_arch("a", 784, 0, 0, 32, n_hidden=[768, 384]), make_arch("b", 147, 0, 0, 32, n_hidden=[768, 256])]
    B = 2000
    plan = _plan(V, monkeypatch, capfd, archs, [True, False], "softplus", B, dtype)
    cfg, items = [(c, it) for n, c, it in plan if n == "fwd_enc1"][0]
    assert cfg == 1 and [(k, M, N) for k, M, N, _K in items] == [(0, B, 768), (0, B, 768)], (cfg, items)
    dgrad = [it for n, c, its in plan if c == 1 for it in its if it[0] == 4]      # K_DGRAD_HIDDEN into the 768-wide layers
    assert dgrad and all((M, N) == (B, 768) for _k, M, N, _K in dgrad), [(n, c) for n, c, _i in plan]
    check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", B, dtype, steps=2, grad_every_step=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_tile_path(V, monkeypatch, capfd, dtype):
    """Launches with >= 192 tiles of 256x128 run the 8-wave kernel (hidden-layer forward / dgrad and plain weight
    gradients of the big nets, unfused Adam): parity at that size, softplus for the reason given above.  The plan dump must show
    the 8-wave NT/TN tiles (cfg 2) and the 8-wave loss tiles (cfg 6)."""
    archs = [make_arch("a", 784, 0, 0, 16, n_hidden=[1024, 768]), make_arch("b", 147, 0, 0, 16, n_hidden=[1024, 768])]
    plan = _plan(V, monkeypatch, capfd, archs, [True, False], "softplus", 4096, dtype)
    cf = {n: c for n, c, _i in plan}
    wide_wgrad = [c for n, c, _i in plan if n.startswith("wgrad")][0]          # (wide products first: "wgrad" or "wgrad1")
    assert cf["fwd_enc1"] == 2 and cf["fwd_out_loss"] == 6 and wide_wgrad == 2, cf
    assert 12 not in cf.values(), cf
    check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", 4096, dtype, steps=1, grad_every_step=True)


@pytest.mark.parametrize("env", [{"AVAE_TN_G": "2"}, {"AVAE_TN_G": "8"}, {"AVAE_NO_TN_BALANCE": "1"}, {"AVAE_NO_BIAS_MFMA": "1"},
                                 {"AVAE_NO_256": "1"}])
def test_planner_switches_big_launches(V, monkeypatch, env):
    """The planner's A/B switches (read by avae_create) select other routes through the same kernels -- other XCD groupings of
    the weight-gradient entries (8 leaves holes in the entry table), plan-order entries, bias rows as tile rows, 128x128
    tiles -- and every route must give the same parity."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    archs = [make_arch("a", 784, 0, 0, 16, n_hidden=[1024, 768]), make_arch("b", 147, 0, 0, 16, n_hidden=[1024, 768])]
    check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", 4096, "bf16", steps=1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_lean_small_tile_kernel(V, monkeypatch, dtype):
    """The chain's hidden-layer launches of small nets run on k_small (32x32 tiles, kind and transfer function at compile time,
    register epilogue); AVAE_NO_LEAN=1 keeps them on k_grouped's 32x32 instance.  Both pass the oracle parity and agree bitwise
    (same tiles, same K order, same rounding points); relu and softplus, a partial last row tile."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    for act in ("relu", "softplus", "tanh"):
        monkeypatch.delenv("AVAE_NO_LEAN", raising=False)
        on, _e, X, eps = check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, act, 100, dtype, steps=1)
        monkeypatch.setenv("AVAE_NO_LEAN", "1")
        off, _e, X, eps = check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, act, 100, dtype, steps=1)
        assert np.array_equal(on.get_grads(), off.get_grads()) and np.array_equal(on.get_params(), off.get_params()), act


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("hidden", [(500, 500), (24, 24), (130, 70)])
def test_fused_adam_launch_is_bitwise(V, monkeypatch, dtype, hidden):
    """The small nets' weight-gradient launch with Adam in its epilogue (k_small_tn<.., ADAM>: interior tiles on whole 16-byte stores,
    edge tiles with row bounds and a partial last quad (147 = 36 quads + 3), every XCD running its own list of layers) against (a)
    the same launch on the plain tile order (AVAE_NO_XCD_PIECES=1) and (b) the unfused pair k_grouped + k_adam
    (AVAE_NO_ADAM_FUSE=1): parameters, both moments and the last gradient bitwise after 4 steps -- the moments and the compute-dtype
    shadows of step s are what step s+1 runs on, so a stale shadow column (a hipcc store-merging miscompile once produced one in
    fp32) shows up from the second step on."""
    archs = [make_arch("image", 784, hidden[0], hidden[1], 20), make_arch("joint", 147, max(8, hidden[0] // 2), max(8, hidden[1] // 2), 20)]
    B = 64
    rng = np.random.default_rng(5)
    X = synth_batch(rng, 4 * B, [784, 147], [True, False])
    res = []
    for env in ({}, {"AVAE_NO_XCD_PIECES": "1"}, {"AVAE_NO_ADAM_FUSE": "1"}):
        for k in ("AVAE_NO_XCD_PIECES", "AVAE_NO_ADAM_FUSE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, batch_size=B,
                                          compute_dtype=dtype, seed=1)
        costs = [m.partial_fit([x[i * B:(i + 1) * B] for x in X]) for i in range(4)]
        mo, vo, step = m.get_opt_state()
        assert shadow_err(m)[:2] == (0.0, 0.0), env
        res.append((np.array(costs), m.get_params(), mo, vo, m.get_grads()))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [256, 100, 37])
def test_chain2_experiment_is_bitwise(V, monkeypatch, dtype, B):
    """VERDICT r2 #6 (AVAE_CHAIN2=1): fwd_enc1 -> fwd_enc2 in ONE launch behind a row-block-local hand-off (write-through stores, a
    ticket per row block, sc1 loads) instead of a kernel boundary: the same tiles, K order and rounding points -- bitwise the two
    launches' results, at the bench batch (8 row blocks = 8 XCDs) and at batches whose row blocks do not line up with the XCDs."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    rng = np.random.default_rng(11)
    X = synth_batch(rng, 20 * B, [784, 147], [True, False])
    res = []
    for on in (False, True):
        if on:
            monkeypatch.setenv("AVAE_CHAIN2", "1")
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, batch_size=B,
                                          compute_dtype=dtype, seed=1)
        c0 = m.partial_fit([x[:B] for x in X])
        m.partial_fit_steps([x[B:] for x in X], 19, return_cost=False)
        res.append((c0, m.cost_history(20).copy(), m.get_params()))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nz", [32, 31, 5])
def test_lean_head_kernels(V, monkeypatch, dtype, nz):
    """The two fused head launches of small nets on the lean frame (k_small_head: [mu | lv] -> z -> decoder's first layer;
    k_small_latb: dz -> [dmu | dlv] -> heads' input gradient, with the step's cost item) against k_grouped's 32x64 instance
    (AVAE_NO_LEAN_HEAD=1): oracle parity on both routes, bitwise equal to each other.  n_z = 32 fills the 64-column tile (and makes
    [z | 1] two K tiles of fp32), 31 is odd (unaligned dlv columns), 5 leaves most of the tile empty; a partial last row tile."""
    archs = [make_arch("image", 300, 0, 0, nz, n_hidden=[96, 72]), make_arch("joint", 47, 0, 0, nz, n_hidden=[40])]
    on, _e, X, eps = check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", 70, dtype, steps=2)
    monkeypatch.setenv("AVAE_NO_LEAN_HEAD", "1")
    off, _e, X, eps = check_step_parity(V, archs, [True, False], [5.0, 1.0], 0.5, "softplus", 70, dtype, steps=2)
    assert np.array_equal(on.get_grads(), off.get_grads()) and np.array_equal(on.get_params(), off.get_params())
    assert np.array_equal(on.cost_history(2), off.cost_history(2))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [256, 100])
def test_tail_product_route(V, monkeypatch, dtype, B):
    """Small nets: the decoder's first layer rides in the heads' launch and the heads' input gradient in bwd_dec1_latent's (the
    tail product of the 32x64 head tiles, avae_host.hip::fuse_tail).  Default route = tail on; AVAE_NO_TAIL=1 = the four
    separate launches.  Both pass the oracle parity, and they agree with each other bitwise after a step (same products,
    same K order, same rounding points).  B = 100: a last, partial row tile."""
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    on, _e, _X, _eps = check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, dtype, steps=1)
    import ctypes as C
    L, h = on._L, on._h
    assert L.avae_timing_enable(h, 1) == 0
    on.partial_fit(_X, _eps[0])
    buf = C.create_string_buffer(1 << 16)
    assert L.avae_timing_report(h, buf, len(buf)) == 0 and L.avae_timing_enable(h, 0) == 0
    names = [ln.split()[0] for ln in buf.value.decode().splitlines()]
    monkeypatch.setenv("AVAE_NO_TAIL", "1")
    off, _e, _X, _eps = check_step_parity(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, dtype, steps=1)
    off.partial_fit(_X, _eps[0])             # (the second step `on` took under the timer)
    assert np.array_equal(on.get_grads(), off.get_grads())
    assert np.array_equal(on.get_params(), off.get_params())
    assert "fwd_head+fwd_dec1" in names, names
    assert "bwd_dec1_latent+bwd_head" in names, names      # ([dmu | dlv] = 40 columns: one 128-byte K tile of bf16, two of fp32)


@pytest.mark.parametrize("env", [{"AVAE_NO_THIN": "1"}, {"AVAE_NO_ADJ": "1"}, {"AVAE_NO_THIN": "1", "AVAE_NO_ADJ": "1"}, {"AVAE_NO_SINK": "1"}, {"AVAE_NO_SUMS_MERGE": "1"}, {"AVAE_NO_WADJ_FOLD": "1"},
                                 {"AVAE_NO_IMPLICIT": "1"}, {"AVAE_NO_IMPLICIT": "1", "AVAE_NO_THIN": "1"}, {"AVAE_NO_IMPLICIT": "1", "AVAE_NO_ADJ": "1"},
                                 {"AVAE_NO_IMPLICIT": "1", "AVAE_NO_WADJ_FOLD": "1"}, {"AVAE_NO_IMPLICIT": "1", "AVAE_NO_SUMS_MERGE": "1"},
                                 {"AVAE_IMPL_POLICY": "E:fwb,H:fwb,D1:fwb,DT:fwb"}, {"AVAE_IMPL_POLICY": "E:fw,H:fwb,D1:fwb,DT:b"},
                                 {"AVAE_IMPL_POLICY": "E:fw,H:fwb,D1:fwb,DT:wb"}, {"AVAE_IMPL_POLICY": "E:b,H:b,D1:b,DT:w"},
                                 {"AVAE_IMPL_POLICY": "E:fwb,H:fwb,D1:fwb,DT:fwb", "AVAE_NO_THIN": "1"},
                                 {"AVAE_NO_THIN_FAST": "1"}, {"AVAE_THIN_FAST_SPLIT": "2,2,2"}, {"AVAE_THIN_FAST_SPLIT": "4,1,4"}])
def test_planner_switches_conv_routes(V, monkeypatch, env):
    """Conv stages through the patch-matrix route instead of the direct / adjoint-frame ones; the MLP modality's hidden layers as
    launches of their own instead of riding in the conv modality's GEMM launches (AVAE_NO_SINK); the sums behind the weight
    gradients as k_colsum + k_reduce + k_gperm launches instead of one k_sums launch (AVAE_NO_SUMS_MERGE); the adjoint filter
    shadows by a k_wadj launch instead of by k_adam's pass (AVAE_NO_WADJ_FOLD): same parity."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img = dict(make_arch("image", 784, 8, 24, 6), hidden_conv=True, n_hidden_gener_1=24, n_hidden_gener_2=8)
    jnt = make_arch("joint", 147, 40, 32, 6)
    check_step_parity(V, [img, jnt], [True, False], [5.0, 1.0], 0.5, "relu", 12, "fp32", steps=1)


def test_graph_replay_equals_eager(V):
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    rng = np.random.default_rng(3)
    X = synth_batch(rng, 256, [784, 147], [True, False])
    eps = rng.standard_normal((4, 256, 20)).astype(np.float32)
    present = rng.random((4, 256, 2)) < 0.6             # the masked plan: its graphs against its eager path
    for P in (None, present):
        res = []
        for use_graph in (True, False):
            m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                              batch_size=256, compute_dtype="bf16", seed=1, use_graph=use_graph)
            costs = [m.partial_fit(X, eps[s], present=None if P is None else P[s]) for s in range(4)]
            res.append((costs, m.get_params()))
        assert res[0][0] == res[1][0], "graph and eager costs differ (kernels are deterministic)"
        assert np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("given_eps", [False, True])
def test_train_steps_equals_single_steps(V, given_eps):
    """avae_train_steps (16 or 4 steps per graph replay, all their batches staged by one launch, each executable's staging node
    re-pointed with hipGraphExecKernelNodeSetParams while its previous replay is still queued) is exactly n successive
    avae_train_step calls: bitwise equal costs and weights."""
    archs = [make_arch("image", 784, 64, 48, 8), make_arch("joint", 147, 40, 32, 8)]
    rng = np.random.default_rng(9)
    n, B = 41, 32                                          # 16 + 16 + 4 + 4 + 1: every multi-step executable is re-pointed and
                                                           # replayed twice back to back, with no synchronise in between
    data = np.concatenate(synth_batch(rng, n * B, [784, 147], [True, False]), axis=1)
    dev = torch.as_tensor(data).cuda()
    X = [dev[:, :784], dev[:, 784:]]                       # column slices of one matrix: row stride 931
    eps = torch.as_tensor(rng.standard_normal((n * B, 8)).astype(np.float32)).cuda() if given_eps else None
    res = []
    for many in (False, True):
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          batch_size=B, compute_dtype="bf16", seed=4)
        if many:
            last = m.partial_fit_steps(X, n, eps)
        else:
            for i in range(n):
                last = m.partial_fit([x[i * B:(i + 1) * B] for x in X], None if eps is None else eps[i * B:(i + 1) * B],
                                     return_cost=i == n - 1)
        res.append((last, m.cost_history(n).copy(), m.get_params()))
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and len(set(res[0][1].tolist())) == n      # n different batches, n different costs
    assert np.array_equal(res[0][2], res[1][2])
    with pytest.raises(ValueError):
        m.partial_fit_steps([x[:B] for x in X], 2)         # rows must be batch_size x n_steps


def test_train_steps_with_conv_modality(V):
    """The staging-set relocation of the multi-step replays also covers the conv branch (its first im2col reads the
    staged image): a run of 41 batches (replays of 16, 16, 4, 4 steps + a single step) equals 41 single steps, bitwise."""
    img = dict(make_arch("image", 784, 8, 16, 6), hidden_conv=True, n_hidden_gener_1=16, n_hidden_gener_2=8)
    jnt = make_arch("joint", 147, 24, 16, 6)
    rng = np.random.default_rng(13)
    n, B = 41, 8                                            # 16 + 16 + 4 + 4 + 1, as above
    data = np.concatenate(synth_batch(rng, n * B, [784, 147], [True, False]), axis=1)
    dev = torch.as_tensor(data).cuda()
    X = [dev[:, :784], dev[:, 784:]]
    res = []
    for many in (False, True):
        m = V.AssocVariationalAutoEncoder([img, jnt], binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          batch_size=B, compute_dtype="bf16", seed=2)
        if many:
            m.partial_fit_steps(X, n)
        else:
            for i in range(n):
                m.partial_fit([x[i * B:(i + 1) * B] for x in X])
        res.append((m.cost_history(n).copy(), m.get_params()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ----------------------------------------------------------------------------- inference surface
def test_transform_generate_reconstruct_rows(V):
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)]
    B = 64
    model, ref = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32")
    rng = np.random.default_rng(8)
    for rows in (1, 7, 64, 65, 150):               # below, at and above batch_size (chunked), ragged tail
        X = synth_batch(rng, rows, [784, 147], [True, False])
        mus, rmu = model.transform(X), ref.transform(X)
        one = model.transform(X[1], sens_idx=1)
        assert np.abs(one - rmu[1]).max() <= 1e-5 * max(1, np.abs(rmu[1]).max())
        z = rng.standard_normal((rows, 20)).astype(np.float32)
        gen, rgen = model.generate(z), ref.generate(z)
        e = [rng.standard_normal((rows, 20)).astype(np.float32) for _ in range(2)]
        rec, rrec = model.reconstruct(X, eps=e), ref.reconstruct(X, eps=e)
        for m in range(2):
            assert mus[m].shape == (rows, 20) and gen[m].shape == (rows, archs[m]["n_input"])
            assert np.abs(mus[m] - rmu[m]).max() <= 1e-5 * max(1, np.abs(rmu[m]).max())
            assert np.abs(gen[m] - rgen[m]).max() <= 1e-5 * max(1, np.abs(rgen[m]).max())
            assert np.abs(rec[m] - rrec[m]).max() <= 1e-5 * max(1, np.abs(rrec[m]).max())
    # empty input
    assert model.transform(np.zeros((0, 147), np.float32), sens_idx=1).shape == (0, 20)
    # torch tensors in -> torch tensors out, on the device
    xt = torch.as_tensor(X[0]).cuda()
    out = model.transform(xt, sens_idx=0)
    assert torch.is_tensor(out) and out.is_cuda
    # generate() with no argument draws batch_size rows from numpy's RNG (vae_assoc.py:412-414)
    np.random.seed(0)
    g0 = model.generate()
    np.random.seed(0)
    zz = np.random.normal(size=(B, 20))
    assert g0[0].shape == (B, 784) and np.abs(g0[1] - ref.generate(zz)[1]).max() <= 1e-4
    # cross-modal inference pattern of the reference's callers (baxter_vae_assoc_writer.py:426-432)
    z_rep = model.transform([X[0], np.zeros_like(X[1])])
    jnt = model.generate(z_mu=z_rep[0])[1]
    assert np.abs(jnt - ref.generate(ref.transform([X[0], np.zeros_like(X[1])])[0])[1]).max() <= 1e-4
    # training right after inference still matches (inference must not disturb the zero padding)
    Xb = synth_batch(rng, B, [784, 147], [True, False])
    eb = rng.standard_normal((B, 20)).astype(np.float32)
    c, cr = model.partial_fit(Xb, eb), ref.partial_fit(Xb, eb)
    assert abs(c - cr) <= 1e-5 * abs(cr)
    assert np.abs(model.get_params() - ref.get_params()).max() <= 2e-5


@pytest.mark.parametrize("env", [{}, {"AVAE_NO_TAIL": "1"}, {"AVAE_NO_LEAN": "1"}])
def test_generate_serving_buckets(V, monkeypatch, env):
    """avae_generate (per call: k_serve_in, which also runs the decoder's first layer as its tail product and publishes the call's
    slot, then the remaining decoder launches of every modality, eagerly, whose output launch stores straight into the caller's
    buffers; AVAE_NO_LEAN=1: the same staging launch on k_grouped + one graph replay of the rest; AVAE_NO_TAIL=1: plain staging
    kernel + all decoder launches in the graph): row counts on both sides of the 64-row serving bucket and of batch_size (chunked),
    interleaved with training steps that use the same activation buffers; fp32 against the oracle, bf16 bitwise against the
    per-modality avae_decode path."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)]
    B = 160
    model, ref = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32")
    rng = np.random.default_rng(18)
    for rows in (1, 3, 64, 65, 160, 161, 400):
        z = rng.standard_normal((rows, 20)).astype(np.float32)
        gen, rgen = model.generate(z), ref.generate(z)
        for m in range(2):
            assert gen[m].shape == (rows, archs[m]["n_input"])
            assert np.abs(gen[m] - rgen[m]).max() <= 1e-5 * max(1, np.abs(rgen[m]).max()), (rows, m)
        if rows == 64:          # a training step in between must see intact padding / constant-1 columns
            Xb = synth_batch(rng, B, [784, 147], [True, False])
            eb = rng.standard_normal((B, 20)).astype(np.float32)
            c, cr = model.partial_fit(Xb, eb), ref.partial_fit(Xb, eb)
            assert abs(c - cr) <= 1e-5 * abs(cr)
    mb = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=B, compute_dtype="bf16", seed=3)
    for rows in (5, 64, 200):
        z = torch.as_tensor(rng.standard_normal((rows, 20)).astype(np.float32)).cuda()
        gen = mb.generate(z)
        for m in range(2):
            o = torch.empty((rows, archs[m]["n_input"]), dtype=torch.float32, device="cuda")
            assert mb._L.avae_decode(mb._h, m, z.data_ptr(), rows, o.data_ptr(), mb._stream()) == 0
            assert torch.equal(gen[m], o), (rows, m)


@pytest.mark.parametrize("B", [100, 33, 7])
def test_generate_serving_odd_batch_sizes(V, B):
    """The serving path (staging launch with the decoder's first layer as its tail product, 32-row tiles) with batch sizes that are
    not multiples of 32 and smaller than the 64-row bucket: bitwise the per-modality avae_decode path, both dtypes."""
    archs = [make_arch("image", 784, 96, 80, 12), make_arch("joint", 147, 40, 24, 12)]
    rng = np.random.default_rng(41)
    for dtype in ("fp32", "bf16"):
        mb = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="softplus", batch_size=B, compute_dtype=dtype, seed=4)
        for rows in (1, B - 1, B, B + 1, 3 * B + 2):
            if rows < 1:
                continue
            z = torch.as_tensor(rng.standard_normal((rows, 12)).astype(np.float32)).cuda()
            gen = mb.generate(z)
            for m in range(2):
                o = torch.empty((rows, archs[m]["n_input"]), dtype=torch.float32, device="cuda")
                assert mb._L.avae_decode(mb._h, m, z.data_ptr(), rows, o.data_ptr(), mb._stream()) == 0
                assert torch.equal(gen[m], o), (dtype, B, rows, m)


@pytest.mark.parametrize("nz", [33, 48, 63])
def test_generate_serving_wide_latents(V, nz):
    """the lean per-call serving launch (k_serve_in) stages EVERY latent column -- 32 < n_z <= 63 takes two trips
    of its 8 threads x 4 columns per row.  fp32 against the oracle, bf16 bitwise against the per-modality avae_decode path (whose
    staging kernel loops over all n_z), rows on both sides of the 64-row bucket."""
    archs = [make_arch("image", 784, 96, 80, nz), make_arch("joint", 147, 40, 24, nz)]
    B = 96
    rng = np.random.default_rng(nz)
    model, ref = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32")
    for rows in (1, 33, 64, 65, 200):
        z = rng.standard_normal((rows, nz)).astype(np.float32)
        z[:, 32:] *= 3.0                    # the columns the round-2 kernel dropped carry weight
        gen, rgen = model.generate(z), ref.generate(z)
        for m in range(2):
            assert np.abs(gen[m] - rgen[m]).max() <= 1e-5 * max(1, np.abs(rgen[m]).max()), (rows, m)
    mb = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="softplus", batch_size=B, compute_dtype="bf16", seed=4)
    for rows in (2, 64, 97):
        z = torch.as_tensor(rng.standard_normal((rows, nz)).astype(np.float32)).cuda()
        gen = mb.generate(z)
        for m in range(2):
            o = torch.empty((rows, archs[m]["n_input"]), dtype=torch.float32, device="cuda")
            assert mb._L.avae_decode(mb._h, m, z.data_ptr(), rows, o.data_ptr(), mb._stream()) == 0
            assert torch.equal(gen[m], o), (nz, rows, m)


def test_strided_modalities_from_one_matrix(V):
    """train() hands column slices of one [B, 931] matrix (vae_assoc.py:510,543): no copies."""
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)]
    B = 50
    model, ref = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32")
    rng = np.random.default_rng(1)
    X = synth_batch(rng, B, [784, 147], [True, False])
    eps = rng.standard_normal((B, 20)).astype(np.float32)
    big = torch.as_tensor(np.concatenate(X, axis=1)).cuda()
    c = model.partial_fit([big[:, :784], big[:, 784:]], eps)
    cr = ref.partial_fit(X, eps)
    assert abs(c - cr) <= 1e-5 * abs(cr)


def test_wrong_shapes_raise(V):
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)]
    model, _ = build_pair(V, archs, [True, False], 1.0, 1.0, "relu", 16, "bf16")
    with pytest.raises(ValueError):
        model.partial_fit([np.zeros((15, 784), np.float32), np.zeros((15, 147), np.float32)])
    with pytest.raises(ValueError):
        model.transform(np.zeros((4, 100), np.float32), sens_idx=0)
    with pytest.raises(ValueError):          # the conv branch is hard-wired to 28x28 / binary
        V.AssocVariationalAutoEncoder([dict(make_arch("x", 100, 4, 4, 20), hidden_conv=True)], batch_size=4)
    with pytest.raises(ValueError):
        V.AssocVariationalAutoEncoder([dict(archs[0], hidden_conv=True)], binary=False, batch_size=4)
    with pytest.raises(ValueError):
        V.AssocVariationalAutoEncoder([archs[0], dict(archs[1], n_z=7)], batch_size=4)


# ----------------------------------------------------------------------------- internal eps stream
def philox4x32_10(c, k):
    c = [np.uint32(x) for x in c]
    k = [np.uint32(x) for x in k]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * np.uint64(c[0])
        p1 = np.uint64(0xCD9E8D57) * np.uint64(c[2])
        c = [np.uint32(p1 >> np.uint64(32)) ^ c[1] ^ k[0], np.uint32(p1 & np.uint64(0xFFFFFFFF)),
             np.uint32(p0 >> np.uint64(32)) ^ c[3] ^ k[1], np.uint32(p0 & np.uint64(0xFFFFFFFF))]
        k = [np.uint32((int(k[0]) + 0x9E3779B9) & 0xFFFFFFFF), np.uint32((int(k[1]) + 0xBB67AE85) & 0xFFFFFFFF)]
    return [int(x) for x in c]


def fetch(model, name, shape):
    import ctypes as C
    buf = np.empty(int(np.prod(shape)), dtype=np.float32)
    cnt = C.c_size_t(0)
    assert model._L.avae_debug_fetch(model._h, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt)) == 0
    return buf[:cnt.value].reshape(shape)


def test_internal_eps_is_philox_normal_and_shard_consistent(V):
    archs = [make_arch("image", 784, 32, 24, 20), make_arch("joint", 147, 24, 16, 20)]
    B = 512
    rng = np.random.default_rng(0)
    X = synth_batch(rng, B, [784, 147], [True, False])
    m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=B, compute_dtype="bf16", seed=77)
    m.partial_fit(X)                              # eps=None -> internal stream, step 0
    e0 = fetch(m, "eps", (B, 20)).copy()
    m.partial_fit(X)
    e1 = fetch(m, "eps", (B, 20)).copy()
    assert abs(e0.mean()) < 0.05 and abs(e0.std() - 1) < 0.05 and not np.array_equal(e0, e1)
    # documented generator: counter (global row, dim quad, step lo, step hi ^ salt), key = seed; Box-Muller
    salt = 0x7261696E
    for (row, q) in ((0, 0), (5, 3), (511, 4)):
        r = philox4x32_10([row, q, 0, salt & 0xFFFFFFFF], [77, 0])
        u = [((x >> 8) + 0.5) / 16777216.0 for x in r]
        want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
                np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])]
        assert np.allclose(e0[row, 4 * q:4 * q + 4], want, atol=2e-4), (row, q, e0[row, 4 * q:4 * q + 4], want)
    # a replica that owns global rows [256, 512) draws the same numbers for them (data-parallel consistency)
    from vae_assoc_amd import _capi
    half = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=256, compute_dtype="bf16", seed=77)
    half._L.avae_destroy(half._h)
    half._cfg.row_offset = 256
    half._cfg.batch_global = 512
    import ctypes as C
    h = C.c_void_p()
    _capi.check(None, half._L.avae_create(C.byref(half._cfg), C.byref(h)), "avae_create")
    half._h = h
    half.set_params(m.get_params())
    half.partial_fit([x[256:] for x in X], return_cost=False)
    assert np.array_equal(fetch(half, "eps", (256, 20)), e0[256:])


def test_internal_eps_is_fresh_per_call_modality_and_chunk(V):
    """with eps=None every evaluate_cost / reconstruct call draws its own noise, as each sess.run of the reference
    does (vae_assoc.py:90, 388-391, 421-425): different across calls with no training step in between, across modalities, and
    across the batch_size-row chunks of a long input; and it is N(0,1).  The decoder of an IDENTITY-like probe is not available,
    so the noise is read back through the library's eps buffer (last chunk) and through its effect on the outputs."""
    archs = [make_arch("image", 784, 32, 24, 20), make_arch("joint", 147, 24, 16, 20)]
    B = 256
    rng = np.random.default_rng(2)
    m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=B, compute_dtype="fp32", seed=5)
    X = synth_batch(rng, B, [784, 147], [True, False])
    # evaluate_cost twice with no step in between: two draws
    m.evaluate_cost(X)
    e0 = fetch(m, "eps", (B, 20)).copy()
    c1 = m.evaluate_cost(X)
    e1 = fetch(m, "eps", (B, 20)).copy()
    assert not np.array_equal(e0, e1) and abs(np.corrcoef(e0.ravel(), e1.ravel())[0, 1]) < 0.05
    for e in (e0, e1):
        assert abs(e.mean()) < 0.05 and abs(e.std() - 1) < 0.05
    assert m.evaluate_cost(X) != c1
    # reconstruct: a draw per modality (the eps buffer holds the LAST modality's after the call) and per call
    same = [X[1], X[1]]                                    # feed modality 1's rows to a model with two identical joint branches
    twin = V.AssocVariationalAutoEncoder([archs[1], dict(archs[1], scope="joint2")], binary=[False, False], transfer_fct="relu",
                                         batch_size=B, compute_dtype="fp32", seed=5)
    p = twin.get_params()
    half = p.size // 2
    p[half:] = p[:half]                                    # same weights in both branches: outputs differ only through eps
    twin.set_params(p)
    r1 = twin.reconstruct(same)
    assert np.abs(r1[0] - r1[1]).max() > 1e-3, "both modalities reconstructed with the same noise"
    r2 = twin.reconstruct(same)
    assert np.abs(r1[0] - r2[0]).max() > 1e-3, "two reconstruct calls drew the same noise"
    # rows beyond batch_size: chunk 2 must not repeat chunk 1's noise (same input rows in both chunks -> outputs would be equal)
    long = [np.concatenate([X[1], X[1]]), np.concatenate([X[1], X[1]])]
    r3 = twin.reconstruct(long)
    assert np.abs(r3[0][:B] - r3[0][B:]).max() > 1e-3, "rows r and r + batch_size got identical noise"
    # explicit eps is still honoured exactly
    eg = rng.standard_normal((2 * B, 20)).astype(np.float32)
    r4, r5 = twin.reconstruct(long, eps=[eg, eg]), twin.reconstruct(long, eps=[eg, eg])
    assert np.array_equal(r4[0], r5[0]) and np.array_equal(r4[0], r4[1])
    # the training stream is untouched by the draws above (documented counter layout, checked in the test before this one)
    m.partial_fit(X)
    want = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=B, compute_dtype="fp32", seed=5)
    want.partial_fit(X)
    assert np.array_equal(fetch(m, "eps", (B, 20)), fetch(want, "eps", (B, 20)))


# ----------------------------------------------------------------------------- data-parallel property on one GPU
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_shard_replicas_sum_to_global_batch(V, dtype):
    """Size-independent property at the BENCH size: two replicas with B_loc=256, B_global=512 (built
    through the C ABI with row_offset / batch_global) produce gradients whose SUM equals the
    single-replica B=512 gradient -- the data-parallel contract of SURVEY.md 8e."""
    import ctypes as C
    from vae_assoc_amd import _capi
    archs = [make_arch("image", 784, 500, 500, 20), make_arch("joint", 147, 200, 200, 20)]
    rng = np.random.default_rng(12)
    X = synth_batch(rng, 512, [784, 147], [True, False])
    eps = rng.standard_normal((512, 20)).astype(np.float32)
    kw = dict(binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, compute_dtype=dtype, seed=2)
    full = V.AssocVariationalAutoEncoder(archs, batch_size=512, **kw)
    p0 = full.get_params()
    full._backward(X, eps)
    g_full = full._grad_tensor().clone()
    gsum = torch.zeros_like(g_full)
    for r in range(2):
        rep = V.AssocVariationalAutoEncoder(archs, batch_size=256, **kw)
        rep._L.avae_destroy(rep._h)
        rep._cfg.row_offset, rep._cfg.batch_global = 256 * r, 512
        h = C.c_void_p()
        _capi.check(None, rep._L.avae_create(C.byref(rep._cfg), C.byref(h)), "avae_create")
        rep._h = h
        rep.set_params(p0)
        rep._backward([x[256 * r:256 * (r + 1)] for x in X], eps[256 * r:256 * (r + 1)])
        assert rep._grad_tensor().shape == g_full.shape
        gsum += rep._grad_tensor()
    torch.cuda.synchronize()
    gf, gs = g_full.cpu().numpy().astype(np.float64), gsum.cpu().numpy().astype(np.float64)
    cost_full, cost_sum = gf[-1], gs[-1]
    assert abs(cost_full - cost_sum) <= 1e-5 * abs(cost_full)
    # gradients agree to accumulation-order rounding (K = 512 in one product vs 256 + 256)
    assert np.abs(gf[:-1] - gs[:-1]).max() <= (2e-5 if dtype == "fp32" else 2e-3) * np.abs(gf[:-1]).max()


# ----------------------------------------------------------------------------- checkpoint, history, train()
def test_save_restore_roundtrip(V, tmp_path, capsys):
    archs = [make_arch("image", 784, 32, 24, 4), make_arch("joint", 147, 24, 16, 4)]
    B = 32
    rng = np.random.default_rng(4)
    X = synth_batch(rng, B, [784, 147], [True, False])
    eps = rng.standard_normal((4, B, 4)).astype(np.float32)
    a, _ = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32")
    for s in range(2):
        a.partial_fit(X, eps[s])
    folder = str(tmp_path)
    a.save_model(os.path.join(folder, "m.ckpt"))
    b, _ = build_pair(V, archs, [True, False], [50.0, 1.0], 8.0, "relu", B, "fp32", seed=99)
    b.restore_model(folder=folder)                       # newest *.ckpt in the folder
    assert np.array_equal(a.get_params(), b.get_params())
    ma, va, sa = a.get_opt_state()
    mb, vb, sb = b.get_opt_state()
    assert sa == sb == 2 and np.array_equal(ma, mb) and np.array_equal(va, vb)
    ca = [a.partial_fit(X, eps[s]) for s in (2, 3)]
    cb = [b.partial_fit(X, eps[s]) for s in (2, 3)]
    assert ca == cb and np.array_equal(a.get_params(), b.get_params())      # resume is exact
    # reference behaviour: failures print and return, they do not raise (vae_assoc.py:448,459,462)
    b.restore_model(folder=os.path.join(folder, "nope"))
    b.restore_model(folder=folder, fname="missing.ckpt")
    (tmp_path / "bad.ckpt").write_bytes(b"not a checkpoint")
    b.restore_model(folder=folder, fname="bad.ckpt")
    out = capsys.readouterr().out
    assert "Invalid or non-exist model folder." in out and out.count("Invalid or non-exist model file.") >= 2
    c = V.AssocVariationalAutoEncoder([make_arch("image", 784, 16, 8, 4)], batch_size=B, compute_dtype="fp32")
    c.restore_model(folder=folder, fname="m.ckpt")       # architecture mismatch: printed, not raised
    assert "mismatch" in capsys.readouterr().out


def test_train_loop_matches_oracle_loop(V):
    """train() (vae_assoc.py:498-583): same data order, same explicit eps => same avg_cost_hist."""
    from vae_assoc_amd import dataset
    archs = [make_arch("image", 784, 32, 24, 4), make_arch("joint", 147, 24, 16, 4)]
    rng = np.random.default_rng(6)
    N, B = 300, 32
    data = np.concatenate(synth_batch(rng, N, [784, 147], [True, False]), axis=1)
    eps_all = rng.standard_normal((64, B, 4)).astype(np.float32)
    results = []
    for which in ("hip", "oracle"):
        np.random.seed(42)
        ds = dataset.construct_datasets(data.copy())
        if which == "hip":
            # explicit eps through partial_fit: wrap the model class so train() feeds it
            class Fed(V.AssocVariationalAutoEncoder):
                _k = 0

                def partial_fit(self, X, eps=None, return_cost=True):
                    e = eps_all[Fed._k]
                    Fed._k += 1
                    return super().partial_fit(X, e, return_cost)

                def partial_fit_steps(self, X, n_steps, eps=None, return_cost=True):
                    e = np.concatenate(eps_all[Fed._k:Fed._k + n_steps])
                    Fed._k += n_steps
                    return super().partial_fit_steps(X, n_steps, e, return_cost)
            orig = V.AssocVariationalAutoEncoder
            V.AssocVariationalAutoEncoder = Fed
            try:
                model, hist = V.train(ds, archs, binary=[True, False], weights=[50.0, 1.0], assoc_lambda=8.0, batch_size=B,
                                      training_epochs=3, display_step=10, compute_dtype="fp32", seed=8)
            finally:
                V.AssocVariationalAutoEncoder = orig
            p0 = None
            results.append((hist, model.get_params()))
        else:
            p_init = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", batch_size=B,
                                                   compute_dtype="fp32", seed=8).get_params()
            model, hist = O.train(ds, archs, binary=[True, False], weights=[50.0, 1.0], assoc_lambda=8.0, batch_size=B,
                                  training_epochs=3, params_flat=p_init.astype(np.float64), eps_fn=lambda s: eps_all[s])
            results.append((hist, model.get_params()))
    (h_hip, p_hip), (h_ref, p_ref) = results
    assert len(h_hip) == len(h_ref) == 3 * (240 // B)
    assert np.allclose(h_hip, h_ref, rtol=2e-5)
    assert np.abs(p_hip - p_ref).max() <= 5e-5


def test_device_resident_dataset_same_order_and_costs(V):
    """dataset.DeviceDataSet: same batch order as the host DataSet (fixture-pinned to the reference), and
    train() on it gives the same cost history as on host batches."""
    from vae_assoc_amd import dataset
    archs = [make_arch("image", 784, 16, 12, 4), make_arch("joint", 147, 12, 8, 4)]
    rng = np.random.default_rng(6)
    data = np.concatenate(synth_batch(rng, 150, [784, 147], [True, False]), axis=1)
    np.random.seed(5)                                     # the two share numpy's global RNG: run them one after the other
    host = dataset.DataSet(data.copy())
    want = [host.next_batch(32)[0].copy() for _ in range(12)]      # wraps twice over 150 rows
    np.random.seed(5)
    devd = dataset.DeviceDataSet(data.copy())
    for a in want:
        b, _l = devd.next_batch(32)
        assert b.is_cuda and np.array_equal(a, b.cpu().numpy())
    hists = []
    for on_device in (False, True):
        np.random.seed(11)
        ds = dataset.construct_datasets(data.copy())
        if on_device:
            ds = dataset.to_device(ds)
        _m, hist = V.train(ds, archs, binary=[True, False], batch_size=20, training_epochs=2, display_step=10,
                           compute_dtype="fp32", seed=3)
        hists.append(hist)
    assert hists[0] == hists[1]


def test_early_stop_runs(V, capsys):
    from vae_assoc_amd import dataset
    archs = [make_arch("image", 784, 16, 12, 4), make_arch("joint", 147, 12, 8, 4)]
    rng = np.random.default_rng(6)
    data = np.concatenate(synth_batch(rng, 200, [784, 147], [True, False]), axis=1)
    np.random.seed(1)
    ds = dataset.construct_datasets(data)
    model, hist = V.train(ds, archs, binary=[True, False], batch_size=10, training_epochs=4, early_stop=2, display_step=1)
    assert "Validation cost=" in capsys.readouterr().out and len(hist) >= 16 and np.all(np.isfinite(hist))


def test_concurrent_callers_serialise(V):
    """The reference's callers hit one session from a worker thread and the GUI thread
    (baxter_vae_assoc_writer.py:651-673): calls on one handle must serialise, not corrupt."""
    archs = [make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)]
    model, ref = build_pair(V, archs, [True, False], 1.0, 1.0, "relu", 64, "fp32")
    rng = np.random.default_rng(0)
    zs = [rng.standard_normal((64, 20)).astype(np.float32) for _ in range(4)]
    want = [ref.generate(z) for z in zs]
    errs = []

    def worker(i):
        try:
            for _ in range(10):
                out = model.generate(zs[i])
                for m in range(2):
                    if np.abs(out[m] - want[i][m]).max() > 1e-4:
                        errs.append((i, m))
        except Exception as e:      # noqa
            errs.append(repr(e))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs


@pytest.mark.parametrize("act", ["identity", "relu"])
def test_back_to_back_steps_equal_synchronised_steps(V, act):
    """Two single steps submitted back to back, 300 times, against the same two steps with a host synchronisation in between: bitwise.
    The identity activation is the case that matters: act'(y) = 1 lets the compiler drop the loads of y in the kernels that have the
    transfer function at compile time, and k_small_latb's counted waits (written for a fixed number of younger loads) then let a K
    tile be read before it had landed -- about once in 60 steps, found by tools/fuzz_parity.py api as runs that differed from
    themselves (n_z = 32: the 64-column head tile of the lean tail kernel; fp32)."""
    archs = [make_arch("image", 784, 500, 500, 32), make_arch("joint", 147, 200, 200, 32)]
    B, n = 64, 2
    rng = np.random.default_rng(5)
    model, _ref = build_pair(V, archs, [True, False], [1.0, 50.0], 0.0, act, B, "fp32", seed=3001)
    p0 = model.get_params()
    data = torch.as_tensor(np.concatenate(synth_batch(rng, n * B, [784, 147], [True, False]), axis=1)).cuda()
    X = [data[:, :784], data[:, 784:]]
    eps = torch.as_tensor(rng.standard_normal((n * B, 32)).astype(np.float32)).cuda()

    def run(sync):
        m = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct=act, weights=[1.0, 50.0], assoc_lambda=0.0, batch_size=B,
                                          compute_dtype="fp32", seed=7)
        m.set_params(p0)
        for i in range(n):
            m.partial_fit([x[i * B:(i + 1) * B] for x in X], eps[i * B:(i + 1) * B], return_cost=False)
            if sync:
                torch.cuda.synchronize()
        return m.get_params()
    truth = run(True)
    differing = sum(1 for _ in range(300) if not np.array_equal(run(False), truth))
    assert differing == 0, "%d of 300 back-to-back runs differ from the synchronised run" % differing


def test_determinism_and_stress_config_c4(V):
    """BASELINE C4 (4x1024 hidden, n_z=64, B=4096, bf16): too big for the oracle in seconds at full
    batch, so: bitwise run-to-run determinism, finite decreasing cost, and oracle parity of the cost on
    the same weights for the first 128 rows via evaluate on a B=128 replica."""
    hs = [1024] * 4
    archs = [make_arch("image", 784, 0, 0, 64, n_hidden=hs), make_arch("joint", 147, 0, 0, 64, n_hidden=hs)]
    B = 4096
    rng = np.random.default_rng(21)
    X = synth_batch(rng, B, [784, 147], [True, False])
    eps = rng.standard_normal((B, 64)).astype(np.float32)
    kw = dict(binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0, compute_dtype="bf16", seed=5)
    runs = []
    for _ in range(2):
        m = V.AssocVariationalAutoEncoder(archs, batch_size=B, **kw)
        assert m.n_params == 14900387
        costs = [m.partial_fit(X, eps) for _ in range(5)]
        assert shadow_err(m) == (0.0, 0.0, 20)                          # both compute-dtype shadows of all 20 layers = the parameters, rounded once
        runs.append((costs, m.get_params()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    costs = runs[0][0]
    assert np.all(np.isfinite(costs)) and costs[-1] < costs[0]
    small = V.AssocVariationalAutoEncoder(archs, batch_size=128, **kw)
    ref = O.OracleAssocVAE(archs, [True, False], "relu", [50, 1], 8.0, 1e-3, 128, params_flat=small.get_params().astype(np.float64))
    Xs, es = [x[:128] for x in X], eps[:128]
    c, cr = small.evaluate_cost(Xs, es), ref.evaluate_cost(Xs, es)
    assert abs(c - cr) <= 1e-3 * abs(cr), (c, cr)
