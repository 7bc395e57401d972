"""``complete`` / avae_complete on a real MI355X (include/avae.h): gradient latent refinement for partially
observed rows against the fp64 definition in tests/complete_reference.py.

Tolerances are the project's: fp32 against fp64 -- objective 1e-5 relative, gradient 1e-4 of the tensor's
maximum; bf16 against the reference run with quant='bf16' -- 5e-5 and 3e-3.  relu cases hand the kernels' own relu decisions of
the pass to the reference (conftest.hip_relu_masks), as tests/test_gpu_parity.py does, so that what is compared is arithmetic.
The trajectory bound is measured, not chosen: see test_trajectory_matches_reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import complete_cases as cases
import complete_reference as R
from conftest import hip_relu_masks, make_arch

pytestmark = pytest.mark.gpu

TOL = {"fp32": (1e-5, 1e-4), "bf16": (5e-5, 3e-3)}
CONV = dict(archs=[dict(make_arch("image", 784, 8, 24, 6), hidden_conv=True, n_hidden_gener_1=24, n_hidden_gener_2=8),
                   make_arch("joint", 147, 40, 30, 6)], binary=[True, False], weights=[5.0, 1.0], lam=0.5, B=32)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _model(V, net, dtype, act, seed=11, set_p0=True, **kw):
    m = V.AssocVariationalAutoEncoder(net["archs"], binary=net["binary"], transfer_fct=act, weights=net["weights"],
                                      assoc_lambda=net["lam"], learning_rate=1e-3, batch_size=net["B"], compute_dtype=dtype, seed=seed, **kw)
    if set_p0:
        m.set_params(cases.params0(net))
    return m


def _ref(net, X, obs, z0, act, dtype, n_iters, masks0=None, prior=cases.PRIOR, lr=cases.LR):
    return R.complete(net["archs"], cases.params0(net), X, obs, z0, net["binary"], net["weights"], act, n_iters, lr, prior,
                      quant="bf16" if dtype == "bf16" else None, masks0=masks0)


def _same(a, b):
    assert np.array_equal(a["z"], b["z"]) and np.array_equal(a["objective"], b["objective"]) and np.array_equal(a["grad0"], b["grad0"])
    for xa, xb in zip(a["x"], b["x"]):
        assert np.array_equal(xa, xb)


@pytest.mark.parametrize("act,dtype", [("relu", "fp32"), ("softplus", "fp32"), ("relu", "bf16"), ("softplus", "bf16")])
@pytest.mark.parametrize("name,pattern", [("two", "random"), ("two", "none_last"), ("two", "full_last"),
                                          ("three", "random"), ("three", "none_last"), ("three", "full_last")])
def test_gradient_and_objective_at_z0(V, name, pattern, act, dtype):
    net = cases.NETS[name]
    X, obs, z0 = cases.inputs(net, net["B"], pattern)
    model = _model(V, net, dtype, act)
    got = model.complete(X, obs, n_iters=0, z0=z0, prior_weight=cases.PRIOR)
    masks = hip_relu_masks(model, net["archs"]) if act == "relu" else None      # the decoders' decisions of the one pass made
    ref = _ref(net, X, obs, z0, act, dtype, 0, masks0=masks)
    tol_j, tol_g = TOL[dtype]
    ej = (np.abs(got["objective"][0] - ref["objective"][0]) / np.abs(ref["objective"][0])).max()
    eg = np.abs(got["grad0"] - ref["grad0"]).max() / np.abs(ref["grad0"]).max()
    ex = max(np.abs(a - b).max() for a, b in zip(got["x"], ref["x"]))
    print("%s %s %s %s: objective rel %.2e, grad %.2e of max, x abs %.2e" % (name, pattern, act, dtype, ej, eg, ex))
    assert got["objective"].shape == (1, net["B"]) and got["grad0"].shape == z0.shape
    assert np.array_equal(got["z"], z0)                  # n_iters = 0 evaluates only
    assert ej <= tol_j and eg <= tol_g
    assert ex <= (1e-5 if dtype == "fp32" else 2e-3)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tie_to_score_samples_and_generate(V, dtype):
    """everything observed, n_iters = 0, z0 = transform(X)[s]: objective[0] is score_samples' cross columns of source s plus the
    prior term (1e-5 relative), and x is generate(z0) BITWISE on these nets and both dtypes (measured difference: 0), although
    generate's staging launch runs the decoders' first layer itself and the plan here has a first-layer launch of its own."""
    net = cases.NETS["two"]
    X, _, _ = cases.inputs(net, 2 * net["B"] + 3, "all")
    model = _model(V, net, dtype, "relu")
    for s in range(2):
        z0 = model.transform(X)[s]
        got = model.complete(X, None, n_iters=0, z0=z0, prior_weight=0.7)
        cross = model.score_samples(X, cross_modal=True)["cross"][:, s, :]
        want = sum(w * cross[:, d].astype(np.float64) for d, w in enumerate(net["weights"])) + 0.7 * 0.5 * np.sum(z0.astype(np.float64) ** 2, 1)
        assert (np.abs(got["objective"][0] - want) / np.abs(want)).max() <= 1e-5
        gen = model.generate(z0)
        dx = max(np.abs(a - b).max() for a, b in zip(got["x"], gen))
        print("source %d %s: max |x - generate(z0)| = %.3e" % (s, dtype, dx))
        assert all(np.array_equal(a, b) for a, b in zip(got["x"], gen))


def test_trajectory_matches_reference(V):
    """z and objective after T = 20 Adam iterations, fp32 kernels against the fp64 reference (softplus: no relu kinks).  Adam
    amplifies rounding, so the bound is measured: the reference in fp64 against the same reference in float32 arithmetic on these
    inputs deviates by 8.1e-7 of max |z| in z and 2.9e-7 relative in the objective (tests/test_complete_cpu.py re-measures it);
    the kernels may deviate 4 times as much, for a different summation order: 3.24e-6 and 1.16e-6."""
    net = cases.NETS["two"]
    X, obs, z0 = cases.inputs(net, net["B"], "random")
    model = _model(V, net, "fp32", "softplus")
    got = model.complete(X, obs, n_iters=cases.T_TRAJ, lr=cases.LR, prior_weight=cases.PRIOR, z0=z0)
    ref = _ref(net, X, obs, z0, "softplus", "fp32", cases.T_TRAJ)
    dz = np.abs(got["z"] - ref["z"]).max() / np.abs(ref["z"]).max()
    dj = (np.abs(got["objective"] - ref["objective"]) / np.abs(ref["objective"])).max()
    print("trajectory: z %.3e of max|z| (bound %.3e), objective %.3e relative (bound %.3e)" % (dz, cases.TRAJ_BOUND_Z, dj, cases.TRAJ_BOUND_OBJ))
    assert got["objective"].shape == (cases.T_TRAJ + 1, net["B"])
    assert dz <= cases.TRAJ_BOUND_Z and dj <= cases.TRAJ_BOUND_OBJ


@pytest.mark.parametrize("name,pattern,act,dtype", [(n, p, a, "bf16" if q else "fp32") for n, p, a, q in
                                                    [(n, p, a, q) for n in ("two", "three") for p in ("random", "none_last", "full_last")
                                                     for a, q in (("softplus", None), ("relu", None), ("relu", "bf16"))]])
def test_objective_decreases_on_every_row(V, name, pattern, act, dtype):
    """the same inputs, lr and iteration count on which tests/test_complete_cpu.py shows that the reference decreases on every row"""
    net = cases.NETS[name]
    X, obs, z0 = cases.inputs(net, net["B"], pattern)
    got = _model(V, net, dtype, act).complete(X, obs, n_iters=cases.T_TRAJ, lr=cases.LR, prior_weight=cases.PRIOR, z0=z0)
    assert np.all(np.isfinite(got["objective"]))
    assert np.all(got["objective"][-1] < got["objective"][0]), (got["objective"][0] - got["objective"][-1]).min()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_unobserved_entries_are_never_read(V, dtype):
    net = cases.NETS["three"]
    rows = net["B"] + 5
    X, obs, z0 = cases.inputs(net, rows, "random")
    obs[2][:] = False                                       # modality 2 unobserved on every row, through its mask
    model = _model(V, net, dtype, "relu")
    clean = model.complete(X, obs, n_iters=5, z0=z0)
    bad = [x.copy() for x in X]
    for m in range(3):
        hole = ~obs[m]
        bad[m][hole] = np.where(np.arange(hole.sum()) % 2 == 0, np.nan, np.inf).astype(np.float32)
    assert np.all(~np.isfinite(bad[2]))
    _same(clean, model.complete(bad, obs, n_iters=5, z0=z0))
    _same(clean, model.complete([X[0], X[1], None], [obs[0], obs[1], None], n_iters=5, z0=z0))     # None == an all-zero mask
    assert np.all(np.isfinite(clean["z"])) and all(np.all(np.isfinite(x)) for x in clean["x"])


def _state(m, n_hist):
    mm, vv, st = m.get_opt_state()
    return m.get_params(), mm, vv, st, m.get_grads(), m.cost_history(n_hist)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_state_is_untouched(V, dtype):
    net = cases.NETS["two"]
    B = net["B"]
    rng = np.random.default_rng(23)
    X, obs, z0 = cases.inputs(net, B, "random")
    Xc, obsc, z0c = cases.inputs(net, 2 * B + 3, "full_last", seed=9)
    eps = [rng.standard_normal((B, 20)).astype(np.float32) for _ in range(4)]
    present = rng.random((B, 2)) < 0.7
    a, b = _model(V, net, dtype, "relu"), _model(V, net, dtype, "relu")
    assert a.partial_fit(X, eps[0]) == b.partial_fit(X, eps[0])
    before = _state(a, 1)
    a.complete(Xc, obsc, n_iters=7, z0=z0c)
    a.complete(X, obs, n_iters=3)                           # start from the encoder
    for x, y, what in zip(before, _state(a, 1), ("params", "adam m", "adam v", "step", "grads", "cost history")):
        assert np.array_equal(x, y), what
    assert a.partial_fit(X, eps[1]) == b.partial_fit(X, eps[1])
    a.complete(Xc, obsc, n_iters=2, z0=z0c)
    assert a.partial_fit(X, eps[2], present=present) == b.partial_fit(X, eps[2], present=present)
    sa = a.score_samples(X, eps=eps[3])
    a.complete(X, obs, n_iters=1, z0=z0)
    sb = b.score_samples(X, eps=eps[3])
    assert np.array_equal(sa["cost"], sb["cost"])
    assert a.partial_fit(X, eps[3]) == b.partial_fit(X, eps[3])
    for x, y, what in zip(_state(a, 4), _state(b, 4), ("params", "adam m", "adam v", "step", "grads", "cost history")):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_any_row_count_and_rows_are_independent(V, dtype):
    net = cases.NETS["two"]
    B = net["B"]
    model = _model(V, net, dtype, "relu")
    tol_g = TOL[dtype][1]
    for rows in (1, B - 1, B + 1, 3 * B + 7):
        X, obs, z0 = cases.inputs(net, rows, "random", seed=rows)
        got = model.complete(X, obs, n_iters=4, z0=z0)
        _same(got, model.complete(X, obs, n_iters=4, z0=z0))        # bitwise from call to call
        assert got["z"].shape == (rows, 20) and got["objective"].shape == (5, rows) and got["x"][0].shape == (rows, 784)
        for n in range(rows):
            one = model.complete([x[n:n + 1] for x in X], [o[n:n + 1] for o in obs], n_iters=4, z0=z0[n:n + 1])
            for key in ("z", "grad0"):
                assert np.abs(one[key][0] - got[key][n]).max() <= tol_g * np.abs(got[key]).max(), (rows, n, key)
            assert np.abs(one["objective"][:, 0] - got["objective"][:, n]).max() <= tol_g * np.abs(got["objective"]).max(), (rows, n)
            for m in range(2):
                assert np.abs(one["x"][m][0] - got["x"][m][n]).max() <= tol_g * np.abs(got["x"][m]).max(), (rows, n, m)
    X, obs, z0 = cases.inputs(net, 0, "random")
    empty = model.complete(X, obs, n_iters=4, z0=z0)
    assert empty["z"].shape == (0, 20) and empty["objective"].shape == (5, 0) and empty["grad0"].shape == (0, 20)
    assert [x.shape for x in empty["x"]] == [(0, 784), (0, 147)]
    # device tensors in, device tensors out
    X, obs, z0 = cases.inputs(net, B + 1, "random", seed=B + 1)
    dev = model.complete([torch.from_numpy(x).cuda() for x in X], [torch.from_numpy(o).cuda() for o in obs], n_iters=4,
                         z0=torch.from_numpy(z0).cuda())
    assert torch.is_tensor(dev["z"]) and dev["z"].is_cuda and all(torch.is_tensor(x) for x in dev["x"])
    assert np.array_equal(dev["z"].cpu().numpy(), model.complete(X, obs, n_iters=4, z0=z0)["z"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eager_passes_equal_replayed_graphs(V, dtype):
    """use_graph = 0 and timing mode launch the passes one by one instead of replaying graphs of 16 / 4 / 1 passes: same bits"""
    net = cases.NETS["two"]
    X, obs, z0 = cases.inputs(net, net["B"] + 9, "random")
    model = _model(V, net, dtype, "relu")
    want = model.complete(X, obs, n_iters=22, z0=z0)              # 23 passes = 16 + 4 + 1 + 1 + 1
    _same(want, _model(V, net, dtype, "relu", use_graph=False).complete(X, obs, n_iters=22, z0=z0))
    assert model._L.avae_timing_enable(model._h, 1) == 0
    buf = C.create_string_buffer(1 << 16)
    try:
        timed = model.complete(X, obs, n_iters=22, z0=z0)
        assert model._L.avae_timing_report(model._h, buf, len(buf)) == 0
    finally:
        assert model._L.avae_timing_enable(model._h, 0) == 0
    _same(want, timed)
    names = [line.split()[0] for line in buf.value.decode().splitlines() if line.strip()]
    for name in ("complete_begin", "cmpl_dec1", "cmpl_dec2", "cmpl_out", "complete_out", "cmpl_bwd_out", "cmpl_bwd_dec2", "cmpl_bwd_dz",
                 "complete_update"):
        assert name in names, (name, names)


def test_errors_have_messages(V):
    net = cases.NETS["two"]
    B = net["B"]
    model = _model(V, net, "bf16", "relu")
    X, obs, z0 = cases.inputs(net, B, "random")
    with pytest.raises(ValueError):
        model.complete([X[0][:, :100], X[1]], None, z0=z0)                     # wrong width
    with pytest.raises(ValueError):
        model.complete([X[0], X[1][:5]], None, z0=z0)                           # row counts disagree
    with pytest.raises(ValueError):
        model.complete(X, [obs[0][:5], obs[1]], z0=z0)                          # mask rows != data rows
    with pytest.raises(ValueError):
        model.complete(X, [obs[0], obs[1][:, :10]], z0=z0)                      # mask width
    with pytest.raises(ValueError):
        model.complete(X, obs, z0=z0[:, :7])                                    # z0 width
    with pytest.raises(ValueError):
        model.complete(X, obs, z0=z0[:3])                                       # z0 rows
    with pytest.raises(ValueError):
        model.complete(X, obs, n_iters=-1, z0=z0)
    with pytest.raises(ValueError):
        model.complete([None, None], None, z0=z0)
    with pytest.raises(ValueError):
        model.complete([None, X[1]], None, init=0)                              # init names an unobserved modality
    with pytest.raises(ValueError):
        model.complete(X[:1], None, z0=z0)
    # straight through the C ABI
    L, h = model._L, model._h
    xt = [torch.from_numpy(x).cuda() for x in X]
    zt = torch.from_numpy(z0).cuda()
    out = torch.empty_like(zt)
    xp = (C.c_void_p * 2)(xt[0].data_ptr(), xt[1].data_ptr())
    none = (C.c_void_p * 2)(None, None)
    st = model._stream()

    def call(x=xp, z0p=zt.data_ptr(), rows=B, n_iters=1, zp=out.data_ptr()):
        rc = L.avae_complete(h, x, None, None, z0p, rows, n_iters, 0.05, 1.0, zp, None, None, None, st)
        return rc, L.avae_last_error(h).decode()

    for kw, word in ((dict(z0p=None), "z0_dev"), (dict(zp=None), "z_dev"), (dict(n_iters=-2), "n_iters"), (dict(rows=-1), "rows"),
                     (dict(x=none), "NULL"), (dict(x=None), "x_dev")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    assert call(rows=0, z0p=None, zp=None)[0] == 0                               # rows = 0 is a no-op
    assert call()[0] == 0
    torch.cuda.synchronize()
    conv = _model(V, CONV, "bf16", "relu", set_p0=False)
    Xc = [np.zeros((4, 784), np.float32), np.zeros((4, 147), np.float32)]
    with pytest.raises(RuntimeError, match="conv"):
        conv.complete(Xc, None, n_iters=1, z0=np.zeros((4, 6), np.float32))
    # the model keeps working after every refused call
    assert np.all(np.isfinite(model.complete(X, obs, n_iters=2, z0=z0)["z"]))


def test_workspace_size_is_unchanged(V):
    """avae_workspace_bytes for C2 (784-500-500 / 147-200-200, n_z 20, batch 256, bf16) is the number of the commit before
    avae_complete existed: its scratch is allocated by the first call, outside the workspace"""
    from vae_assoc_amd import _capi
    cfg = _capi.Config()
    cfg.abi_version = _capi.AVAE_ABI_VERSION
    cfg.n_modalities = 2
    for m, (n_in, hid) in enumerate(((784, 500), (147, 200))):
        cfg.mod[m].n_input, cfg.mod[m].n_hidden_layers, cfg.mod[m].binary, cfg.mod[m].weight = n_in, 2, 1 - m, 1.0
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = hid
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = 20, 256, 1, 1
    n = C.c_size_t(0)
    assert _capi.lib().avae_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    assert n.value == 62817792
