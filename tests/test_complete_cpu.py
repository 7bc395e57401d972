"""CPU checks of tests/complete_reference.py, the fp64 definition of ``complete`` (include/avae.h: avae_complete): its decoder
input-gradient chain against central finite differences of its own objective and against a torch fp64 autograd transcription, the
objective against the oracle's per-row terms, unobserved elements never entering, the Adam recurrence against a hand computation,
and -- on the very inputs tests/test_gpu_complete.py uses -- the conditions those tests impose (decrease on every row, the
rounding spread of the 20-iteration trajectory)."""
import numpy as np
import pytest

import complete_cases as cases
import complete_reference as R
from masked_reference import per_row_terms
from oracle import vae_assoc_oracle as O


def _setup(name, pattern, rows=6, act="softplus"):
    net = cases.NETS[name]
    p0 = cases.params0(net).astype(np.float64)
    X, obs, z0 = cases.inputs(net, rows, pattern)
    params = O.unflatten_params(net["archs"], p0, np.float64)
    X64 = [None if x is None else x.astype(np.float64) for x in X]
    return net, p0, params, X64, obs, z0.astype(np.float64)


@pytest.mark.parametrize("act", ["softplus", "tanh"])
@pytest.mark.parametrize("name,pattern", [("two", "random"), ("two", "none_last"), ("three", "full_last")])
def test_gradient_matches_central_differences(name, pattern, act):
    net, _, params, X, obs, z = _setup(name, pattern, rows=4, act=act)
    f = lambda zz: R.objective_and_grad(net["archs"], params, X, obs, zz, net["binary"], net["weights"], act, 0.7)[0]  # noqa: E731
    _, g, _ = R.objective_and_grad(net["archs"], params, X, obs, z, net["binary"], net["weights"], act, 0.7)
    h = 1e-6
    fd = np.zeros_like(z)
    for j in range(z.shape[1]):
        e = np.zeros_like(z)
        e[:, j] = h
        fd[:, j] = (f(z + e) - f(z - e)) / (2 * h)          # rows are independent: one column perturbs every row at once
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_gradient_matches_torch_autograd(act):
    torch = pytest.importorskip("torch")
    net, _, params, X, obs, z = _setup("two", "random", rows=5, act=act)
    J, g, _ = R.objective_and_grad(net["archs"], params, X, obs, z, net["binary"], net["weights"], act, 1.3)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    f = {"relu": torch.relu, "softplus": torch.nn.functional.softplus}[act]
    Jt = 1.3 * 0.5 * (zt * zt).sum(1)
    for na, p, x, o, b, w in zip(net["archs"], params, X, obs, net["binary"], net["weights"]):
        hcur = zt
        for i in range(len(O.hidden_sizes(na))):
            hcur = f(hcur @ torch.tensor(p["dec_W%d" % (i + 1)]) + torch.tensor(p["dec_b%d" % (i + 1)]))
        logits = hcur @ torch.tensor(p["dec_Wout"]) + torch.tensor(p["dec_bout"])
        ot = torch.tensor(np.asarray(o) != 0)
        xt = torch.tensor(np.where(np.asarray(o) != 0, x, 0.0))
        if b:
            ph = torch.sigmoid(logits)
            t = -(xt * torch.log(1e-3 + ph) + (1 - xt) * torch.log(1e-3 + 1 - ph))
        else:
            t = 0.5 * (xt - logits) ** 2
        Jt = Jt + w * torch.where(ot, t, torch.zeros_like(t)).sum(1)
    Jt.sum().backward()
    assert np.abs(Jt.detach().numpy() - J).max() <= 1e-12 * np.abs(J).max()
    assert np.abs(zt.grad.numpy() - g).max() <= 1e-11 * np.abs(g).max()


def test_everything_observed_is_the_oracles_per_row_terms():
    net, p0, params, X, _, z = _setup("two", "all", rows=7, act="relu")
    J, _, outs = R.objective_and_grad(net["archs"], params, X, None, z, net["binary"], net["weights"], "relu", 0.0)
    want = np.zeros(7)
    for m, (na, b, w) in enumerate(zip(net["archs"], net["binary"], net["weights"])):
        xhat, _ = O.decode(na, params[m], z, "relu", b)
        assert np.array_equal(xhat, outs[m])
        r = -np.sum(X[m] * np.log(1e-3 + xhat) + (1 - X[m]) * np.log(1e-3 + 1 - xhat), 1) if b else np.sum((X[m] - xhat) ** 2, 1) / 2
        want += w * r
    assert np.abs(J - want).max() <= 1e-13 * np.abs(want).max()
    # and, from z = the posterior mean with eps = 0, score_samples' recon columns
    mus = [O.encode(na, params[m], X[m], "relu")[0] for m, na in enumerate(net["archs"])]
    J0, _, _ = R.objective_and_grad(net["archs"], params, X, None, mus[0], net["binary"], net["weights"], "relu", 0.0)
    recon, _, _ = per_row_terms(net["archs"], p0, [X[0], X[1]], np.zeros_like(z), net["binary"], "relu")
    xh1, _ = O.decode(net["archs"][1], params[1], mus[0], "relu", False)
    assert np.abs(J0 - (net["weights"][0] * recon[:, 0] + net["weights"][1] * np.sum((X[1] - xh1) ** 2, 1) / 2)).max() <= 1e-12 * np.abs(J0).max()


def test_unobserved_values_never_enter():
    net, _, params, X, obs, z = _setup("two", "random", rows=5)
    J, g, _ = R.objective_and_grad(net["archs"], params, X, obs, z, net["binary"], net["weights"], "softplus", 1.0)
    Xd = [np.where(np.asarray(o) != 0, x, np.nan) for x, o in zip(X, obs)]
    Xd[1][~(np.asarray(obs[1]) != 0)] = np.inf
    with np.errstate(all="ignore"):
        Jd, gd, _ = R.objective_and_grad(net["archs"], params, Xd, obs, z, net["binary"], net["weights"], "softplus", 1.0)
    assert np.array_equal(J, Jd) and np.array_equal(g, gd)
    # a None modality == an all-zero mask on it
    Jn, gn, _ = R.objective_and_grad(net["archs"], params, [X[0], None], [obs[0], None], z, net["binary"], net["weights"], "softplus", 1.0)
    Jz, gz, _ = R.objective_and_grad(net["archs"], params, X, [obs[0], np.zeros_like(obs[1])], z, net["binary"], net["weights"], "softplus", 1.0)
    assert np.array_equal(Jn, Jz) and np.array_equal(gn, gz)


def test_adam_recurrence_by_hand():
    b1, b2, eps, lr = R.BETA1, R.BETA2, R.ADAM_EPS, 0.05
    z, m, v = np.array([[0.3]]), np.zeros((1, 1)), np.zeros((1, 1))
    zs, ms, vs = 0.3, 0.0, 0.0
    for t, g in enumerate([2.0, -0.5, 0.25], 1):
        z, m, v = R.adam_update(z, m, v, np.array([[g]]), t, lr)
        ms = b1 * ms + (1 - b1) * g
        vs = b2 * vs + (1 - b2) * g * g
        zs = zs - lr * (ms / (1 - b1 ** t)) / ((vs / (1 - b2 ** t)) ** 0.5 + eps)
        assert abs(z[0, 0] - zs) <= 1e-15
    # the first step moves every element by lr against the sign of its gradient (m_hat / sqrt(v_hat) = g / |g|)
    z1, _, _ = R.adam_update(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), np.array([[4.0, -1e-3, 7.0]]), 1, lr)
    assert np.allclose(z1, [[-lr, lr, -lr]], rtol=1e-4)


DECREASE = [(name, pattern, act, quant) for name in ("two", "three") for pattern in ("random", "none_last", "full_last")
            for act, quant in (("softplus", None), ("relu", None), ("relu", "bf16"))]


@pytest.mark.parametrize("name,pattern,act,quant", DECREASE)
def test_reference_decreases_on_every_row_of_the_gpu_tests_inputs(name, pattern, act, quant):
    net = cases.NETS[name]
    X, obs, z0 = cases.inputs(net, net["B"], pattern)
    r = R.complete(net["archs"], cases.params0(net), X, obs, z0, net["binary"], net["weights"], act, cases.T_TRAJ, cases.LR,
                   cases.PRIOR, quant=quant)
    assert np.all(r["objective"][-1] < r["objective"][0]), (r["objective"][0] - r["objective"][-1]).min()


def test_trajectory_rounding_spread_of_the_gpu_tests_inputs():
    """fp64 reference against the same reference in float32 arithmetic, on the trajectory test's inputs: the measured spread is
    what complete_cases.TRAJ_DEV_* record (the GPU test allows 4 times as much)."""
    net = cases.NETS["two"]
    X, obs, z0 = cases.inputs(net, net["B"], "random")
    kw = dict(n_iters=cases.T_TRAJ, lr=cases.LR, prior_weight=cases.PRIOR)
    r64 = R.complete(net["archs"], cases.params0(net), X, obs, z0, net["binary"], net["weights"], "softplus", **kw)
    r32 = R.complete(net["archs"], cases.params0(net), X, obs, z0, net["binary"], net["weights"], "softplus", dtype=np.float32, **kw)
    assert r32["z"].dtype == np.float32 and r32["objective"].dtype == np.float32
    dz = np.abs(r32["z"] - r64["z"]).max() / np.abs(r64["z"]).max()
    dj = (np.abs(r32["objective"] - r64["objective"]) / np.abs(r64["objective"])).max()
    print("trajectory spread fp32 vs fp64: z %.3e of max|z|, objective %.3e relative" % (dz, dj))
    assert cases.TRAJ_DEV_Z / 4 <= dz <= 2 * cases.TRAJ_DEV_Z, dz
    assert cases.TRAJ_DEV_OBJ / 4 <= dj <= 2 * cases.TRAJ_DEV_OBJ, dj
