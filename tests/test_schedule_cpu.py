"""Training schedules without a GPU (include/avae.h, avae_set_schedule): the fp64 restatement of the
scheduled cost against the oracle, avae_schedule_value (host only -- the evaluator the device runs) against the Python evaluator,
the errors, the helper dicts and train_loop's epoch -> step conversion."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O
from schedule_reference import hyper, schedule_value, scheduled_cost_and_grads, scheduled_step, ulp_distance
from test_oracle import CASES


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def _case_inputs(case, seed=5):
    rng = np.random.default_rng(seed)
    archs, B = case["archs"], case["B"]
    X = synth_batch(rng, B, [a["n_input"] for a in archs], case["binary"])
    eps = rng.standard_normal((B, archs[0]["n_z"]))
    m = O.OracleAssocVAE(archs, case["binary"], case["act"], case["weights"], case["lam"], 1e-3, B, seed=11)
    th = m.get_params() + 0.05 * rng.standard_normal(O.param_count(archs))
    m.set_params(th)
    return m, th, X, eps


# ----------------------------------------------------------------------------- the restated cost
@pytest.mark.parametrize("case", CASES)
def test_unit_multipliers_are_the_oracle(case):
    m, th, X, eps = _case_inputs(case)
    cost, g, _ = m.cost_and_grads(X, eps)
    c, tg = scheduled_cost_and_grads(case["archs"], th, X, eps, case["binary"], case["weights"], case["lam"], case["act"], kl=1.0)
    assert abs(cost - c) <= 1e-11 * abs(c)
    assert np.abs(g - tg).max() <= 1e-9 * max(1.0, np.abs(tg).max())
    # a shard of a global batch: the oracle's batch_global form
    Bg = 3 * case["B"]
    cost, g, _ = m.cost_and_grads(X, eps, batch_global=Bg)
    c, tg = scheduled_cost_and_grads(case["archs"], th, X, eps, case["binary"], case["weights"], case["lam"], case["act"], kl=1.0,
                                     batch_global=Bg)
    assert abs(cost - c) <= 1e-11 * abs(c)
    assert np.abs(g - tg).max() <= 1e-9 * max(1.0, np.abs(tg).max())


@pytest.mark.parametrize("case", CASES[:2])
def test_cost_is_linear_in_kl_and_lambda(case):
    m, th, X, eps = _case_inputs(case)

    def at(kl, lam):
        return scheduled_cost_and_grads(case["archs"], th, X, eps, case["binary"], case["weights"], lam, case["act"], kl=kl)
    c00, g00 = at(0.0, 0.0)
    c10, g10 = at(1.0, 0.0)
    c01, g01 = at(0.0, 1.0)
    assert c10 > c00 and c01 > c00, "the KL and association terms are positive"
    for kl, lam in ((0.37, 8.0), (2.0, 0.25), (0.0, 3.0)):
        c, g = at(kl, lam)
        want_c = c00 + kl * (c10 - c00) + lam * (c01 - c00)
        want_g = g00 + kl * (g10 - g00) + lam * (g01 - g00)
        assert abs(c - want_c) <= 1e-11 * abs(want_c)
        assert np.abs(g - want_g).max() <= 1e-9 * max(1.0, np.abs(want_g).max())


def test_scheduled_step_is_the_oracles_adam_with_the_scheduled_rate():
    case = CASES[0]
    m, th, X, eps = _case_inputs(case)
    twin = O.OracleAssocVAE(case["archs"], case["binary"], case["act"], case["weights"], case["lam"], 0.25e-3, case["B"], params_flat=th)
    m.set_params(th)
    c, g = scheduled_step(m, X, eps, 1.0, case["lam"], 0.25e-3)
    c2 = twin.partial_fit(X, eps)
    assert abs(c - c2) <= 1e-11 * abs(c2) and m.t == twin.t == 1
    assert np.abs(m.get_params() - twin.get_params()).max() <= 1e-12


# ----------------------------------------------------------------------------- avae_schedule_value
STEPS = list(range(41)) + [2 ** 31 + 3, 2 ** 40]
PIECEWISE = [dict(knots=[(0, 0), (10, 1)]), dict(knots=[(3, 0.25), (4, 2), (17, 0.5)]), dict(knots=[(5, 0.3)]),
             dict(knots=[(0, 0), (3, 1)], period=7)]


def lib_value(capi, spec, t):
    from vae_assoc_amd._marshal import schedule_struct
    sc = schedule_struct(spec)
    out = C.c_float(-1.0)
    rc = capi.lib().avae_schedule_value(None if sc is None else C.byref(sc), t, C.byref(out))
    assert rc == 0, capi.lib().avae_last_error(None)
    return np.float32(out.value)


@pytest.mark.parametrize("spec", PIECEWISE)
def test_piecewise_value_is_bitwise_the_reference(capi, spec):
    for u in STEPS:
        got, want = lib_value(capi, spec, u + 1), schedule_value(spec, u + 1)
        assert got.tobytes() == want.tobytes(), (spec, u, got, want)
    # spot values: the ends are held, the period wraps
    if spec.get("period"):
        assert lib_value(capi, spec, 1) == 0 and lib_value(capi, spec, 4) == 1 and lib_value(capi, spec, 7) == 1 and lib_value(capi, spec, 8) == 0
        assert lib_value(capi, spec, 9) == np.float32(1.0 / 3.0)


@pytest.mark.parametrize("staircase", [False, True])
def test_exp_value_is_within_one_ulp(capi, staircase):
    for rate, steps in ((0.96, 10), (0.5, 3), (1.25, 7)):
        spec = dict(decay_rate=rate, decay_steps=steps, staircase=staircase)
        for u in range(41):
            got, want = lib_value(capi, spec, u + 1), schedule_value(spec, u + 1)
            assert ulp_distance(got, want) <= 1, (spec, u, got, want)
    # large step numbers: the exponent is formed in double from the 64-bit counter
    spec = dict(decay_rate=0.999, decay_steps=2 ** 30, staircase=staircase)
    for u in (2 ** 31 + 3, 2 ** 40):
        got, want = lib_value(capi, spec, u + 1), schedule_value(spec, u + 1)
        assert 0 < want < 1 and ulp_distance(got, want) <= 1, (u, got, want)
    assert lib_value(capi, None, 5) == 1 and lib_value(capi, 0.25, 5) == np.float32(0.25)


def _raw(capi, **kw):
    sc = capi.Schedule()
    sc.kind = kw.pop("kind", capi.SCHED_PIECEWISE)
    knots = kw.pop("knots", [])
    sc.n_knots = kw.pop("n_knots", len(knots))
    for i, (s, v) in enumerate(knots[:8]):
        sc.knot_step[i], sc.knot_value[i] = s, v
    for k, v in kw.items():
        setattr(sc, k, v)
    return sc


def test_every_error_names_its_field(capi):
    L = capi.lib()
    out = C.c_float()
    E = capi.SCHED_EXP
    bad = [(_raw(capi, n_knots=0), "n_knots"), (_raw(capi, knots=[(i, 1.0) for i in range(8)], n_knots=9), "n_knots"),
           (_raw(capi, knots=[(0, 0.0), (4, 1.0), (4, 0.5)]), "knot_step[2]"), (_raw(capi, knots=[(5, 0.0), (2, 1.0)]), "knot_step[1]"),
           (_raw(capi, knots=[(-1, 0.0)]), "knot_step[0]"), (_raw(capi, knots=[(0, float("nan"))]), "knot_value[0]"),
           (_raw(capi, knots=[(0, 0.0), (3, -0.5)]), "knot_value[1]"), (_raw(capi, knots=[(0, float("inf"))]), "knot_value[0]"),
           (_raw(capi, knots=[(0, 0.0), (7, 1.0)], period=7), "period"), (_raw(capi, knots=[(0, 0.0)], period=-2), "period"),
           (_raw(capi, kind=E, decay_rate=0.0, decay_steps=5), "decay_rate"), (_raw(capi, kind=E, decay_rate=-1.0, decay_steps=5), "decay_rate"),
           (_raw(capi, kind=E, decay_rate=float("nan"), decay_steps=5), "decay_rate"),
           (_raw(capi, kind=E, decay_rate=0.5, decay_steps=0), "decay_steps"), (_raw(capi, kind=E, decay_rate=0.5, decay_steps=-3), "decay_steps"),
           (_raw(capi, kind=7), "kind")]
    for sc, field in bad:
        assert L.avae_schedule_value(C.byref(sc), 1, C.byref(out)) != 0, field
        assert field.encode() in L.avae_last_error(None), (field, L.avae_last_error(None))
    ok = _raw(capi, knots=[(0, 0.0), (6, 1.0)], period=7)
    assert L.avae_schedule_value(C.byref(ok), 1, C.byref(out)) == 0
    assert L.avae_schedule_value(C.byref(ok), 0, C.byref(out)) != 0 and b"step" in L.avae_last_error(None)


def test_python_arguments_raise_before_the_library():
    from vae_assoc_amd import _marshal as M
    for bad, field in ((dict(knots=[]), "n_knots"), (dict(knots=[(i, 1) for i in range(9)]), "n_knots"),
                       (dict(knots=[(0, 0), (0, 1)]), "knot_step"), (dict(knots=[(-2, 0)]), "knot_step"),
                       (dict(knots=[(0, float("nan"))]), "knot_value"), (dict(knots=[(0, -1.0)]), "knot_value"),
                       (dict(knots=[(0, 0), (9, 1)], period=9), "period"), (dict(decay_rate=0.0, decay_steps=4), "decay_rate"),
                       (dict(decay_rate=0.5, decay_steps=0), "decay_steps"), (dict(knots=[(0, 1)], rate=3), "unknown"),
                       ("fast", "must be None"), (-0.5, "knot_value"), (dict(foo=1), "knots=")):
        with pytest.raises(ValueError, match=field.replace("[", r"\[")):
            M.schedule_spec(bad, "kl")
    with pytest.raises(ValueError, match="unit"):
        M.schedule_kwargs(dict(kl=0.5, unit="minute"))
    with pytest.raises(ValueError, match="unknown"):
        M.schedule_kwargs(dict(beta=0.5))
    assert M.schedule_kwargs(None) == {} and M.schedule_kwargs(dict(kl=None)) == {}


def test_helper_dicts():
    from vae_assoc_amd import _marshal as M
    from vae_assoc_amd import cyclical, exponential_decay, linear_warmup
    w = linear_warmup(10)
    assert w == dict(knots=[(0, 0.0), (10, 1.0)], period=None)
    assert [float(schedule_value(w, t)) for t in (1, 6, 11, 50)] == [0.0, 0.5, 1.0, 1.0]
    assert float(schedule_value(linear_warmup(4, start=0.5), 3)) == 0.75
    c = cyclical(8, ramp=0.25, start=0.0)
    assert c == dict(knots=[(0, 0.0), (2, 1.0)], period=8)
    assert [float(schedule_value(c, t)) for t in (1, 2, 3, 8, 9, 10)] == [0.0, 0.5, 1.0, 1.0, 0.0, 0.5]
    with pytest.raises(ValueError, match="ramp"):
        cyclical(4, ramp=1.0)
    with pytest.raises(ValueError, match="whole number"):
        M.schedule_spec(cyclical(5, ramp=0.5), "kl")
    e = exponential_decay(0.96, 100, staircase=True)
    assert e == dict(decay_rate=0.96, decay_steps=100, staircase=True)
    assert schedule_value(e, 100) == 1 and schedule_value(e, 101) == np.float32(0.96)
    for h in (w, c, e):
        M.schedule_struct(h)           # every helper's dict is a valid argument
    lam, lr = 8.0, 1e-3
    k, l, r = hyper(w, c, e, lam, lr, 2)
    assert k == np.float32(0.1) and l == np.float32(8.0) * np.float32(0.5) and r == np.float32(1e-3)


# ----------------------------------------------------------------------------- train_loop: epochs -> steps
T_ARCHS = [make_arch("image", 60, 20, 16, 5), make_arch("joint", 21, 12, 10, 5)]
T_BIN, T_W, T_LAM, T_LR = [True, False], [50.0, 1.0], 8.0, 1e-3


class ScheduledOracleReplica(object):
    """The model surface train_loop drives, on the CPU oracle with the scheduled cost of tests/schedule_reference.py.  Records
    what set_schedule was handed and the multipliers of every training step; evaluation uses the configured objective."""

    def __init__(self, B, params, eps_all):
        self.model = O.OracleAssocVAE(T_ARCHS, T_BIN, "relu", T_W, T_LAM, T_LR, B, params_flat=params)
        self.B, self.eps_all, self.k, self.sched, self.hist, self.costs, self.evals = B, eps_all, 0, None, [], [], []

    def set_schedule(self, kl=None, assoc=None, lr=None):
        self.sched = dict(kl=kl, assoc=assoc, lr=lr)

    def partial_fit(self, X, eps=None, return_cost=True):
        s = self.sched or dict(kl=None, assoc=None, lr=None)
        h = hyper(s["kl"], s["assoc"], s["lr"], T_LAM, T_LR, self.model.t + 1)
        c, _g = scheduled_step(self.model, X, self.eps_all[self.k], *[float(x) for x in h])
        self.k += 1
        self.hist.append(h)
        self.costs.append(c)
        return c

    def partial_fit_steps(self, X, n_steps, eps=None, return_cost=True):
        for i in range(n_steps):
            self.partial_fit([x[i * self.B:(i + 1) * self.B] for x in X])

    def cost_history(self, n):
        return np.asarray(self.costs[-n:])

    def evaluate_cost(self, X, eps=None):
        c = self.model.evaluate_cost(X, self.eps_all[self.k])
        self.k += 1
        self.evals.append(c)
        return c


def test_train_loop_converts_epochs_to_steps():
    from vae_assoc_amd import dataset
    from vae_assoc_amd import cyclical, exponential_decay, linear_warmup
    from vae_assoc_amd.vae_assoc import train_loop
    N, B, epochs = 100, 8, 3
    rng = np.random.default_rng(31)
    data = np.concatenate(synth_batch(rng, N, [60, 21], T_BIN), axis=1).astype(np.float64)
    eps_all = rng.standard_normal((64, B, 5))
    p0 = O.flatten_params(T_ARCHS, O.init_params(T_ARCHS, np.random.default_rng(0)))
    np.random.seed(9)
    ds = dataset.construct_datasets(data.copy())
    n_train = ds.train._data.shape[0]
    per_epoch = n_train // B
    assert per_epoch >= 4 and per_epoch % 2 == 0, "half an epoch must be a whole number of steps"
    rep = ScheduledOracleReplica(B, p0, eps_all)
    sched = dict(kl=linear_warmup(2), assoc=cyclical(1, ramp=0.5), lr=exponential_decay(0.5, 1.5, staircase=True), unit="epoch")
    _m, hist = train_loop(rep, ds, T_ARCHS, B, training_epochs=epochs, display_step=10, early_stop=1, schedule=sched)
    want = dict(kl=dict(knots=[(0, 0.0), (2 * per_epoch, 1.0)], period=0),
                assoc=dict(knots=[(0, 0.0), (per_epoch // 2, 1.0)], period=per_epoch),
                lr=dict(decay_rate=0.5, decay_steps=int(1.5 * per_epoch), staircase=True))
    assert rep.sched == want
    assert len(rep.hist) == epochs * per_epoch == len(hist)
    for i, (k, l, r) in enumerate(rep.hist):
        assert k == schedule_value(want["kl"], i + 1) and l == np.float32(T_LAM) * schedule_value(want["assoc"], i + 1)
        assert r == np.float32(T_LR) * schedule_value(want["lr"], i + 1)
    assert rep.hist[0][0] == 0 and rep.hist[2 * per_epoch][0] == 1 and rep.hist[per_epoch][1] == 0
    assert len(rep.evals) > 0, "the early-stop cost is the stub's unscheduled evaluate_cost"
    # unit='step' passes the schedules through; a data-parallel loop counts global batches
    rep2 = ScheduledOracleReplica(B, p0, eps_all)
    np.random.seed(9)
    train_loop(rep2, dataset.construct_datasets(data.copy()), T_ARCHS, B, training_epochs=1, display_step=10,
               schedule=dict(kl=linear_warmup(5)))
    assert rep2.sched == dict(kl=dict(knots=[(0, 0.0), (5, 1.0)], period=0), assoc=None, lr=None)
    # half an epoch that is no whole number of steps is refused, naming the schedule
    rep3 = ScheduledOracleReplica(B, p0, eps_all)
    with pytest.raises(ValueError, match="kl"):
        train_loop(rep3, ds, T_ARCHS, B, training_epochs=1, schedule=dict(kl=linear_warmup(1.0 / 3.0 + 1e-3), unit="epoch"))
    assert rep3.sched is None and not rep3.hist
