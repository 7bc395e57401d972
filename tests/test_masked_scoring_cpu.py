"""CPU checks of scoring, log-likelihood and train() for partially paired rows (include/avae.h): the fp64
reference of tests/masked_scoring_reference.py against the pattern identity and the masked cost, the new entry points in the C
ABI and the model surface, presence travelling through the data sets, and train_loop on a presence-carrying data set against a
hand-written masked loop (an oracle-backed replica stands in for the HIP model, as in tests/test_parallel_gloo.py).

Presence is deterministic (all_patterns_mask: row n -> a fixed permutation of n mod 2^M) and batch_size >= 2^M in every case."""
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_arch, synth_batch
from masked_reference import masked_cost_and_grads, masked_cost_from_rows
from masked_scoring_reference import (all_patterns_mask, has_every_pattern, pattern_loglik, pattern_scores, ref_loglik_masked,
                                      ref_scores_masked)
from oracle import vae_assoc_oracle as O
from scoring_reference import ref_loglik, ref_scores
from vae_assoc_amd import dataset

CASES = [
    dict(archs=[make_arch("image", 30, 12, 10, 4), make_arch("joint", 9, 8, 6, 4)], binary=[True, False],
         weights=[3.0, 1.0], lam=0.8, act="softplus", B=6),
    dict(archs=[make_arch("a", 14, 10, 8, 3), make_arch("b", 11, 8, 6, 3), make_arch("c", 9, 6, 6, 3)],
         binary=[True, False, False], weights=[2.0, 1.0, 0.5], lam=0.7, act="relu", B=9),
]


def _setup(case, seed, N, quant=None):
    rng = np.random.default_rng(seed)
    archs = case["archs"]
    flat = O.flatten_params(archs, O.init_params(archs, rng)) + 0.02 * rng.standard_normal(O.param_count(archs))
    ref = O.OracleAssocVAE(archs, case["binary"], case["act"], case["weights"], case["lam"], 1e-3, case["B"], params_flat=flat,
                           quant=quant)
    X = [x.astype(np.float64) for x in synth_batch(rng, N, [na["n_input"] for na in archs], case["binary"])]
    return rng, ref, X


def _assert_chunks_have_every_pattern(p, B):
    assert B >= 1 << p.shape[1]
    for r0 in range(0, p.shape[0] - B + 1, B):
        assert has_every_pattern(p[r0:r0 + B]), r0


def _same_where_defined(got, want, exact, what):
    """``want`` (pattern by pattern) is NaN where the pattern defines nothing; elsewhere got == want (or to 1e-12 relative)"""
    ok = ~np.isnan(want)
    assert ok.any(), what
    if exact:
        assert np.array_equal(got[ok], want[ok]), what
    else:
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])), what


# ------------------------------------------------------------------------------------------------ the reference
def test_all_patterns_mask_meets_the_input_condition():
    for M in (1, 2, 3, 4):
        for shift in (0, 3):
            p = all_patterns_mask(5 * (1 << M) + 3, M, shift)
            for r0 in range(p.shape[0] - (1 << M) + 1):          # any 2^M consecutive rows, so any chunk of B >= 2^M rows
                assert has_every_pattern(p[r0:r0 + (1 << M)])
    assert np.array_equal(all_patterns_mask(40, 3), all_patterns_mask(40, 3))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("quant", [None, "bf16"])
def test_score_reference_is_the_sub_model_per_pattern(case, quant):
    N, M = 2 * case["B"] + 3, len(case["archs"])
    rng, ref, X = _setup(case, 1, N, quant)
    eps = rng.standard_normal((N, case["archs"][0]["n_z"]))
    p = all_patterns_mask(N, M)
    _assert_chunks_have_every_pattern(p, case["B"])
    got = ref_scores_masked(ref, X, p, eps, cross=True)
    want = pattern_scores(ref, X, p, eps, cross=True)
    for key in ("recon", "latent", "assoc", "cross"):
        _same_where_defined(got[key], want[key], True, key)
    _same_where_defined(got["cost"], want["cost"], False, "cost")
    # what the patterns do not define: zeros (NaN for cross), and a row with nothing present costs nothing
    for key in ("recon", "latent", "assoc"):
        assert np.all(got[key][np.isnan(want[key])] == 0.0), key
    assert np.array_equal(np.isnan(got["cross"]), np.isnan(want["cross"]))
    empty = ~p.any(1)
    assert empty.any() and np.all(got["cost"][empty] == 0.0)
    # all present: the unmasked reference itself
    un = ref_scores(ref, X, eps, cross=True)
    full = ref_scores_masked(ref, X, np.ones((N, M), bool), eps, cross=True)
    for key in ("recon", "latent", "assoc", "cross"):
        assert np.array_equal(full[key], un[key]), key
    assert np.all(np.abs(full["cost"] - un["cost"]) <= 1e-12 * np.abs(un["cost"]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", ["N<B,K>B", "N=2B+3,K<B", "N=B,K=B"])
def test_loglik_reference_is_the_sub_model_per_pattern(case, which):
    B, M = case["B"], len(case["archs"])
    N, K = {"N<B,K>B": (B - 1, B + 4), "N=2B+3,K<B": (2 * B + 3, 3), "N=B,K=B": (B, B)}[which]
    rng, ref, X = _setup(case, 2, N)
    eps = rng.standard_normal((N, K, case["archs"][0]["n_z"]))
    p = all_patterns_mask(N, M, shift=K)
    assert B >= 1 << M and has_every_pattern(p)
    got = ref_loglik_masked(ref, X, p, eps)
    want = pattern_loglik(ref, X, p, eps)
    for key in ("marginal", "conditional"):
        _same_where_defined(got[key], want[key], True, key)
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    _same_where_defined(got["joint"], want["joint"], False, "joint")
    assert np.array_equal(np.isnan(got["joint"]), ~p)
    for s in range(M):                                       # a row with only s: joint[s] is marginal[s]
        only = p[:, s] & (p.sum(1) == 1)
        assert only.any() and np.array_equal(got["joint"][only, s], got["marginal"][only, s])
    assert np.all(np.isnan(got["marginal"][~p.any(1)])) and np.all(np.isnan(got["conditional"][~p.any(1)]))
    un = ref_loglik(ref, X, eps)
    full = ref_loglik_masked(ref, X, np.ones((N, M), bool), eps)
    for key in ("marginal", "conditional"):
        assert np.array_equal(full[key], un[key]), key
    assert np.all(np.abs(full["joint"] - un["joint"]) <= 1e-12 * np.abs(un["joint"]))


@pytest.mark.parametrize("case", CASES)
def test_absent_content_never_reaches_the_reference(case):
    N, M = 2 * case["B"] + 3, len(case["archs"])
    rng, ref, X = _setup(case, 3, N)
    eps = rng.standard_normal((N, case["archs"][0]["n_z"]))
    eps_k = rng.standard_normal((N, 3, case["archs"][0]["n_z"]))
    p = all_patterns_mask(N, M)
    p[:, M - 1] = False
    Xg = [np.where(p[:, m:m + 1], x, np.nan) for m, x in enumerate(X)]
    Xn = list(X)
    Xn[M - 1] = None
    pn = all_patterns_mask(N, M)                            # the None overrules the last column
    a, b, c = (ref_scores_masked(ref, Xa, pa, eps, cross=True) for Xa, pa in ((X, p), (Xg, p), (Xn, pn)))
    la, lb, lc = (ref_loglik_masked(ref, Xa, pa, eps_k) for Xa, pa in ((X, p), (Xg, p), (Xn, pn)))
    for x, y, z in ((a, b, c), (la, lb, lc)):
        for key in x:
            assert np.array_equal(x[key], y[key], equal_nan=True) and np.array_equal(x[key], z[key], equal_nan=True), key


@pytest.mark.parametrize("case", CASES)
def test_masked_columns_add_up_to_the_masked_cost(case):
    B, M = case["B"], len(case["archs"])
    N = 2 * B + 3
    rng, ref, X = _setup(case, 4, N)
    eps = rng.standard_normal((N, case["archs"][0]["n_z"]))
    p = all_patterns_mask(N, M, shift=1)
    _assert_chunks_have_every_pattern(p, B)
    sc = ref_scores_masked(ref, X, p, eps)
    # the masked columns need no presence: handing masked_cost_from_rows all ones gives what the true presence gives
    want = masked_cost_from_rows(sc["recon"], sc["latent"], sc["assoc"], p, case["binary"], case["weights"], case["lam"], N)
    blind = masked_cost_from_rows(sc["recon"], sc["latent"], sc["assoc"], np.ones((N, M)), case["binary"], case["weights"],
                                  case["lam"], N)
    assert abs(blind - want) <= 1e-12 * abs(want)
    # a full batch: the cost of the masked step
    Xb, pb, eb = [x[:B] for x in X], p[:B], eps[:B]
    sb = ref_scores_masked(ref, Xb, pb, eb)
    total = sum(w * (sb["latent"][:, m].sum() / B + (sb["recon"][:, m].sum() / B if b else sb["recon"][:, m].sum()))
                for m, (w, b) in enumerate(zip(case["weights"], case["binary"])))
    total += case["lam"] * sb["assoc"].sum()
    step_cost, _ = masked_cost_and_grads(case["archs"], ref.get_params(), Xb, eb, pb, case["binary"], case["weights"], case["lam"],
                                         case["act"])
    assert abs(total - step_cost) <= 1e-11 * abs(step_cost)
    # and the per-row cost column is the row's share of it (no 1/B: cost[n] is the row's own sum)
    w = np.asarray(case["weights"])
    assert np.allclose(sb["cost"], ((sb["recon"] + sb["latent"]) * w).sum(1) + case["lam"] * sb["assoc"].sum(1), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ symbols and surface
def test_masked_scoring_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    L = _capi.lib()
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "avae.h")) as f:
        header = f.read()
    for name in ("avae_score_masked", "avae_loglik_masked"):
        assert "int %s(" % name in header
        assert name in _capi.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is not None
    assert len(L.avae_score_masked.argtypes) == 9 and len(L.avae_loglik_masked.argtypes) == 9


def test_masked_scoring_methods_are_part_of_the_model_surface():
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder as A
    sig = inspect.signature(A.score_samples_masked)
    assert list(sig.parameters) == ["self", "X", "present", "eps", "cross_modal"]
    assert sig.parameters["present"].default is inspect.Parameter.empty
    assert sig.parameters["eps"].default is None and sig.parameters["cross_modal"].default is False
    sig = inspect.signature(A.log_likelihood_masked)
    assert list(sig.parameters) == ["self", "X", "present", "n_samples", "eps"]
    assert sig.parameters["n_samples"].default == 64 and sig.parameters["eps"].default is None
    # the unmasked twins keep their exact signatures
    assert list(inspect.signature(A.score_samples).parameters) == ["self", "X", "eps", "cross_modal"]
    assert list(inspect.signature(A.log_likelihood).parameters) == ["self", "X", "n_samples", "eps"]
    for fn in (dataset.DataSet.__init__, dataset.DeviceDataSet.__init__, dataset.construct_datasets):
        assert inspect.signature(fn).parameters["present"].default is None


# ------------------------------------------------------------------------------------------------ data sets
def _tagged(N, M):
    """rows whose first column is their index, presence a function of that index"""
    data = np.arange(N, dtype=np.float64)[:, None] * np.ones((1, 3))
    return data, all_patterns_mask(N, M)


def test_presence_follows_its_rows_through_split_reshuffle_and_runs():
    N, M, B = 57, 3, 8
    data, present = _tagged(N, M)
    np.random.seed(11)
    ds = dataset.construct_datasets(data.copy(), present=present.copy())
    for split in (ds.train, ds.validation, ds.test):
        assert np.array_equal(split._present, present[split._data[:, 0].astype(int)])
    assert ds.train.last_present().shape == (0, M)
    seen_wrap = False
    for i in range(30):
        before = ds.train._epochs_completed
        if i % 3 == 2:
            d, _l, n = ds.train.next_batches(B, 3)
        else:
            (d, _l), n = ds.train.next_batch(B), 1
        seen_wrap |= ds.train._epochs_completed > before
        p = ds.train.last_present()
        assert d.shape[0] == n * B and p.shape == (n * B, M)
        assert np.array_equal(p, present[d[:, 0].astype(int)])
        assert ds.train.last_rows() == (ds.train._index_in_epoch - n * B, ds.train._index_in_epoch)
    assert seen_wrap
    # labels, presence and data all together
    np.random.seed(3)
    ds = dataset.construct_datasets(data.copy(), labels=data[:, :1] * 10, present=present.copy())
    d, l = ds.train.next_batch(5)
    assert np.array_equal(l[:, 0], d[:, 0] * 10) and np.array_equal(ds.train.last_present(), present[d[:, 0].astype(int)])
    with pytest.raises(ValueError):
        dataset.DataSet(data, present=present[:-1])


def test_without_presence_nothing_changes():
    """the batch order of the reference fixture, the number of np.random calls, and no presence anywhere"""
    z = np.load(os.path.join(GOLDEN, "dataset_order.npz"), allow_pickle=False)
    np.random.seed(int(z["seed"]))
    ds = dataset.construct_datasets(z["data"].copy(), validation_ratio=.1, test_ratio=.1)
    B = int(z["batch"])
    for want in z["batches"]:
        got, lab = ds.train.next_batch(B)
        assert lab is None and np.array_equal(got[:, 0], want)
        assert ds.train.last_present() is None
    after_plain = np.random.random()
    # the same walk with presence: the same rows and the same state of NumPy's generator afterwards
    np.random.seed(int(z["seed"]))
    n = z["data"].shape[0]
    dp = dataset.construct_datasets(z["data"].copy(), validation_ratio=.1, test_ratio=.1, present=all_patterns_mask(n, 2))
    for want in z["batches"]:
        got, _lab = dp.train.next_batch(B)
        assert np.array_equal(got[:, 0], want)
    assert np.random.random() == after_plain


# ------------------------------------------------------------------------------------------------ train_loop
T_ARCHS = [make_arch("image", 60, 20, 16, 5), make_arch("joint", 21, 12, 10, 5)]
T_BIN, T_W, T_LAM, T_LR = [True, False], [50.0, 1.0], 8.0, 1e-3


class MaskedOracleReplica(object):
    """The model surface train_loop drives, on the CPU oracle: masked cost and gradient from tests/masked_reference.py, the
    oracle's Adam.  Records the (data rows, presence rows) every call was handed.  ``steps`` adds partial_fit_steps /
    cost_history, so both branches of the loop are driven."""

    def __init__(self, B, params, eps_all, steps):
        self.model = O.OracleAssocVAE(T_ARCHS, T_BIN, "relu", T_W, T_LAM, T_LR, B, params_flat=params)
        self.B, self.eps_all, self.k, self.calls, self.costs = B, eps_all, 0, [], []
        if steps:
            self.partial_fit_steps = self._steps
            self.cost_history = lambda n: np.asarray(self.costs[-n:])

    def _cost_grad(self, X, present, kind):
        X = [np.asarray(x, np.float64) for x in X]
        self.calls.append((kind, X[0][:, 0].copy(), None if present is None else np.asarray(present).copy()))
        if present is None:
            c, g, _ = self.model.cost_and_grads(X, self.eps_all[self.k])
        else:
            c, g = masked_cost_and_grads(T_ARCHS, self.model.get_params(), X, self.eps_all[self.k], present, T_BIN, T_W, T_LAM, "relu")
        self.k += 1
        return float(c), g

    def partial_fit(self, X, eps=None, return_cost=True, present=None):
        c, g = self._cost_grad(X, present, "fit")
        self.model.apply_gradients(g)
        self.costs.append(c)
        return c

    def _steps(self, X, n_steps, eps=None, return_cost=True, present=None):
        for i in range(n_steps):
            rows = slice(i * self.B, (i + 1) * self.B)
            self.partial_fit([x[rows] for x in X], present=None if present is None else present[rows])

    def evaluate_cost(self, X, eps=None, present=None):
        return self._cost_grad(X, present, "eval")[0]


def _train_data(N):
    rng = np.random.default_rng(31)
    data = np.concatenate(synth_batch(rng, N, [60, 21], T_BIN), axis=1).astype(np.float64)
    data[:, 0] = np.arange(N) / float(N)                    # column 0 names the row (and stays a Bernoulli target in [0, 1))
    eps_all = rng.standard_normal((200, 8, 5))
    p0 = O.flatten_params(T_ARCHS, O.init_params(T_ARCHS, np.random.default_rng(0))) + 0.01 * rng.standard_normal(O.param_count(T_ARCHS))
    return data, eps_all, p0


def _hand_loop(data, present, p0, eps_all, B, epochs, early_stop):
    np.random.seed(9)
    ds = dataset.construct_datasets(data.copy(), present=present.copy())
    ref = O.OracleAssocVAE(T_ARCHS, T_BIN, "relu", T_W, T_LAM, T_LR, B, params_flat=p0)
    lookup = {float(v): i for i, v in enumerate(data[:, 0])}
    n = ds.train._data.shape[0]
    k, hist, valid = 0, [], None
    for epoch in range(epochs):
        avg = 0.0
        if epoch % early_stop == 0:
            nv = ds.validation._data.shape[0] // B
            cur = 0
            for _ in range(nv):
                x, _l = ds.validation.next_batch(B)
                pr = present[[lookup[float(v)] for v in x[:, 0]]]           # presence looked up by row identity, not carried
                cur += masked_cost_and_grads(T_ARCHS, ref.get_params(), [x[:, :60], x[:, 60:]], eps_all[k], pr, T_BIN, T_W, T_LAM,
                                             "relu")[0] / nv
                k += 1
            if valid is not None and cur > valid:
                break
            valid = cur
        for _ in range(n // B):
            x, _l = ds.train.next_batch(B)
            pr = present[[lookup[float(v)] for v in x[:, 0]]]
            c, g = masked_cost_and_grads(T_ARCHS, ref.get_params(), [x[:, :60], x[:, 60:]], eps_all[k], pr, T_BIN, T_W, T_LAM, "relu")
            k += 1
            ref.apply_gradients(g)
            avg += float(c) / n * B
            hist.append(avg)
    return hist, ref.get_params()


@pytest.mark.parametrize("steps", [False, True])
def test_train_loop_hands_every_step_its_presence_rows(steps):
    from vae_assoc_amd.vae_assoc import train_loop
    N, B, epochs, M = 100, 8, 3, 2
    data, eps_all, p0 = _train_data(N)
    present = all_patterns_mask(N, M, shift=2)
    assert B >= 1 << M
    lookup = {float(v): i for i, v in enumerate(data[:, 0])}
    np.random.seed(9)
    ds = dataset.construct_datasets(data.copy(), present=present.copy())
    rep = MaskedOracleReplica(B, p0, eps_all, steps)
    _m, hist = train_loop(rep, ds, T_ARCHS, B, training_epochs=epochs, display_step=10, early_stop=1)
    # every call got the presence rows of exactly its data rows
    assert rep.calls and any(kind == "eval" for kind, _r, _p in rep.calls)
    for kind, rows, pr in rep.calls:
        assert pr is not None and pr.shape == (B, M), kind
        assert np.array_equal(pr != 0, present[[lookup[float(v)] for v in rows]]), kind
    h_ref, p_ref = _hand_loop(data, present, p0, eps_all, B, epochs, 1)
    assert len(hist) == len(h_ref) > 0
    assert np.array_equal(np.asarray(hist), np.asarray(h_ref))
    assert np.array_equal(rep.model.get_params(), p_ref)


def test_train_loop_without_presence_issues_todays_calls_and_refuses_presence_on_many_ranks():
    import types
    from vae_assoc_amd.vae_assoc import train_loop
    N, B = 100, 8
    data, eps_all, p0 = _train_data(N)
    np.random.seed(9)
    ds = dataset.construct_datasets(data.copy())
    rep = MaskedOracleReplica(B, p0, eps_all, True)
    train_loop(rep, ds, T_ARCHS, B, training_epochs=2, display_step=10, early_stop=1)
    assert rep.calls and all(pr is None for _k, _r, pr in rep.calls)
    # presence + a data-parallel model: refused before any step (and before the first collective)
    np.random.seed(9)
    dp = dataset.construct_datasets(data.copy(), present=all_patterns_mask(N, 2))
    rep = MaskedOracleReplica(B, p0, eps_all, True)
    with pytest.raises(RuntimeError, match="one replica"):
        train_loop(rep, dp, T_ARCHS, B, training_epochs=1, sync=types.SimpleNamespace(world_size=2, rank=0))
    assert not rep.calls
