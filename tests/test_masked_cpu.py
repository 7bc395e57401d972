"""CPU checks of partially paired training (include/avae.h): the pattern-composed fp64 reference of
tests/masked_reference.py against the oracle and against finite differences, the per-row identity of the masked cost, and the
masked entry points' presence in the C ABI and the model surface."""
import inspect

import numpy as np
import pytest

from conftest import make_arch, synth_batch
from masked_reference import masked_cost_and_grads, masked_cost_from_rows, patterns, per_row_terms
from oracle import vae_assoc_oracle as O

CASES = [
    dict(archs=[make_arch("image", 30, 12, 10, 4), make_arch("joint", 9, 8, 6, 4)], binary=[True, False],
         weights=[3.0, 1.0], lam=0.8, act="softplus", B=7),
    dict(archs=[make_arch("a", 14, 10, 8, 3), make_arch("b", 11, 8, 6, 3), make_arch("c", 9, 6, 6, 3)],
         binary=[True, False, False], weights=[2.0, 1.0, 0.5], lam=0.7, act="tanh", B=9),
]


def _setup(case, seed):
    rng = np.random.default_rng(seed)
    archs = case["archs"]
    flat = O.flatten_params(archs, O.init_params(archs, rng))
    X = [x.astype(np.float64) for x in synth_batch(rng, case["B"], [na["n_input"] for na in archs], case["binary"])]
    eps = rng.standard_normal((case["B"], archs[0]["n_z"]))
    return rng, flat, X, eps


def _random_mask(rng, B, M):
    p = rng.random((B, M)) < 0.6
    p[0] = False                       # a row with nothing present
    p[1] = True                        # a fully paired row
    p[2] = False
    p[2, M - 1] = True                 # a single-modality row
    return p


@pytest.mark.parametrize("case", CASES)
def test_all_present_is_the_oracle_step(case):
    _, flat, X, eps = _setup(case, 1)
    archs, B = case["archs"], case["B"]
    ref = O.OracleAssocVAE(archs, binary=case["binary"], transfer_fct=case["act"], weights=case["weights"],
                           assoc_lambda=case["lam"], batch_size=B, params_flat=flat)
    c0, g0, _ = ref.cost_and_grads(X, eps)
    c1, g1 = masked_cost_and_grads(archs, flat, X, eps, np.ones((B, len(archs)), bool), case["binary"], case["weights"],
                                   case["lam"], case["act"])
    assert abs(c1 - c0) <= 1e-12 * abs(c0)
    np.testing.assert_allclose(g1, g0, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("case", CASES)
def test_masked_gradient_by_central_differences(case):
    rng, flat, X, eps = _setup(case, 2)
    archs, B, M = case["archs"], case["B"], len(case["archs"])
    p = _random_mask(rng, B, M)

    def cost(th):
        return masked_cost_and_grads(archs, th, X, eps, p, case["binary"], case["weights"], case["lam"], case["act"])[0]

    _, g = masked_cost_and_grads(archs, flat, X, eps, p, case["binary"], case["weights"], case["lam"], case["act"])
    idx = rng.choice(flat.size, 60, replace=False)
    h = 1e-6
    for i in idx:
        e = np.zeros_like(flat)
        e[i] = h
        fd = (cost(flat + e) - cost(flat - e)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, g[i])


@pytest.mark.parametrize("case", CASES)
def test_masked_cost_is_the_per_row_formula(case):
    rng, flat, X, eps = _setup(case, 3)
    archs, B, M = case["archs"], case["B"], len(case["archs"])
    p = _random_mask(rng, B, M)
    recon, latent, assoc = per_row_terms(archs, flat, X, eps, case["binary"], case["act"])
    want = masked_cost_from_rows(recon, latent, assoc, p, case["binary"], case["weights"], case["lam"], B)
    got, _ = masked_cost_and_grads(archs, flat, X, eps, p, case["binary"], case["weights"], case["lam"], case["act"])
    assert abs(got - want) <= 1e-11 * max(1.0, abs(want))


def test_absent_modality_gets_no_gradient_and_absent_content_is_ignored():
    case = CASES[1]
    rng, flat, X, eps = _setup(case, 4)
    archs, B, M = case["archs"], case["B"], len(case["archs"])
    p = _random_mask(rng, B, M)
    p[:, 1] = False
    c, g = masked_cost_and_grads(archs, flat, X, eps, p, case["binary"], case["weights"], case["lam"], case["act"])
    n = [sum(int(np.prod(s)) for _, s in O.layer_shapes(na)) for na in archs]
    assert np.all(g[n[0]:n[0] + n[1]] == 0)
    X2 = list(X)
    X2[1] = None                                            # never read
    X3 = [x.copy() for x in X]
    X3[0][~p[:, 0]] = np.nan                               # absent entries of a present column
    for Xa in (X2, X3):
        c2, g2 = masked_cost_and_grads(archs, flat, Xa, eps, p, case["binary"], case["weights"], case["lam"], case["act"])
        assert c2 == c and np.array_equal(g2, g)


def test_empty_mask_is_zero_and_patterns_group_rows():
    case = CASES[0]
    _, flat, X, eps = _setup(case, 5)
    B, M = case["B"], 2
    c, g = masked_cost_and_grads(case["archs"], flat, X, eps, np.zeros((B, M), bool), case["binary"], case["weights"],
                                 case["lam"], case["act"])
    assert c == 0.0 and not np.any(g)
    pat = patterns(np.array([[1, 0], [0, 0], [1, 1], [1, 0], [0, 1]]))
    assert {k: v.tolist() for k, v in pat.items()} == {(0,): [0, 3], (0, 1): [2], (1,): [4]}


def test_masked_entry_points_are_in_the_abi_and_the_model_surface():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    L = _capi.lib()
    for name in ("avae_train_steps_masked", "avae_eval_cost_masked"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    for meth in ("partial_fit", "partial_fit_steps", "evaluate_cost"):
        sig = inspect.signature(getattr(AssocVariationalAutoEncoder, meth))
        assert "present" in sig.parameters and sig.parameters["present"].default is None
