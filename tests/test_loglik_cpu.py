"""CPU checks of the importance-weighted log-likelihoods: avae_loglik is declared, exported and bound, log_likelihood is part of
the model surface, and the NumPy reference of scoring_reference meets two closed forms on the oracle (the K = 1 identity with
O.forward's reconstruction, and Jensen's inequality)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_arch, synth_batch
from oracle import vae_assoc_oracle as O
from scoring_reference import logsumexp, recon_rows, ref_loglik


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def test_avae_loglik_is_declared_exported_and_bound(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avae.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+avae_loglik\s*\(", txt)
    assert "avae_loglik" in capi.SYMBOLS
    L = capi.lib()
    assert hasattr(L, "avae_loglik")
    assert len(L.avae_loglik.argtypes) == 8


def test_log_likelihood_is_part_of_the_model_surface():
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    sig = inspect.signature(AssocVariationalAutoEncoder.log_likelihood)
    assert list(sig.parameters) == ["self", "X", "n_samples", "eps"]
    assert sig.parameters["n_samples"].default == 64 and sig.parameters["eps"].default is None


def _oracle(seed=3):
    archs = [make_arch("image", 64, 24, 16, 6), make_arch("joint", 20, 16, 12, 6), make_arch("third", 12, 12, 8, 6)]
    binary = [True, False, False]
    ref = O.OracleAssocVAE(archs, binary, "softplus", [2.0, 1.0, 0.5], 0.7, 1e-3, 8, seed=seed)
    return ref, archs, binary, np.random.default_rng(seed)


def test_reference_k1_identity_on_the_oracle():
    """K = 1: conditional[n, m, m] = -recon[n, m] and marginal[n, m] = -recon[n, m] + r[n, m], with recon from O.forward at that
    eps and r = sum(-z^2/2 + eps^2/2 + lv/2) of that forward pass."""
    ref, archs, binary, rng = _oracle()
    N = 11
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, 6))
    fw = O.forward(archs, ref.params, [x.astype(np.float64) for x in X], eps, binary, ref.act)
    ll = ref_loglik(ref, X, eps[:, None, :])
    for m, (f, x, b) in enumerate(zip(fw, X, binary)):
        recon = recon_rows(x.astype(np.float64), f["xhat"], b)
        r = np.sum(-0.5 * f["z"] ** 2 + 0.5 * eps ** 2 + 0.5 * f["lv"], axis=1)
        np.testing.assert_allclose(ll["conditional"][:, m, m], -recon, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ll["marginal"][:, m], -recon + r, rtol=1e-12, atol=1e-12)
    # the joint at K = 1 is the sum of the per-modality terms plus r of its proposal
    r0 = np.sum(-0.5 * fw[0]["z"] ** 2 + 0.5 * eps ** 2 + 0.5 * fw[0]["lv"], axis=1)
    np.testing.assert_allclose(ll["joint"][:, 0], ll["conditional"][:, 0, :].sum(1) + r0, rtol=1e-12)


def test_reference_jensen_on_the_oracle():
    """K samples against the K single-sample values on the same eps slices: log-mean-exp, so >= their mean and <= their max."""
    ref, archs, binary, rng = _oracle(5)
    N, K = 7, 9
    X = synth_batch(rng, N, [a["n_input"] for a in archs], binary)
    eps = rng.standard_normal((N, K, 6))
    full = ref_loglik(ref, X, eps)
    ones = [ref_loglik(ref, X, eps[:, k:k + 1]) for k in range(K)]
    for key in full:
        per_k = np.stack([o[key] for o in ones], 0)
        assert np.all(full[key] >= per_k.mean(0) - 1e-9), key
        assert np.all(full[key] <= per_k.max(0) + 1e-9), key
        np.testing.assert_allclose(full[key], logsumexp(per_k, 0) - np.log(K), rtol=1e-12)
        assert np.any(full[key] > per_k.mean(0) + 1e-6), key          # the bound is strict somewhere: K samples tighten it
