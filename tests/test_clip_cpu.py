"""CPU checks of global-norm gradient clipping / non-finite step skipping: the fp64 reference (tests/clip_reference.py) against
the oracle's own optimiser, the Python argument validation (no device needed) and the two new exports of libavae.so."""
import ctypes as C

import numpy as np
import pytest

from clip_reference import clip_factor, clipped_step, global_norm
from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O

ARCHS = [make_arch("image", 784, 24, 24, 4), make_arch("joint", 147, 12, 12, 4)]
BIN, W, LAM, LR, B = [True, False], [50, 1], 8.0, 1e-3, 32


def _pair(seed=3):
    rng = np.random.default_rng(seed)
    p0 = O.flatten_params(ARCHS, O.init_params(ARCHS, rng))
    X = synth_batch(rng, B, [784, 147], BIN)
    eps = rng.standard_normal((3, B, 4))
    mk = lambda: O.OracleAssocVAE(ARCHS, BIN, "relu", W, LAM, LR, B, params_flat=p0.copy())
    return mk, X, eps


def test_below_the_threshold_is_the_plain_step():
    mk, X, eps = _pair()
    a, b = mk(), mk()
    for s in range(3):
        ca = a.partial_fit(X, eps[s])
        r = clipped_step(b, X, eps[s], max_norm=float("inf") if s == 0 else 1e30)
        assert r["c"] == 1.0 and not r["skipped"] and r["cost"] == ca
        assert np.array_equal(a.get_params(), b.get_params()) and np.array_equal(a.m, b.m) and np.array_equal(a.v, b.v)
    assert a.t == b.t == 3


def test_above_the_threshold_scales_to_max_norm():
    mk, X, eps = _pair()
    a, b = mk(), mk()
    _, g, _ = a.cost_and_grads(X, eps[0])
    n0 = global_norm(g)
    mx = 0.5 * n0
    th0, m0, v0 = b.get_params(), b.m.copy(), b.v.copy()
    r = clipped_step(b, X, eps[0], max_norm=mx)
    assert r["norm"] == n0 and abs(r["c"] - 0.5) <= 1e-15
    assert abs(global_norm(r["gc"]) - mx) <= 1e-12 * mx
    assert np.array_equal(r["g"], g)                                   # the raw gradient is what is reported
    th, m, v = O.adam_step(th0, m0, v0, r["gc"], 1, LR)
    assert np.array_equal(b.get_params(), th) and np.array_equal(b.m, m) and np.array_equal(b.v, v)
    assert clip_factor(float("nan"), 1.0) == 1.0 and clip_factor(3.0, 0.0) == 1.0 and clip_factor(3.0, float("inf")) == 1.0


def test_nonfinite_gradient_is_skipped_and_still_counts():
    mk, X, eps = _pair()
    b = mk()
    clipped_step(b, X, eps[0], skip_nonfinite=True)
    th0, m0, v0, t0 = b.get_params(), b.m.copy(), b.v.copy(), b.t
    bad = [X[0], X[1].copy()]
    bad[1][5, 7] = np.nan
    r = clipped_step(b, bad, eps[1], skip_nonfinite=True)
    assert r["skipped"] and not np.isfinite(r["norm"]) and np.isnan(r["cost"])
    assert np.array_equal(b.get_params(), th0) and np.array_equal(b.m, m0) and np.array_equal(b.v, v0)
    assert b.t == t0 + 1
    r = clipped_step(b, X, eps[2], skip_nonfinite=True)
    assert not r["skipped"] and b.t == t0 + 2 and np.all(np.isfinite(b.get_params()))


def test_python_argument_validation_needs_no_device():
    from vae_assoc_amd._marshal import grad_clip_fields, grad_clip_kwargs
    assert grad_clip_fields(0.0, False) == (0.0, 0)
    assert grad_clip_fields(None, True) == (0.0, 1)
    assert grad_clip_fields(float("inf"), 0) == (float("inf"), 0)
    assert grad_clip_fields(0.1, 1) == (float(np.float32(0.1)), 1)
    for bad in (-1.0, float("nan"), -0.5, "3", [1.0], True):
        with pytest.raises(ValueError, match="max_norm"):
            grad_clip_fields(bad, False)
    assert grad_clip_kwargs(None) == {}
    assert grad_clip_kwargs(2.5) == {"max_norm": 2.5}
    assert grad_clip_kwargs(dict(skip_nonfinite=True)) == {"skip_nonfinite": True}
    with pytest.raises(ValueError, match="max_norm"):
        grad_clip_kwargs(dict(max_norm=float("nan")))
    with pytest.raises(ValueError, match="max_nrom"):
        grad_clip_kwargs(dict(max_nrom=1.0))
    # the constructor refuses a bad value before it looks for a device
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    with pytest.raises(ValueError, match="max_norm"):
        AssocVariationalAutoEncoder(ARCHS, binary=BIN, transfer_fct="relu", weights=W, batch_size=B, grad_clip=-2.0)


def test_library_exports_the_clip_entry_points():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    L = _capi.lib()
    for name in ("avae_set_grad_clip", "avae_grad_norm_history"):
        assert name in _capi.SYMBOLS
        assert hasattr(L, name), "libavae.so does not export %s" % name
    assert L.avae_set_grad_clip(None, C.c_float(1.0), 0) != 0           # a null handle is refused, not dereferenced
    assert L.avae_grad_norm_history(None, 0, None, None, None) != 0
