"""Parameter averaging without a GPU: the reference statement (tests/ema_reference.py) against the closed forms, the argument
checks of the Python surface (vae_assoc_amd/_marshal.py) and the binding's symbol list."""
import numpy as np
import pytest

from ema_reference import F32, decay_t, ema_run, ema_step, one_minus_decay


def test_constant_parameters_keep_the_average():
    rng = np.random.default_rng(0)
    th = rng.standard_normal(257).astype(np.float32)
    for warmup in (False, True):
        e = ema_run(th, [th] * 12, 0.999, warmup)
        assert np.array_equal(e, th.astype(np.float64))          # theta - e == 0: nothing is added, not even a rounding


def test_warmup_factors():
    """(1 + t) / (10 + t): 2/11, 3/12, ... until it exceeds decay; from then on decay."""
    decay = 0.9
    got = [decay_t(decay, True, t) for t in range(1, 120)]
    assert all(isinstance(g, np.float32) for g in got)
    for t, g in enumerate(got, start=1):
        exact = (1.0 + t) / (10.0 + t)
        if exact < 0.9 - 1e-6:
            assert g == F32(F32(1 + t) / F32(10 + t)) and abs(float(g) - exact) <= 2.0 ** -24
        elif exact > 0.9 + 1e-6:
            assert g == F32(decay)
    assert got[0] == F32(F32(2) / F32(11)) and got[1] == F32(0.25) and got[2] == F32(F32(4) / F32(13))
    first_decay = next(t for t, g in enumerate(got, start=1) if g == F32(decay))
    assert first_decay == 80                                     # (1 + t) / (10 + t) >= 0.9  <=>  t >= 80 (81 / 90 rounds to float32(0.9) itself)
    assert all(g == F32(decay) for g in got[first_decay:])
    assert np.all(np.diff(np.array(got, np.float64)) >= 0)
    # without warm-up the step does not matter
    assert {decay_t(decay, False, t) for t in (1, 7, 10 ** 6)} == {F32(decay)}
    assert one_minus_decay(decay, False, 3) == F32(1.0) - F32(decay)
    # a step number beyond float32's integers still gives decay
    assert decay_t(0.999, True, 2 ** 40) == F32(0.999)


def test_closed_geometric_form():
    """Without warm-up, n steps from e0: e_n = d^n e0 + (1 - d) sum_k d^(n-1-k) theta_k, d the float32 decay."""
    rng = np.random.default_rng(1)
    n, decay = 9, 0.75
    e0 = rng.standard_normal(33)
    th = rng.standard_normal((n, 33))
    d = 1.0 - float(one_minus_decay(decay, False, 1))
    want = d ** n * e0 + (1.0 - d) * sum(d ** (n - 1 - k) * th[k] for k in range(n))
    got = ema_run(e0, th, decay, False)
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(th))
    # one step is the convex combination
    one = ema_step(e0, th[0], decay, False, 1)
    assert np.allclose(one, d * e0 + (1 - d) * th[0], rtol=0, atol=1e-15)


def test_marshal_rejects_bad_arguments():
    from vae_assoc_amd import _marshal as M
    assert M.ema_fields(0.999) == (float(F32(0.999)), 0)
    assert M.ema_fields(0.5, True) == (0.5, 1)
    assert M.ema_fields(None) == (0.0, 0) and M.ema_fields(0) == (0.0, 0)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-9):      # (the last rounds to 1.0f)
        with pytest.raises(ValueError, match="decay must be in"):
            M.ema_fields(bad)
    for bad in ("0.9", True, [0.9]):
        with pytest.raises(ValueError, match="decay must be a number"):
            M.ema_fields(bad)
    for bad in (2, -1, "yes", None):
        with pytest.raises(ValueError, match="warmup must be True or False"):
            M.ema_fields(0.9, bad)
    assert M.ema_kwargs(None) == {}
    assert M.ema_kwargs(0.99) == {"decay": 0.99}
    assert M.ema_kwargs(dict(decay=0.99, warmup=True)) == {"decay": 0.99, "warmup": True}
    with pytest.raises(ValueError, match=r"ema: unknown key\(s\) rate"):
        M.ema_kwargs(dict(decay=0.9, rate=1))
    with pytest.raises(ValueError, match="ema: the dict needs a decay"):
        M.ema_kwargs(dict(warmup=True))
    with pytest.raises(ValueError, match="decay must be in"):
        M.ema_kwargs(dict(decay=2.0))
    with pytest.raises(ValueError, match="decay must be in"):
        M.ema_kwargs(-1)


def test_binding_lists_the_new_symbols():
    from vae_assoc_amd import _capi
    for name in ("avae_set_ema", "avae_get_ema", "avae_set_ema_params", "avae_use_averaged"):
        assert name in _capi.SYMBOLS
    assert len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
