"""CPU checks of the scoring entry points of the C ABI: avae_score_width is host-only (no GPU), sizes a score row as
1 + 2M + P (+ M*M with AVAE_SCORE_CROSS) and rejects unknown flags with a message."""
import ctypes as C
import inspect

import pytest


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def _config(capi, n_mod):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = n_mod
    for m in range(n_mod):
        cfg.mod[m].n_input = 40 + 10 * m
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = 32
        cfg.mod[m].binary = m % 2
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = 8, 16, 1, 1
    return cfg


def _width(capi, cfg, flags):
    k = C.c_int32(-1)
    rc = capi.lib().avae_score_width(C.byref(cfg), flags, C.byref(k))
    return rc, k.value


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_score_width(capi, M):
    cfg = _config(capi, M)
    P = M * (M - 1) // 2
    assert _width(capi, cfg, 0) == (0, 1 + 2 * M + P)
    assert _width(capi, cfg, capi.SCORE_CROSS) == (0, 1 + 2 * M + P + M * M)


def test_score_width_rejects_unknown_flags_and_bad_configs(capi):
    L = capi.lib()
    cfg = _config(capi, 2)
    for flags in (2, 4, 0x100, -1):
        rc, _ = _width(capi, cfg, flags)
        assert rc != 0
        assert "flags" in L.avae_last_error(None).decode()
    cfg.n_modalities = 5
    rc, _ = _width(capi, cfg, 0)
    assert rc != 0 and "n_modalities" in L.avae_last_error(None).decode()
    k = C.c_int32(0)
    assert L.avae_score_width(None, 0, C.byref(k)) != 0


def test_score_samples_is_part_of_the_model_surface():
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    sig = inspect.signature(AssocVariationalAutoEncoder.score_samples)
    assert list(sig.parameters) == ["self", "X", "eps", "cross_modal"]
    assert sig.parameters["eps"].default is None and sig.parameters["cross_modal"].default is False
