"""AVAE_NO_LD_SPREAD is read per handle, not once per process (avae_host.hip: PlanSwitches, spread_ld).  avae_workspace_bytes
plans the memory of a temporary handle on the host, so no GPU is needed: one process sizes the same model with the switch set and
without, and each size is the one a fresh process gives under the same setting.

Model: bf16, hidden width 256 -- a W-shadow row of 256 bf16 is 512 bytes, the stride spread_ld pads by one K unit."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT

SWITCH = "AVAE_NO_LD_SPREAD"


def _bytes(capi):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = 2
    for m, n_in in enumerate((784, 147)):
        cfg.mod[m].n_input = n_in
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = 256
        cfg.mod[m].binary = 1 - m
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = 20, 64, 1, capi.DTYPE_IDS["bf16"]
    cfg.learning_rate, cfg.assoc_lambda = 1e-3, 1.0
    n = C.c_size_t(0)
    assert capi.lib().avae_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    return n.value


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def _fresh_process(switch_on):
    env = {k: v for k, v in os.environ.items() if k != SWITCH}
    if switch_on:
        env[SWITCH] = "1"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_plan_switches_cpu as t; from vae_assoc_amd import _capi; print(t._bytes(_capi))"
            % (ROOT, os.path.join(ROOT, "tests")))
    return int(subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, check=True, capture_output=True, text=True).stdout.split()[-1])


def test_ld_spread_switch_is_per_handle(capi, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    spread = _bytes(capi)                    # the process's first plan: a per-process cache would keep this setting
    monkeypatch.setenv(SWITCH, "1")
    plain = _bytes(capi)
    monkeypatch.delenv(SWITCH)
    assert _bytes(capi) == spread
    assert plain != spread
    assert spread == _fresh_process(False) and plain == _fresh_process(True)
