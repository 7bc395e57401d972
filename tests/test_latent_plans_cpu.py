"""The five *_plan entry points of the latent-space features (host-only, no GPU) against tests/golden/latent_plans.json: every output
field at row counts on both sides of every boundary of the five partitions (one slice -> two, the min_rows floor -> the max_slices
ceiling, kTopkChunkRows, kTopkMaxSplits, kTopkMinTilesPerSplit).  The partitions are determinism contracts (the order of every sum
follows from them), so a change of one number here is a change of results.

The table was recorded from the library as it was before the plans were rebuilt on row_slices / tile_splits
(csrc/avae_latent_common.h), with this file's own recorder:  python tests/test_latent_plans_cpu.py --record"""
import ctypes as C
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_plans.json")
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 16383, 16384, 16385, 65535, 65536, 262145, 2 ** 31 - 1]
KS = [1, 5, 64]                 # k of the top-k, n_components of the mixture
NZS = [1, 20, 64]
MODS = [1, 4]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


def _config(capi, n_z, n_mod=2):
    cfg = capi.Config()
    cfg.abi_version = capi.AVAE_ABI_VERSION
    cfg.n_modalities = n_mod
    for m in range(n_mod):
        cfg.mod[m].n_input = 147
        cfg.mod[m].n_hidden_layers = 2
        cfg.mod[m].n_hidden[0] = cfg.mod[m].n_hidden[1] = 72
        cfg.mod[m].binary = 0
        cfg.mod[m].weight = 1.0
    cfg.n_z, cfg.batch_size, cfg.activation, cfg.compute_dtype = n_z, 16, 1, 0
    cfg.learning_rate, cfg.assoc_lambda = 1e-3, 1.0
    return cfg


def _call(capi, fn, cfg, args, n_int):
    """fn(cfg, *args, n_int int32 outputs, one size_t output) -> the outputs, or the error text"""
    outs = [C.c_int32(-7) for _ in range(n_int)] + [C.c_size_t(7)]
    if fn(C.byref(cfg), *args, *[C.byref(o) for o in outs]) != 0:
        return capi.lib().avae_last_error(None).decode()
    return [o.value for o in outs]


def _table(capi):
    L = capi.lib()
    cfgs = {nz: _config(capi, nz) for nz in NZS}
    t = {"topk": {}, "agg": {}, "stats": {}, "gmm": {}, "embed": {}}
    for rows in ROWS:
        for G in ROWS:
            for k in KS:          # query_tile, gallery_tile, n_splits, scratch_bytes
                t["topk"]["%d,%d,%d" % (rows, G, k)] = _call(capi, L.avae_latent_topk_plan, cfgs[20], (rows, G, k), 3)
            for nz in NZS:        # query_tile, chunk_rows, slice_rows, n_slices, scratch_bytes
                t["agg"]["%d,%d,%d" % (rows, G, nz)] = _call(capi, L.avae_agg_logpdf_plan, cfgs[nz], (rows, G), 4)
        for nz in NZS:
            for M in MODS:        # row_tile, n_slices, scratch_bytes
                t["stats"]["%d,%d,%d" % (rows, nz, M)] = _call(capi, L.avae_latent_stats_plan, _config(capi, nz, M), (rows,), 2)
            for K in KS:          # slice_rows, n_slices, scratch_bytes
                t["gmm"]["%d,%d,%d" % (rows, K, nz)] = _call(capi, L.avae_gmm_plan, cfgs[nz], (rows, K), 2)
        if rows <= 65536:         # row_tile, n_splits, tiles_per_split, scratch_bytes
            t["embed"]["%d" % rows] = _call(capi, L.avae_embed_plan, cfgs[20], (rows,), 3)
    t["embed"]["65537"] = _call(capi, L.avae_embed_plan, cfgs[20], (65537,), 3)
    return t


def test_every_plan_field_is_the_recorded_one(capi):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _table(capi)
    assert sorted(got) == sorted(want)
    for feature in want:
        assert sorted(got[feature]) == sorted(want[feature]), feature
        for case, fields in want[feature].items():
            assert got[feature][case] == fields, (feature, case)
    assert isinstance(want["embed"]["65537"], str) and "65536" in want["embed"]["65537"]       # the one recorded error


def test_topk_and_embed_plans_do_not_depend_on_n_z(capi):
    L = capi.lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    for nz in (1, 64):
        cfg = _config(capi, nz)
        for case, fields in want["topk"].items():
            assert _call(capi, L.avae_latent_topk_plan, cfg, tuple(int(x) for x in case.split(",")), 3) == fields, (nz, case)
        for case, fields in want["embed"].items():
            assert _call(capi, L.avae_embed_plan, cfg, (int(case),), 3) == fields, (nz, case)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_latent_plans_cpu.py --record"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    with open(GOLDEN, "w") as f:
        json.dump(_table(_capi), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
