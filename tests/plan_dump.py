"""The training step's launch plan as the library runs it, read from its AVAE_DEBUG_SYNC=1 dump (test-side only).

A handle created with AVAE_DEBUG_SYNC=1 runs eagerly and prints, for every launch, a header
``[avae] launch NAME type=T cfg=C items=N blocks=K`` and one ``item kind= M= N= K= ...`` line per GEMM item of a grouped NT
launch.  Weight-gradient (TN) launches print the header only: their items live in the compact TnItem table, so their list is
empty here and a test takes their shapes (M = in + 1, N = out, K = batch) from the model's layer shapes.

Tile configurations (avae_host.hip::finish_launch): 0 = 64x64, 1 = 128x128, 2 = 256x128 8-wave NT/TN, 3 = 32x64, 4 = 64x128
(wide-latent heads), 5 = 32x32, 6 = 256x64 8-wave loss, 7/9/10/11 = the lean small-net kernels, 12 = small-net weight gradients
with Adam in the epilogue."""
import re

import numpy as np

K_FWD_HIDDEN, K_FWD_HEAD, K_FWD_OUT_LOSS, K_DGRAD_HIDDEN, K_DGRAD_LATENT, K_WGRAD, K_LATENT = 0, 1, 2, 4, 5, 6, 7

_HEAD = re.compile(r"^\[avae\] launch (\S+) type=(-?\d+) cfg=(-?\d+) items=(-?\d+) blocks=(-?\d+)\s*$")
_ITEM = re.compile(r"^\s+item kind=(-?\d+) M=(-?\d+) N=(-?\d+) K=(-?\d+) ")


def parse(text):
    """[(name, cfg, [(kind, M, N, K), ...]), ...] of the grouped GEMM launches (type 0) in dump order"""
    out = []
    cur = None
    for ln in text.splitlines():
        h = _HEAD.match(ln)
        if h:
            cur = (h.group(1), int(h.group(3)), []) if int(h.group(2)) == 0 else None
            if cur is not None:
                out.append(cur)
            continue
        it = _ITEM.match(ln)
        if it and cur is not None:
            cur[2].append(tuple(int(x) for x in it.groups()))
    return out


def step_plan(V, monkeypatch, capfd, archs, B, dtype, X, eps=None, env=None, **kw):
    """Create a handle with AVAE_DEBUG_SYNC=1 (plus `env`), run one partial_fit on (X, eps) and return the plan of that step
    (see parse).  The switches are read once by avae_create; they are unset again before returning."""
    for k, v in dict(env or {}, AVAE_DEBUG_SYNC="1").items():
        monkeypatch.setenv(k, v)
    try:
        m = V.AssocVariationalAutoEncoder(archs, batch_size=B, compute_dtype=dtype, **kw)
    finally:
        for k in dict(env or {}, AVAE_DEBUG_SYNC="1"):
            monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    m.partial_fit(X, eps)
    m.synchronize()
    text = capfd.readouterr().err
    del m
    plan = parse(text)
    assert plan, "no launch dump under AVAE_DEBUG_SYNC=1:\n" + text[-2000:]
    return plan


def launch(plan, name):
    """the (cfg, items) of the launch called `name` (exactly one)"""
    hits = [(c, it) for n, c, it in plan if n == name]
    assert len(hits) == 1, (name, [n for n, _c, _i in plan])
    return hits[0]


def cfgs(plan):
    return {n: c for n, c, _i in plan}


def tn_shapes(archs, O):
    """(M, N) = (in + 1, out) of every dense layer, as the weight-gradient launches see them"""
    out = []
    for na in archs:
        for name, shp in O.layer_shapes(na):
            if len(shp) == 2:
                out.append((name, int(shp[0]) + 1, int(shp[1])))
    return out


def tiles(M, N, TM, TN):
    return int(np.ceil(M / TM)) * int(np.ceil(N / TN))
