"""The training step's launch plan as the library runs it, read from its AVAE_DEBUG_SYNC=1 dump (test-side only).

A handle created with AVAE_DEBUG_SYNC=1 runs eagerly and prints, for every launch, a header
``[avae] launch NAME type=T cfg=C items=N blocks=K`` and one ``item kind= M= N= K= ...`` line per GEMM item of a grouped NT
launch.  Weight-gradient (TN) launches print the header only: their items live in the compact TnItem table, so their list is
empty here and a test takes their shapes (M = in + 1, N = out, K = batch) from the model's layer shapes.

The by-modality decode route and complete() run through the same dump (eager under that switch).  The serve plan cannot: the switch
forces use_graph = 0 and with it the by-modality route.  A handle created with AVAE_PLAN_DUMP=1 runs as any other and prints, when it
builds the serve plan of a row bucket, ``[avae] serve plan bucket=B fused_in=0|1 lean_in=0|1 in_lean_grid=G`` and the same launch and
item lines for the plan's launches, the fused staging launch first (parse_serve, serve_plan).

Tile configurations (the source is the enumeration TileCfg in vae_assoc_amd/csrc/avae_device.h, whose values are pinned for this
text format; avae_host.hip::choose_cfg picks one per launch): 0 = 64x64, 1 = 128x128, 2 = 256x128 8-wave NT/TN, 3 = 32x64,
4 = 64x128 (wide-latent heads), 5 = 32x32, 6 = 256x64 8-wave loss, 7/9/10/11 = the lean small-net kernels, 12 = small-net weight
gradients with Adam in the epilogue.  `type` is LaunchType of the same header (0 = a grouped GEMM launch)."""
import re

import numpy as np

K_FWD_HIDDEN, K_FWD_HEAD, K_FWD_OUT_LOSS, K_DGRAD_HIDDEN, K_DGRAD_LATENT, K_WGRAD, K_LATENT = 0, 1, 2, 4, 5, 6, 7
K_FWD_OUT_STORE, K_DGRAD_F32, K_SERVE_Z = 3, 10, 11

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


_SERVE = re.compile(r"^\[avae\] serve plan bucket=(\d+) fused_in=([01]) lean_in=([01]) in_lean_grid=(\d+)\s*$")


def with_switches(monkeypatch, env, make):
    """make() under the environment `env`: the switches are read once by avae_create and unset again before returning"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return make()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def parse_serve(text):
    """{bucket: dict(fused_in, lean_in, in_lean_grid, plan)} of the serve plans an AVAE_PLAN_DUMP=1 handle printed when it built
    them; `plan` as parse() returns it, the staging launch ("serve_in+serve_dec1", K_SERVE_Z items) first when it is fused"""
    out, cur = {}, None
    for ln in text.splitlines():
        s = _SERVE.match(ln)
        if s:
            b, fused, lean, grid = (int(x) for x in s.groups())
            assert b not in out, "serve plan of bucket %d built twice" % b
            cur = out[b] = dict(fused_in=bool(fused), lean_in=bool(lean), in_lean_grid=grid, lines=[])
        elif cur is not None:
            cur["lines"].append(ln)
    for sv in out.values():
        sv["plan"] = parse("\n".join(sv.pop("lines")))
    return out


def serve_plan(V, monkeypatch, capfd, archs, B, dtype, rows, **kw):
    """The serve plan that generate() of `rows` rows builds on a fresh handle (AVAE_PLAN_DUMP=1; one plan per row bucket the call's
    chunks fall into) -> parse_serve's dict.  The switch changes nothing but the print, so the plan is the one any handle of the
    same model runs."""
    m = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"},
                      lambda: V.AssocVariationalAutoEncoder(archs, batch_size=B, compute_dtype=dtype, **kw))
    capfd.readouterr()
    m.generate(np.zeros((rows, int(archs[0]["n_z"])), np.float32))
    m.synchronize()
    text = capfd.readouterr().err
    del m
    plans = parse_serve(text)
    assert plans, "no serve plan dump under AVAE_PLAN_DUMP=1:\n" + text[-2000:]
    return plans


def slices(sv):
    """columns slices (64 wide) per modality of a fused serve plan's staging launch, from its K_SERVE_Z items"""
    name, _cfg, items = sv["plan"][0]
    assert sv["fused_in"] and name == "serve_in+serve_dec1" and all(k == K_SERVE_Z for k, _M, _N, _K in items), sv["plan"][0]
    return [(N + 63) // 64 for _k, _M, N, _K in items]


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
