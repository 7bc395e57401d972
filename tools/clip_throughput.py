#!/usr/bin/env python3
"""Step time of global-norm gradient clipping (set_grad_clip) against the unclipped step on the same model
and data: C2 and C4 (bench.py's configurations, relu, bf16).  Variants, each a model of its own on the same inputs:

  off          clipping off: the default plan (C2: the fused wgrad+adam launch)
  unfused      clipping off, built under AVAE_NO_ADAM_FUSE=1: wgrad -> adam as two launches, the tail clipping switches to
               (where the default plan has no fused launch -- C4 -- this is the same plan as `off`)
  monitor      max_norm = inf: wgrad -> grad_sumsq -> adam, c = 1
  clip         max_norm = half the first step's norm

Device tensors in; hipEvent timing around partial_fit_steps runs of --steps steps (16-step replays) after a warm-up, then a
synchronise; the median of --repeats runs, the variants interleaved.  Reported per configuration: ms per step of every variant,
the norm launch's own cost (clip - unfused), the price of leaving the fused launch (unfused - off), and grad_sumsq's line from
avae_timing_report (eager launches) set against the bytes it reads.  Run from a checkout of another commit with --variants
off,unfused to measure that commit's step.  One JSON line per configuration; --out FILE also writes them there."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as g
g.build()
import bench
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder


def time_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def build(archs, B, dtype, hy, unfused=False):
    old = os.environ.get("AVAE_NO_ADAM_FUSE")
    if unfused:
        os.environ["AVAE_NO_ADAM_FUSE"] = "1"       # read while the handle plans its step
    try:
        return AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=1, **hy)
    finally:
        if unfused:
            if old is None:
                del os.environ["AVAE_NO_ADAM_FUSE"]
            else:
                os.environ["AVAE_NO_ADAM_FUSE"] = old


def launch_report(model, fn):
    L, h = model._L, model._h
    L.avae_timing_enable(h, 1)
    fn()
    buf = C.create_string_buffer(1 << 16)
    L.avae_timing_report(h, buf, len(buf))
    L.avae_timing_enable(h, 0)
    return {nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2), "min_us": round(float(mn) * 1e3, 2)}
            for nm, c, a, mn in (ln.split() for ln in buf.value.decode().splitlines())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4")
    ap.add_argument("--variants", default="off,unfused,monitor,clip")
    ap.add_argument("--steps", type=int, default=64, help="steps per timed run (a multiple of 16: whole replays)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    variants = args.variants.split(",")
    lines = []
    for name in args.configs.split(","):
        archs, B, dtype, label = bench.CONFIGS[name]
        hy = bench.hyper_for(archs)
        rng = np.random.default_rng(0)
        n = args.steps
        X = [torch.as_tensor(x).cuda() for x in bench.synth(rng, B * n)]
        models = {v: build(archs, B, dtype, hy, unfused=(v == "unfused")) for v in variants}
        rec = dict(config=name, batch=B, dtype=dtype, steps=n, repeats=args.repeats)
        if "monitor" in models:
            models["monitor"].set_grad_clip(max_norm=float("inf"))
        if "clip" in models:
            probe = models["clip"]
            p0 = probe.get_params()
            probe.set_grad_clip(max_norm=float("inf"))
            probe.partial_fit([x[:B] for x in X], return_cost=False)
            n0 = float(probe.grad_norm_history(1)[0][0])
            probe.set_params(p0)
            probe.set_grad_clip(max_norm=0.5 * n0)
            rec["first_norm"] = n0
        runs = {v: (lambda m: lambda: m.partial_fit_steps(X, n, return_cost=False))(m) for v, m in models.items()}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):       # interleaved: drift of the box lands on every variant alike
            for k, fn in runs.items():
                ms[k].append(time_ms(fn, n))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rec["ms_per_step"] = {k: round(v, 5) for k, v in med.items()}
        rec["ms_min_max"] = {k: [round(min(v), 5), round(max(v), 5)] for k, v in ms.items()}
        if "clip" in med and "unfused" in med:
            rec["norm_launch_us"] = round((med["clip"] - med["unfused"]) * 1e3, 2)
        if "unfused" in med and "off" in med:
            rec["leaving_fused_launch_us"] = round((med["unfused"] - med["off"]) * 1e3, 2)
        if "clip" in models:
            m = models["clip"]
            X16 = [x[:16 * B] for x in X]
            rep = launch_report(m, lambda: m.partial_fit_steps(X16, 16, return_cost=False))
            p_int = m._grad_tensor().numel() - 1
            rec["grad_bytes"] = 4 * p_int
            rec["launches_us"] = {k: rep[k] for k in rep if k in ("grad_sumsq", "adam", "wgrad", "_null_kernel") or k.startswith("wgrad")}
            if "grad_sumsq" in rep and rep["grad_sumsq"]["avg_us"] > 0:
                rec["grad_sumsq_GBps"] = round(4 * p_int / (rep["grad_sumsq"]["avg_us"] * 1e-6) / 1e9, 1)
            norms, last, skipped = m.grad_norm_history(16)
            rec["clipped_of_last_16"] = int(np.sum(norms > np.float32(0.5 * rec["first_norm"])))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del models, runs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
