#!/usr/bin/env python3
"""Step time of parameter averaging (set_ema) against the step without it, on ONE model and the same data:
C2 and C4 (bench.py's configurations, relu, bf16).  Measured per configuration:

  off / ema              averaging off, then on (decay 0.999): C2 leaves the fused wgrad+adam launch for wgrad -> adam
  clip / clip+ema        the same with set_grad_clip(max_norm=inf) (wgrad -> grad_sumsq -> adam, c = 1) also on, where the fused
                         launch is already gone: what the average's 8 bytes per parameter cost inside k_adam
  switch                 one use_averaged(True) / use_averaged(False): host wall time of the call (it synchronises the device
                         around its one launch) and the launch's own line from avae_timing_report

Device tensors in; hipEvent timing around partial_fit_steps runs of --steps steps (16-step replays) after a warm-up, then a
synchronise; the median of --repeats runs, the four settings interleaved by switching them on the one handle between runs (a
switch re-captures the step graphs and restarts the average, outside the timed region).  One JSON line per configuration;
--out FILE also writes them there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as g
g.build()
import bench
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder

DECAY = 0.999
SETTINGS = {"off": (False, False), "ema": (False, True), "clip": (True, False), "clip+ema": (True, True)}


def time_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


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
    ap.add_argument("--steps", type=int, default=64, help="steps per timed run (a multiple of 16: whole replays)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(","):
        archs, B, dtype, label = bench.CONFIGS[name]
        hy = bench.hyper_for(archs)
        rng = np.random.default_rng(0)
        n = args.steps
        X = [torch.as_tensor(x).cuda() for x in bench.synth(rng, B * n)]
        model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=1, **hy)
        rec = dict(config=name, batch=B, dtype=dtype, steps=n, repeats=args.repeats, decay=DECAY, params=model.n_params)

        def setting(clip, ema):
            model.set_grad_clip(max_norm=float("inf") if clip else 0.0)
            model.set_ema(DECAY if ema else None)

        def run():
            model.partial_fit_steps(X, n, return_cost=False)

        for clip, ema in SETTINGS.values():     # warm-up of every plan
            setting(clip, ema)
            run()
        torch.cuda.synchronize()
        ms = {k: [] for k in SETTINGS}
        for _ in range(args.repeats):           # interleaved: drift of the box lands on every setting alike
            for k, (clip, ema) in SETTINGS.items():
                setting(clip, ema)
                run()                            # (the fresh graphs' first replay stays out of the figure)
                torch.cuda.synchronize()
                ms[k].append(time_ms(run, n))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rec["ms_per_step"] = {k: round(v, 5) for k, v in med.items()}
        rec["ms_min_max"] = {k: [round(min(v), 5), round(max(v), 5)] for k, v in ms.items()}
        rec["ema_minus_off_us"] = round((med["ema"] - med["off"]) * 1e3, 2)
        rec["clip_ema_minus_clip_us"] = round((med["clip+ema"] - med["clip"]) * 1e3, 2)
        rec["clip_minus_off_us"] = round((med["clip"] - med["off"]) * 1e3, 2)
        # the launches of the averaging step, and the switch
        setting(False, True)
        X16 = [x[:16 * B] for x in X]
        rep = launch_report(model, lambda: model.partial_fit_steps(X16, 16, return_cost=False))
        rec["launches_us"] = {k: rep[k] for k in rep if k in ("adam", "_null_kernel") or k.startswith("wgrad")}
        p_int = model._grad_tensor().numel() - 1
        rec["adam_bytes_per_step"] = {"off": 32 * p_int, "ema": 40 * p_int}
        wall = []
        for _ in range(args.repeats):
            for on in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.use_averaged(on)
                wall.append((time.perf_counter() - t0) * 1e6)
        rec["switch_wall_us"] = round(float(np.median(wall)), 1)
        rep = launch_report(model, lambda: (model.use_averaged(True), model.use_averaged(False)))
        rec["switch_launch_us"] = rep.get("shadow_refresh")
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
