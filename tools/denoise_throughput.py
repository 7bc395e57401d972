#!/usr/bin/env python3
"""Step time of denoising training against the plain step on the same handle and data: C2 and C4
(bench.py's configurations, relu, bf16); on-device corruption with the drop stream only (30 % of every modality), with the drop
and the noise stream (sigma 0.5), and explicit ``inputs=`` (a second device matrix per modality, read by the staging launch).
Device tensors in; hipEvent timing around partial_fit_steps runs of --steps steps (16-step replays) after a warm-up, then a
synchronise; the median of --repeats runs, the variants interleaved.  One JSON line per (config, variant); --out FILE also
writes them there."""
import argparse
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
        model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=1, **hy)
        rng = np.random.default_rng(0)
        n = args.steps
        X = [torch.as_tensor(x).cuda() for x in bench.synth(rng, B * n)]
        IN = [torch.where(torch.rand_like(x) < 0.3, torch.zeros_like(x), x) for x in X]
        # (corruption set before the timed call, explicit inputs or None): the setting is handle state, outside the timed region
        runs = {"plain": (None, None), "drop": (dict(drop=0.3), None), "drop_noise": (dict(drop=0.3, noise=0.5), None),
                "inputs": (None, IN)}

        def run(corr, inputs):
            model.set_corruption(**corr) if corr else model.set_corruption(None)
            return time_ms(lambda: model.partial_fit_steps(X, n, return_cost=False, inputs=inputs), n)
        for corr, inputs in runs.values():      # warm-up
            run(corr, inputs)
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):           # interleaved: drift of the box lands on every variant alike
            for k, (corr, inputs) in runs.items():
                ms[k].append(run(corr, inputs))
        base = float(np.median(ms["plain"]))
        for k in runs:
            if k == "plain":
                continue
            m = float(np.median(ms[k]))
            rec = dict(config=name, variant=k, batch=B, dtype=dtype, steps=n, plain_ms_per_step=round(base, 5),
                       denoise_ms_per_step=round(m, 5), delta_us=round((m - base) * 1e3, 2),
                       plain_spread_us=round((max(ms["plain"]) - min(ms["plain"])) * 1e3, 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
