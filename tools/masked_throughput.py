#!/usr/bin/env python3
"""Step time of partially paired training (partial_fit_steps(..., present=P)) against the unmasked step on
the same model and data: C2 and C4 (bench.py's configurations, relu, bf16), mask patterns all-present, 50 % image-only rows
(joint absent) and the joint modality absent on every row.  Device tensors in; hipEvent timing around partial_fit_steps runs of
--steps steps (16-step replays) after a warm-up, then a synchronise; the median of --repeats runs, the variants interleaved.  One JSON line per
(config, pattern); --out FILE also writes them there."""
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
        M = len(archs)
        pats = {"all_present": np.ones((B * n, M), bool)}
        half = np.ones((B * n, M), bool)
        half[rng.random(B * n) < 0.5, 1] = False
        pats["half_image_only"] = half
        absent = np.ones((B * n, M), bool)
        absent[:, 1] = False
        pats["joint_absent"] = absent
        runs = {"unmasked": lambda: model.partial_fit_steps(X, n, return_cost=False)}
        for pname, P in pats.items():
            Pd = torch.as_tensor(P).cuda()
            runs[pname] = (lambda Pd: lambda: model.partial_fit_steps(X, n, return_cost=False, present=Pd))(Pd)
        for fn in runs.values():            # warm-up (the first masked call builds the masked twin)
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):       # interleaved: drift of the box lands on every variant alike
            for k, fn in runs.items():
                ms[k].append(time_ms(fn, n))
        base = float(np.median(ms["unmasked"]))
        for pname in pats:
            m = float(np.median(ms[pname]))
            rec = dict(config=name, pattern=pname, batch=B, dtype=dtype, steps=n, unmasked_ms_per_step=round(base, 5),
                       masked_ms_per_step=round(m, 5), delta_us=round((m - base) * 1e3, 2))
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
