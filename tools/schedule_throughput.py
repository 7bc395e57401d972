#!/usr/bin/env python3
"""Step time of the on-device training schedules (set_schedule) against the unscheduled step on the same
model and data: C2 and C4 (bench.py's configurations, relu, bf16).  Variants, each a model of its own on the same inputs:

  off          nothing set: the default plan
  const        constant schedules kl = assoc = lr = 1 (the scheduled kernels' instances, multipliers of one)
  kl_assoc     piecewise KL warm-up + cyclical association ramp
  all          those two + an exponential learning-rate decay (pow in the staging launch)

Device tensors in; hipEvent timing around partial_fit_steps runs of --steps steps (16-step replays) after a warm-up, then a
synchronise; the median and the spread (min, max) of --repeats runs, the variants interleaved.  --tree DIR measures the library of
another checkout (its built vae_assoc_amd) -- with --variants off: the parent commit's step in the same session.  One JSON line
per configuration; --out FILE also writes them there."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_ms(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4")
    ap.add_argument("--variants", default="off,const,kl_assoc,all")
    ap.add_argument("--steps", type=int, default=64, help="steps per timed run (a multiple of 16: whole replays)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--tree", default=HERE, help="checkout whose library is measured (default: this one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.tree)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import bench
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder

    variants = args.variants.split(",")
    n = args.steps
    schedules = {
        "off": None,
        "const": dict(kl=1.0, assoc=1.0, lr=1.0),
        "kl_assoc": dict(kl=dict(knots=[(0, 0.0), (10 * n, 1.0)]), assoc=dict(knots=[(0, 0.0), (n // 2, 1.0)], period=n)),
        "all": dict(kl=dict(knots=[(0, 0.0), (10 * n, 1.0)]), assoc=dict(knots=[(0, 0.0), (n // 2, 1.0)], period=n),
                    lr=dict(decay_rate=0.96, decay_steps=100, staircase=False)),
    }
    lines = []
    for name in args.configs.split(","):
        archs, B, dtype, label = bench.CONFIGS[name]
        hy = bench.hyper_for(archs)
        rng = np.random.default_rng(0)
        X = [torch.as_tensor(x).cuda() for x in bench.synth(rng, B * n)]
        models = {}
        for v in variants:
            models[v] = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=1, **hy)
            if schedules[v] is not None:
                models[v].set_schedule(**schedules[v])
        rec = dict(config=name, batch=B, dtype=dtype, steps=n, repeats=args.repeats, tree=root)
        runs = {v: (lambda m: lambda: m.partial_fit_steps(X, n, return_cost=False))(m) for v, m in models.items()}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):       # interleaved: drift of the box lands on every variant alike
            for k, fn in runs.items():
                ms[k].append(time_ms(torch, fn, n))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rec["ms_per_step"] = {k: round(v, 5) for k, v in med.items()}
        rec["ms_min_max"] = {k: [round(min(v), 5), round(max(v), 5)] for k, v in ms.items()}
        if "off" in med:
            rec["over_off_us"] = {k: round((v - med["off"]) * 1e3, 2) for k, v in med.items() if k != "off"}
        for v, m in models.items():
            if schedules[v] is not None:
                h, last = m.hyper_history(1)
                rec.setdefault("last_hyper", {})[v] = [float(x) for x in h[0]] + [int(last)]
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
