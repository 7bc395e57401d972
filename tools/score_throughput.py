#!/usr/bin/env python3
"""Rows per second of score_samples against the composition a user writes without it: encode both modalities (mu, log sigma^2),
z = mu + exp(lv/2) eps in torch, generate(z_m) for each modality, and the per-row loss terms in torch -- plus, with cross_modal,
generate(mu_s) for every source s and the losses of every target.  C2 nets (784-500-500 / 147-200-200, n_z 20, B 256, bf16),
device tensors in and out; hipEvent timing after a warm-up of every shape.  One JSON line per (N, cross_modal); --out FILE also
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


def recon(x, xh, binary):
    if binary:
        return -(x * torch.log(1e-3 + xh) + (1 - x) * torch.log(1e-3 + 1 - xh)).sum(1)
    return 0.5 * ((x - xh) ** 2).sum(1)


def composed(model, X, eps, cross):
    """score_samples' numbers through the public per-step surface (transform / generate) and torch."""
    binary, w, lam = model.binary, model.weights, model.assoc_lambda
    M = len(X)
    mus, lvs = zip(*[model._encode(m, X[m], want_logvar=True) for m in range(M)])
    rec = [recon(X[m], model.generate(mus[m] + torch.exp(0.5 * lvs[m]) * eps)[m], binary[m]) for m in range(M)]
    lat = [-0.5 * (1 + lv - mu * mu - torch.exp(lv)).sum(1) for mu, lv in zip(mus, lvs)]
    assoc = [0.5 * (torch.exp(lvs[i] - lvs[j]) + torch.exp(lvs[j] - lvs[i]) - 2
                    + (mus[i] - mus[j]) ** 2 * (torch.exp(-lvs[i]) + torch.exp(-lvs[j]))).sum(1)
             for i in range(M) for j in range(i + 1, M)]
    cost = sum(w[m] * (rec[m] + lat[m]) for m in range(M)) + lam * sum(assoc)
    out = {"cost": cost}
    if cross:
        out["cross"] = torch.stack([torch.stack([recon(X[d], xh, binary[d]) for d, xh in enumerate(model.generate(mus[s]))], 1)
                                    for s in range(M)], 1)
    return out


def rate(fn, rows, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / reps
    return rows / (ms * 1e-3), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    lines = []
    for N in args.rows:
        data = torch.from_numpy(np.concatenate([rng.random((N, 784)), rng.standard_normal((N, 147))], 1).astype(np.float32)).cuda()
        X = [data[:, :784].contiguous(), data[:, 784:].contiguous()]
        eps = torch.from_numpy(rng.standard_normal((N, 20)).astype(np.float32)).cuda()
        reps = max(3, 65536 * 4 // N)
        for cross in (False, True):
            s = model.score_samples(X, eps=eps, cross_modal=cross)
            c = composed(model, X, eps, cross)
            diff = {k: float(((s[k] - c[k]).abs().max() / c[k].abs().max()).item()) for k in c}
            r_s, ms_s = rate(lambda: model.score_samples(X, eps=eps, cross_modal=cross), N, reps)
            r_c, ms_c = rate(lambda: composed(model, X, eps, cross), N, reps)
            line = {"config": label, "rows": N, "cross_modal": cross, "score_rows_per_s": round(r_s), "score_ms": round(ms_s, 3),
                    "composed_rows_per_s": round(r_c), "composed_ms": round(ms_c, 3), "speedup": round(r_s / r_c, 3),
                    "max_rel_diff_vs_composed": diff}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
