#!/usr/bin/env python3
"""Cost of complete() (avae_complete: gradient latent refinement on the device) on C2 (784-500-500 / 147-200-200, n_z 20, B 256,
bf16, relu), device tensors in and out, hipEvent timing after a warm-up of every shape:

  * microseconds per iteration of one 256-row chunk (the slope between two iteration counts: staging and graph tails cancel);
  * rows x iterations per second for N rows and n_iters iterations;

against (a) the host-driven loop a user writes without it -- per iteration one generate() call on 10 perturbed candidates per row
(the reference's rollouts, baxter_vae_assoc_writer.py:259-304) plus the torch arithmetic of a CEM-style evaluation of J on the
observed elements and the move to the best candidate -- with the same iteration count, and (b) one C2 training step of the same
build (partial_fit_steps).  The image's lower half is missing, the trajectory is unobserved.  One JSON line; --out FILE also
writes it there."""
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

ROLLOUTS = 10


def host_loop(model, img, obs, z0, n_iters, sigma=0.1, prior_weight=1.0):
    """CEM-style search through the public surface: 10 candidates per row around z, J on the observed elements, keep the best."""
    N, nz = z0.shape
    w = model.weights[0]
    z = z0.clone()
    x, o = img.repeat_interleave(ROLLOUTS, 0), obs.repeat_interleave(ROLLOUTS, 0)
    gen = torch.Generator(device=z.device).manual_seed(0)
    for _ in range(n_iters):
        cand = z.repeat_interleave(ROLLOUTS, 0) + sigma * torch.randn((N * ROLLOUTS, nz), device=z.device, generator=gen)
        p = model.generate(cand)[0]
        t = -(x * torch.log(1e-3 + p) + (1 - x) * torch.log(1e-3 + 1 - p))
        J = w * torch.where(o, t, torch.zeros_like(t)).sum(1) + prior_weight * 0.5 * (cand * cand).sum(1)
        best = J.view(N, ROLLOUTS).argmin(1)
        z = cand.view(N, ROLLOUTS, nz)[torch.arange(N, device=z.device), best]
    return z


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    N, T = args.rows, args.iters
    img = torch.from_numpy((rng.random((N, 784)) < 0.2).astype(np.float32)).cuda()
    jnt = torch.from_numpy(rng.standard_normal((N, 147)).astype(np.float32)).cuda()
    obs = torch.zeros((N, 784), dtype=torch.bool, device="cuda")
    obs[:, :392] = True
    z0 = model.transform(torch.where(obs, img, torch.zeros_like(img)), 0)

    chunk = lambda k: model.complete([img[:B], None], [obs[:B], None], n_iters=k, z0=z0[:B])      # noqa: E731
    t_lo, t_hi = timed(lambda: chunk(T), 10), timed(lambda: chunk(5 * T), 10)
    us_iter = (t_hi - t_lo) / (4 * T) * 1e3
    ms_all = timed(lambda: model.complete([img, None], [obs, None], n_iters=T, z0=z0), 5)
    ms_host = timed(lambda: host_loop(model, img, obs, z0, T), 3)
    steps = 64
    X = [img[:B].repeat(steps, 1), jnt[:B].repeat(steps, 1)]
    ms_step = timed(lambda: model.partial_fit_steps(X, steps, return_cost=False), 10) / steps
    r = model.complete([img, None], [obs, None], n_iters=T, z0=z0)
    line = {"config": label, "rows": N, "n_iters": T,
            "complete_us_per_iter_256_rows": round(us_iter, 2), "complete_chunk_ms": {str(T): round(t_lo, 3), str(5 * T): round(t_hi, 3)},
            "complete_ms": round(ms_all, 3), "complete_row_iters_per_s": round(N * T / (ms_all * 1e-3)),
            "host_loop_ms": round(ms_host, 3), "host_loop_row_iters_per_s": round(N * T / (ms_host * 1e-3)),
            "host_loop_us_per_iter_256_rows": round(ms_host * 1e3 / T / (N / B), 2),
            "speedup_vs_host_loop": round(ms_host / ms_all, 2),
            "train_step_ms": round(ms_step, 4), "iter_over_train_step": round(us_iter * 1e-3 / ms_step, 3),
            "objective_first_last_mean": [float(r["objective"][0].mean()), float(r["objective"][-1].mean())]}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
