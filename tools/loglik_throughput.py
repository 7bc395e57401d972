#!/usr/bin/env python3
"""Decoded latent samples per second of log_likelihood (avae_loglik) against the composition a user writes without it: encode
every modality (mu, log sigma^2), z = mu + exp(lv/2) eps in torch, generate(z) for every proposal in chunks that fit, the per-row
reconstruction terms and the log-sum-exp in torch.  C2 nets (784-500-500 / 147-200-200, n_z 20, B 256, bf16), device tensors,
N = 4096 rows, K in {1, 16, 128, 1024}; one decoded z = one latent sample of one proposal, decoded by every modality (N K M per
call).  hipEvent timing after a warm-up call of each path.

Every K runs in a child process of its own under `timeout -k 10 <s>`; a child that fails or times out ends the run.  One JSON
line per K; --out FILE also writes them there."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recon(x, xh, binary):
    if binary:
        return -(x * torch.log(1e-3 + xh) + (1 - x) * torch.log(1e-3 + 1 - xh)).sum(1)
    return 0.5 * ((x - xh) ** 2).sum(1)


def composed(model, X, K, eps, chunk_z=65536):
    """log_likelihood's numbers through the public per-step surface (transform / generate) and torch."""
    M, N = len(X), X[0].shape[0]
    binary = model.binary
    n = max(1, chunk_z // K)                      # input rows per chunk: n K decoded rows of every modality in memory at once
    marg, joint, cond = (torch.empty(shape, device=X[0].device) for shape in ((N, M), (N, M), (N, M, M)))
    mls = [model._encode(m, X[m], want_logvar=True) for m in range(M)]
    for s in range(M):
        mu, lv = mls[s]
        for r0 in range(0, N, n):
            r1 = min(N, r0 + n)
            e = eps[r0:r1]                                                        # [n, K, n_z]
            z = mu[r0:r1, None, :] + torch.exp(0.5 * lv[r0:r1, None, :]) * e
            r = (-0.5 * z * z + 0.5 * e * e + 0.5 * lv[r0:r1, None, :]).sum(2)   # [n, K]
            xh = model.generate(z.reshape(-1, z.shape[2]))
            ell = torch.stack([-recon(X[d][r0:r1].repeat_interleave(K, 0), xh[d], binary[d]).view(r1 - r0, K) for d in range(M)], 2)
            marg[r0:r1, s] = torch.logsumexp(ell[:, :, s] + r, 1) - math.log(K)
            joint[r0:r1, s] = torch.logsumexp(ell.sum(2) + r, 1) - math.log(K)
            cond[r0:r1, s] = torch.logsumexp(ell, 1) - math.log(K)
    return {"marginal": marg, "joint": joint, "conditional": cond}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def one(K, N):
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    data = torch.from_numpy(np.concatenate([rng.random((N, 784)), rng.standard_normal((N, 147))], 1).astype(np.float32)).cuda()
    X = [data[:, :784].contiguous(), data[:, 784:].contiguous()]
    eps = torch.from_numpy(rng.standard_normal((N, K, 20)).astype(np.float32)).cuda()
    M = len(X)
    f = model.log_likelihood(X, n_samples=K, eps=eps)
    c = composed(model, X, K, eps)
    diff = {k: float(((f[k] - c[k]).abs().max() / c[k].abs().max()).item()) for k in c}
    reps = max(1, 256 // K)
    ms_f = timed(lambda: model.log_likelihood(X, n_samples=K, eps=eps), reps)
    ms_c = timed(lambda: composed(model, X, K, eps), reps)
    nz = N * K * M
    return {"config": label, "rows": N, "n_samples": K, "decoded_z": nz,
            "loglik_z_per_s": round(nz / (ms_f * 1e-3)), "loglik_ms": round(ms_f, 2),
            "composed_z_per_s": round(nz / (ms_c * 1e-3)), "composed_ms": round(ms_c, 2),
            "speedup": round(ms_c / ms_f, 3), "max_rel_diff_vs_composed": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 128, 1024])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per K (the child's build, warm-up and timing)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        print(json.dumps(one(args.one, args.rows)), flush=True)
        return 0
    lines = []
    for K in args.samples:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(K), "--rows", str(args.rows)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stdout.write(p.stdout)
            print("loglik_throughput: K=%d failed with exit status %d; stopping" % (K, p.returncode), file=sys.stderr)
            return p.returncode
        line = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    if "--one" in sys.argv:
        sys.path.insert(0, ROOT)
        import numpy as np
        import torch
        import __graft_entry__ as g
        g.build()
        import bench
        from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    sys.exit(main())
