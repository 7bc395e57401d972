#!/usr/bin/env python3
"""Rows per second of score_samples_masked / log_likelihood_masked next to their unmasked twins on the same handle.  C2 nets
(784-500-500 / 147-200-200, n_z 20, B 256, bf16), N = 4096 rows, device tensors in and out, three masks: all present, 50 %
image-only (every other row lacks the joint modality) and joint-absent (X[1] = None).  Timed with device events after a warm-up
of every shape; the variants of one measurement are interleaved (unmasked, all, half, none, unmasked, ...) and each reports the
median of its repeats, so that drift of the machine hits all of them alike.

Every measurement (score without / with cross terms, log-likelihood at each K) runs in a child process of its own under
`timeout -k 10 <s>`; a child that fails or times out ends the run.  One JSON line per measurement; --out FILE also writes them."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interleaved_medians(fns, inner, repeats):
    """{name: median ms per call} over ``repeats`` rounds; a round times ``inner`` calls of every variant, one after the other"""
    for fn in fns.values():                      # warm-up of every shape (plans, graphs, the presence buffer)
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: (float(min(v)), float(max(v))) for k, v in ms.items()}


def one(what, N, repeats):
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    data = torch.from_numpy(np.concatenate([rng.random((N, 784)), rng.standard_normal((N, 147))], 1).astype(np.float32)).cuda()
    X = [data[:, :784].contiguous(), data[:, 784:].contiguous()]
    ones = torch.ones((N, 2), dtype=torch.uint8, device="cuda")
    half = ones.clone()
    half[1::2, 1] = 0
    if what.startswith("score"):
        cross = what == "score_cross"
        eps = torch.from_numpy(rng.standard_normal((N, 20)).astype(np.float32)).cuda()
        fns = {"unmasked": lambda: model.score_samples(X, eps=eps, cross_modal=cross),
               "all_present": lambda: model.score_samples_masked(X, ones, eps=eps, cross_modal=cross),
               "half_image_only": lambda: model.score_samples_masked(X, half, eps=eps, cross_modal=cross),
               "joint_absent": lambda: model.score_samples_masked([X[0], None], ones, eps=eps, cross_modal=cross)}
        inner, K = 8, None
    else:
        K = int(what[len("loglik_k"):])
        eps = torch.from_numpy(rng.standard_normal((N, K, 20)).astype(np.float32)).cuda()
        fns = {"unmasked": lambda: model.log_likelihood(X, n_samples=K, eps=eps),
               "all_present": lambda: model.log_likelihood_masked(X, ones, n_samples=K, eps=eps),
               "half_image_only": lambda: model.log_likelihood_masked(X, half, n_samples=K, eps=eps),
               "joint_absent": lambda: model.log_likelihood_masked([X[0], None], ones, n_samples=K, eps=eps)}
        inner = max(1, 16 // K)
    med, span = interleaved_medians(fns, inner, repeats)
    line = {"config": label, "what": what, "rows": N, "repeats": repeats}
    if K is not None:
        line["n_samples"] = K
    for k in fns:
        line[k + "_rows_per_s"] = round(N / (med[k] * 1e-3))
        line[k + "_ms"] = round(med[k], 3)
        line[k + "_ms_min_max"] = [round(span[k][0], 3), round(span[k][1], 3)]
        if k != "unmasked":
            line[k + "_vs_unmasked"] = round(med[k] / med["unmasked"], 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 128, 1024])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement (the child's build, warm-up and timing)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        print(json.dumps(one(args.one, args.rows, args.repeats)), flush=True)
        return 0
    lines = []
    for what in ["score", "score_cross"] + ["loglik_k%d" % k for k in args.samples]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", what,
               "--rows", str(args.rows), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stdout.write(p.stdout)
            print("masked_scoring_throughput: %s failed with exit status %d; stopping" % (what, p.returncode), file=sys.stderr)
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
