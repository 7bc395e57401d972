#!/usr/bin/env python3
"""Cost of impute() (avae_impute: fused-posterior prediction of missing modalities) on C2 (784-500-500 / 147-200-200, n_z 20,
B 256, bf16, relu), device tensors in and out: N rows with the image present and the trajectory absent, n_samples K in {0, 16, 64},
hipEvent timing after a warm-up, the median of 9 repeats with the candidates interleaved,

against the composition a user writes on the surface without it: transform() of the present modality (with one modality present
the fusion is that posterior; the precision-weighted rule in torch otherwise), then per block of samples z = mu + exp(lv/2) eps,
generate(), and torch's running mean / M2 over the block (Chan's merge), so that it too never holds N K n_input floats.  The
composition needs the log-variance, which transform() does not return: it takes it from the same encoder call (_encode).

Also the per-launch breakdown of one impute call from avae_timing_report (timing mode runs eagerly, modality by modality).
One JSON line; --out FILE also writes it there."""
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


def composition(model, img, K, eps, block):
    """transform -> fusion (one present modality: a select) -> generate per block of samples -> running mean / variance"""
    mu, lv = model._encode(0, img, want_logvar=True)
    if K == 0:
        return mu, lv, model.generate(mu), None
    N, nz = mu.shape
    sd = torch.exp(0.5 * lv)
    mean = M2 = None
    for k0 in range(0, K, block):
        kc = min(block, K - k0)
        z = (mu[:, None, :] + sd[:, None, :] * eps[:, k0:k0 + kc, :]).reshape(N * kc, nz)
        xs = [x.view(N, kc, -1) for x in model.generate(z)]
        bm = [x.mean(1) for x in xs]
        b2 = [((x - m[:, None, :]) ** 2).sum(1) for x, m in zip(xs, bm)]
        if mean is None:
            mean, M2 = bm, b2
        else:
            d = [b - a for a, b in zip(mean, bm)]
            tot = k0 + kc
            M2 = [a + b + dd * dd * (k0 * kc / tot) for a, b, dd in zip(M2, b2, d)]
            mean = [a + dd * (kc / tot) for a, dd in zip(mean, d)]
    return mu, lv, mean, [m / K for m in M2]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--samples", type=int, nargs="*", default=[0, 16, 64])
    ap.add_argument("--block", type=int, default=16, help="samples per generate() call of the composition")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    N = args.rows
    img = torch.from_numpy((rng.random((N, 784)) < 0.2).astype(np.float32)).cuda()
    line = {"config": label, "rows": N, "composition_block": args.block, "cases": {}}
    for K in args.samples:
        eps = torch.randn((N, K, 20), device="cuda") if K else None
        f_imp = lambda: model.impute([img, None], n_samples=K, eps=eps)                    # noqa: E731
        f_cmp = lambda: composition(model, img, K, eps, args.block)                        # noqa: E731
        for f in (f_imp, f_cmp, f_imp, f_cmp):
            f()
        torch.cuda.synchronize()
        t_imp, t_cmp = [], []
        for _ in range(args.repeats):                                                      # interleaved
            t_imp.append(once(f_imp))
            t_cmp.append(once(f_cmp))
        a, b = f_imp(), f_cmp()
        err = float((a["mean"][1] - b[2][1]).abs().max())
        ms_i, ms_c = float(np.median(t_imp)), float(np.median(t_cmp))
        line["cases"][str(K)] = {"impute_ms": round(ms_i, 3), "composition_ms": round(ms_c, 3), "ratio": round(ms_c / ms_i, 3),
                                 "impute_ms_min_max": [round(min(t_imp), 3), round(max(t_imp), 3)],
                                 "composition_ms_min_max": [round(min(t_cmp), 3), round(max(t_cmp), 3)],
                                 "decoded_rows_per_s": round(N * max(K, 1) / (ms_i * 1e-3)),
                                 "max_abs_diff_of_the_joint_mean": err}
    # per-launch breakdown of one call at the largest K
    K = max(args.samples)
    L, h = model._L, model._h
    L.avae_timing_enable(h, 1)
    model.impute([img[:4 * B], None], n_samples=K)
    buf = C.create_string_buffer(1 << 16)
    L.avae_timing_report(h, buf, len(buf))
    L.avae_timing_enable(h, 0)
    line["per_launch_K%d_rows%d" % (K, 4 * B)] = {nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2)}
                                                  for nm, c, a, _ in (ln.split() for ln in buf.value.decode().splitlines())}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
