#!/usr/bin/env python3
"""Cost of the motion calls (avae_motion_eval / _fit / _moments) and of predict_motion(), device tensors in
and out: the reference's sigmoid basis (7 joints x 21 parameters, 100 phase points) with scale, shift and limits, N rows in
{256, 4096}, S samples in {0, 16, 64} (S = 0: motion_eval and motion_fit; S >= 1: motion_moments), hipEvent timing after a
warm-up, the median of 7 repeats with the candidates interleaved,

against the same arithmetic written with torch in fp32: ``einsum`` of the features with the un-normalised parameters, ``clamp``,
counts of the clamped points, ``mean`` / ``var`` over the sample axis, in row chunks so that the [rows, S, 100, 7] trajectories fit
(--chunk-floats).  predict_motion() runs on C2 (784-500-500 / 147-200-200, n_z 20, B 256, bf16, relu) with the image present and the
trajectory absent, against impute() / generate() on the surface followed by that torch arithmetic.

One JSON line; --out FILE also writes it there."""
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
from vae_assoc_amd.motion import MotionBasis
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, motion_matrices, motion_fit_args

D, KB, T = 7, 21, 100


def torch_eval(p, m):
    """[..., 147] -> (clamped trajectories [..., 100, 7], clamped mask)"""
    theta = (p * m["scale"] + m["shift"]).unflatten(-1, (D, KB))
    q = torch.einsum("tk,...dk->...td", m["phi"], theta)
    lo, hi = m["limits"][:, 0], m["limits"][:, 1]
    return torch.minimum(torch.maximum(q, lo), hi), (q > hi) | (q < lo)


def torch_moments(s, m, chunk_floats):
    """[N, S, 147] -> (mean, var [N, 100, 7], saturated_frac [N, 7]) in row chunks"""
    N, S = s.shape[:2]
    rows = max(1, chunk_floats // (S * T * D))
    out = []
    for r0 in range(0, N, rows):
        q, hit = torch_eval(s[r0:r0 + rows], m)
        out.append((q.mean(1), q.var(1, unbiased=False), hit.sum((1, 2)) / float(S * T)))
    return tuple(torch.cat(x) for x in zip(*out))


def torch_fit(tr, pinv, m):
    return ((torch.einsum("kt,ntd->ndk", pinv, tr).flatten(1) - m["shift"]) / m["scale"])


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def race(f_lib, f_torch, repeats):
    for f in (f_lib, f_torch, f_lib, f_torch):
        f()
    torch.cuda.synchronize()
    t_l, t_t = [], []
    for _ in range(repeats):                                                               # interleaved
        t_l.append(once(f_lib))
        t_t.append(once(f_torch))
    ms_l, ms_t = float(np.median(t_l)), float(np.median(t_t))
    return {"library_ms": round(ms_l, 4), "torch_ms": round(ms_t, 4), "ratio": round(ms_t / ms_l, 3),
            "library_ms_min_max": [round(min(t_l), 4), round(max(t_l), 4)], "torch_ms_min_max": [round(min(t_t), 4), round(max(t_t), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--samples", type=int, nargs="*", default=[0, 16, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-floats", type=int, default=1 << 26, help="trajectory floats the torch composition holds at a time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    rng = np.random.default_rng(0)
    basis = MotionBasis(param_mean=0.3 * rng.standard_normal(D * KB), param_std=rng.uniform(0.5, 1.5, D * KB),
                        limits=np.c_[-np.ones(D), np.ones(D)])
    m = motion_matrices(basis, model.device)
    line = {"config": label, "basis": "sigmoid 7 x 21, 100 points", "repeats": args.repeats, "cases": {}}
    for N in args.rows:
        img = torch.from_numpy((rng.random((N, 784)) < 0.2).astype(np.float32)).cuda()
        for S in args.samples:
            case = {}
            if S == 0:
                p = torch.randn((N, D * KB), device="cuda")
                case["motion_eval"] = race(lambda: model.motion_eval(p, basis), lambda: torch_eval(p, m), args.repeats)
                tr = model.motion_eval(p, basis)["trajectory"]
                pinv = motion_fit_args(tr, basis, model.device)[1]
                case["motion_fit"] = race(lambda: model.motion_fit(tr, basis), lambda: torch_fit(tr, pinv, m), args.repeats)
                case["max_abs_diff"] = float((tr - torch_eval(p, m)[0]).abs().max())

                def composed():
                    return torch_eval(model.impute([img, None])["mean"][1], m)
                case["predict_motion"] = race(lambda: model.predict_motion([img, None], basis), composed, args.repeats)
            else:
                s = torch.randn((N, S, D * KB), device="cuda")
                case["motion_moments"] = race(lambda: model.motion_moments(s, basis),
                                              lambda: torch_moments(s, m, args.chunk_floats), args.repeats)
                a, b = model.motion_moments(s, basis), torch_moments(s, m, args.chunk_floats)
                case["max_abs_diff"] = float(max((a["mean"] - b[0]).abs().max(), (a["var"] - b[1]).abs().max()))
                case["samples_GB_per_s"] = round(s.numel() * 4 / (case["motion_moments"]["library_ms"] * 1e-3) / 1e9, 1)
                eps = torch.randn((N, S, 20), device="cuda")

                def composed():
                    post = model.impute([img, None])
                    z = post["mu"][:, None, :] + torch.exp(0.5 * post["logvar"])[:, None, :] * eps
                    rows = max(1, args.chunk_floats // (S * T * D))
                    out = []
                    for r0 in range(0, N, rows):
                        dec = model.generate(z[r0:r0 + rows].reshape(-1, 20))[1]
                        out.append(torch_moments(dec.view(-1, S, D * KB), m, args.chunk_floats))
                    return tuple(torch.cat(x) for x in zip(*out))
                case["predict_motion"] = race(lambda: model.predict_motion([img, None], basis, n_samples=S, eps=eps), composed,
                                              args.repeats)
            line["cases"]["N%d_S%d" % (N, S)] = case
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
