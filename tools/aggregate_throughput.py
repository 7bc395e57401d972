#!/usr/bin/env python3
"""Cost of aggregate_log_density() (avae_agg_logpdf: the streamed log-sum-exp over a gallery of posteriors) against the composition
a user writes in torch on the same device, device tensors in and out: N queries in {256, 4096} against a gallery of G = 65,536
posteriors, n_z in {20, 64}, with and without the per-dimension marginals.  Latents are random (mu ~ N(0, 1), lv ~ U(-6, 1)),
queries half samples of gallery rows' posteriors and half draws from N(0, 9); the call only sees latents, so the model is a small
one.

The composition, in fp32: iv = exp(-lv) once, then per chunk of queries the [c, G, n_z] broadcast of the exponents
l = -0.5 (lv + (z - mu)^2 iv), torch.logsumexp over the gallery of l (marginals) and of l.sum(-1) (joint); c is the largest chunk
whose broadcast stays within --chunk-bytes (1 GiB).

hipEvent timing after a warm-up of both candidates, the median of --repeats calls with the candidates interleaved, the spread of
each (min, max) beside it.  Reported per case: milliseconds, N * G * (n_z + 1) exponent terms per second of the fused call
(N * G without marginals ... the terms it skips are counted all the same, so the two rows compare), the ratio composition /
fused, the worst difference of the two results, and the per-launch device times of one call from avae_timing_report.  No ratio
is a condition.  One JSON line; --out FILE also writes it there."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as g
g.build()
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def arch(scope, n_in, h, n_z):
    return dict(scope=scope, hidden_conv=False, n_hidden_recog_1=h, n_hidden_recog_2=h, n_hidden_gener_1=h, n_hidden_gener_2=h,
                n_input=n_in, n_z=n_z)


def compose(z, gal, marginals, chunk_bytes):
    gm, gl = gal
    G, nz = gm.shape
    iv = torch.exp(-gl)
    c = max(1, int(chunk_bytes // (G * nz * 4)))
    joint, marg = [], []
    for r0 in range(0, z.shape[0], c):
        d = z[r0:r0 + c, None, :] - gm[None]
        l = -0.5 * (gl[None] + d * d * iv[None])
        joint.append(torch.logsumexp(l.sum(-1), dim=1) - (math.log(G) + nz * HALF_LOG_2PI))
        if marginals:
            marg.append(torch.logsumexp(l, dim=1) - (math.log(G) + HALF_LOG_2PI))
    return torch.cat(joint), (torch.cat(marg) if marginals else None)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--gallery", type=int, default=65536)
    ap.add_argument("--nz", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G = args.gallery
    line = {"gallery": G, "repeats": args.repeats, "composition_chunk_bytes": args.chunk_bytes, "cases": []}
    for nz in args.nz:
        model = AssocVariationalAutoEncoder([arch("image", 784, 64, nz), arch("joint", 147, 64, nz)], binary=[True, False],
                                            transfer_fct="relu", batch_size=16, compute_dtype="fp32", seed=0)
        gen = torch.Generator(device="cuda").manual_seed(nz)
        gal = (torch.randn((G, nz), device="cuda", generator=gen), torch.rand((G, nz), device="cuda", generator=gen) * 7.0 - 6.0)
        for N in args.rows:
            own = torch.randint(0, G, (N // 2,), device="cuda", generator=gen)
            z = torch.cat([gal[0][own] + torch.exp(0.5 * gal[1][own]) * torch.randn((N // 2, nz), device="cuda", generator=gen),
                           3.0 * torch.randn((N - N // 2, nz), device="cuda", generator=gen)])
            for marginals in (True, False):
                f_lib = lambda: model.aggregate_log_density(z, gal, marginals=marginals)         # noqa: E731
                f_cmp = lambda: compose(z, gal, marginals, args.chunk_bytes)                       # noqa: E731
                for f in (f_lib, f_cmp, f_lib, f_cmp):
                    f()
                torch.cuda.synchronize()
                t_lib, t_cmp = [], []
                for _ in range(args.repeats):                                                      # interleaved
                    t_lib.append(once(f_lib))
                    t_cmp.append(once(f_cmp))
                a, b = f_lib(), f_cmp()
                diff = float((a["joint"].double() - b[0].double()).abs().div(b[0].double().abs() + nz).max().item())
                if marginals:
                    diff = max(diff, float((a["marginal"].double() - b[1].double()).abs().div(b[1].double().abs() + 1).max().item()))
                ms_l, ms_c = float(np.median(t_lib)), float(np.median(t_cmp))
                line["cases"].append({
                    "n_z": nz, "rows": N, "marginals": marginals, "aggregate_log_density_ms": round(ms_l, 4),
                    "composition_ms": round(ms_c, 4), "ratio": round(ms_c / ms_l, 2),
                    "aggregate_log_density_ms_min_max": [round(min(t_lib), 4), round(max(t_lib), 4)],
                    "composition_ms_min_max": [round(min(t_cmp), 4), round(max(t_cmp), 4)],
                    "exponent_terms_per_s": round(N * G * (nz + 1) / (ms_l * 1e-3)),
                    "worst_relative_difference": diff})
        # per-launch device times of one call at the largest N (timing mode records every launch with its own events)
        L, h = model._L, model._h
        for marginals in (True, False):
            L.avae_timing_enable(h, 1)
            model.aggregate_log_density(z, gal, marginals=marginals)
            buf = C.create_string_buffer(1 << 16)
            L.avae_timing_report(h, buf, len(buf))
            L.avae_timing_enable(h, 0)
            line["per_launch_nz%d_rows%d_%s" % (nz, z.shape[0], "marginals" if marginals else "joint")] = {
                nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2)}
                for nm, c, a, _ in (ln.split() for ln in buf.value.decode().splitlines()) if nm.startswith("agg_logpdf")}
        del model
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
