#!/usr/bin/env python3
"""Cost of latent_topk() (avae_latent_topk: fused latent distance + top-k) against the composition a user writes in torch on the
same device, device tensors in and out: N queries in {1, 256, 4096} against a gallery of G = 65,536 posteriors, n_z in {20, 64},
k = 10, both metrics.  Latents are random (mu ~ N(0, 1), lv ~ U(-6, 1)); the call only sees latents, so the model is a small one.

The composition:
  l2     torch.cdist(q_mu, g_mu) -> topk(k, largest=False): one [N, G] matrix;
  symkl  per chunk of queries the [c, G, n_z] broadcast of the definition (v = exp(lv), iv = exp(-lv) formed once per side),
         summed over n_z, -> topk; c is the largest chunk whose broadcast stays within --chunk-bytes (1 GiB).

hipEvent timing after a warm-up of both candidates, the median of --repeats calls with the candidates interleaved, the spread of
each (min, max) beside it.  The performance condition of DESIGN.md section 18 is on symkl at N = 4096: the call is not slower
than the composition beyond the run-to-run spread of the two; l2 and N = 1 are reported.  Also reported: the share of rows whose
indices agree with the composition's (near-ties may differ: the composition's arithmetic is another), the pairs per second and
the per-launch device times of one call from avae_timing_report.  One JSON line; --out FILE also writes it there."""
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
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder


def arch(scope, n_in, h, n_z):
    return dict(scope=scope, hidden_conv=False, n_hidden_recog_1=h, n_hidden_recog_2=h, n_hidden_gener_1=h, n_hidden_gener_2=h,
                n_input=n_in, n_z=n_z)


def compose_l2(q, gal, k):
    d, i = torch.cdist(q[0], gal[0]).topk(k, dim=1, largest=False)
    return i, d * d


def compose_symkl(q, gal, k, chunk_bytes):
    (qm, ql), (gm, gl) = q, gal
    G, nz = gm.shape
    gv, gi = torch.exp(gl), torch.exp(-gl)
    c = max(1, int(chunk_bytes // (G * nz * 4)))
    idx, dist = [], []
    for r0 in range(0, qm.shape[0], c):
        m, lv = qm[r0:r0 + c, None, :], ql[r0:r0 + c, None, :]
        iq = torch.exp(-lv)
        t = torch.exp(lv) - gv[None]
        d = m - gm[None]
        D = 0.5 * ((t * iq) * (t * gi[None]) + (d * d) * (iq + gi[None])).sum(-1)
        dd, ii = D.topk(k, dim=1, largest=False)
        idx.append(ii)
        dist.append(dd)
    return torch.cat(idx), torch.cat(dist)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 256, 4096])
    ap.add_argument("--gallery", type=int, default=65536)
    ap.add_argument("--nz", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metrics", nargs="*", default=["symkl", "l2"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G, k = args.gallery, args.k
    line = {"gallery": G, "k": k, "repeats": args.repeats, "composition_chunk_bytes": args.chunk_bytes, "cases": []}
    for nz in args.nz:
        model = AssocVariationalAutoEncoder([arch("image", 784, 64, nz), arch("joint", 147, 64, nz)], binary=[True, False],
                                            transfer_fct="relu", batch_size=16, compute_dtype="fp32", seed=0)
        gen = torch.Generator(device="cuda").manual_seed(nz)
        lat = lambda n: (torch.randn((n, nz), device="cuda", generator=gen),                   # noqa: E731
                         torch.rand((n, nz), device="cuda", generator=gen) * 7.0 - 6.0)
        gal = lat(G)
        for N in args.rows:
            q = lat(N)
            for metric in args.metrics:
                f_lib = lambda: model.latent_topk(q, gal, k=k, metric=metric)                  # noqa: E731
                f_cmp = (lambda: compose_l2(q, gal, k)) if metric == "l2" else (lambda: compose_symkl(q, gal, k, args.chunk_bytes))
                for f in (f_lib, f_cmp, f_lib, f_cmp):
                    f()
                torch.cuda.synchronize()
                t_lib, t_cmp = [], []
                for _ in range(args.repeats):                                                  # interleaved
                    t_lib.append(once(f_lib))
                    t_cmp.append(once(f_cmp))
                a, b = f_lib(), f_cmp()
                same = float((a["index"].long() == b[0]).all(dim=1).double().mean().item())
                ms_l, ms_c = float(np.median(t_lib)), float(np.median(t_cmp))
                spread = (max(t_lib) - min(t_lib)) + (max(t_cmp) - min(t_cmp))
                line["cases"].append({
                    "n_z": nz, "rows": N, "metric": metric, "latent_topk_ms": round(ms_l, 4), "composition_ms": round(ms_c, 4),
                    "ratio": round(ms_c / ms_l, 2), "latent_topk_ms_min_max": [round(min(t_lib), 4), round(max(t_lib), 4)],
                    "composition_ms_min_max": [round(min(t_cmp), 4), round(max(t_cmp), 4)],
                    "not_slower_beyond_spread": bool(ms_l <= ms_c + spread),
                    "pairs_per_s": round(N * G / (ms_l * 1e-3)), "rows_with_the_compositions_indices": round(same, 4)})
        # per-launch device times of one call at the largest N (timing mode records every launch with its own events)
        L, h = model._L, model._h
        q = lat(max(args.rows))
        L.avae_timing_enable(h, 1)
        model.latent_topk(q, gal, k=k)
        buf = C.create_string_buffer(1 << 16)
        L.avae_timing_report(h, buf, len(buf))
        L.avae_timing_enable(h, 0)
        line["per_launch_nz%d_rows%d_symkl" % (nz, max(args.rows))] = {
            nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2)}
            for nm, c, a, _ in (ln.split() for ln in buf.value.decode().splitlines()) if nm.startswith("latent_topk")}
        del model
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
