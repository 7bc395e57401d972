#!/usr/bin/env python3
"""Cost of latent_stats() (avae_latent_stats: per-dimension posterior diagnostics in one fused pass) against the same statistics
written with torch on the same device, device tensors in and out: rows in {4096, 65536, 1048576}, n_z in {20, 64}, M = 2, with
and without a presence array.  Latents are random (mu ~ N(0, 1), lv ~ U(-6, 1)); the call only sees latents, so the model is a
small one.

The composition is the two-pass definition (the mean first, then the centred sums; absent rows weighted 0, which finite inputs
allow), once in float64 -- what the definition asks for -- and once in float32, which is faster and wrong where a mean dwarfs its
spread.  cov is the centred matrix product.

hipEvent timing after a warm-up of every candidate, the median of --repeats calls with the candidates interleaved, the spread of
each (min, max) beside it.  No ratio is fixed in advance.  Also reported: the bytes the call has to read over its time, the
largest difference of the call's result to the float64 composition's (relative to 1 + |value|), and the per-launch device times
of one call from avae_timing_report.  One JSON line; --out FILE also writes it there."""
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


def compose(post, present, dt):
    M = len(post)
    nz = post[0][0].shape[1]
    dev = post[0][0].device
    mu, lv = [p[0].to(dt) for p in post], [p[1].to(dt) for p in post]
    v, iv = [torch.exp(x) for x in lv], [torch.exp(-x) for x in lv]
    w = [None if present is None else present[:, m:m + 1].to(dt) for m in range(M)]
    out = {k: torch.empty((M, M, nz), dtype=dt, device=dev) for k in ("mean", "var", "xcov", "assoc")}
    out.update(count=torch.empty((M, M), dtype=torch.int64, device=dev), post_var=torch.empty((M, nz), dtype=dt, device=dev),
               kl=torch.empty((M, nz), dtype=dt, device=dev), cov=torch.empty((M, nz, nz), dtype=dt, device=dev))
    for s in range(M):
        for d in range(M):
            ws = None if present is None else w[s] * w[d]
            tot = (lambda a: a.sum(0)) if ws is None else (lambda a: (a * ws).sum(0))
            n = float(mu[s].shape[0]) if ws is None else ws.sum()
            out["count"][s, d] = n
            ms, md = tot(mu[s]) / n, tot(mu[d]) / n
            cs, cd = mu[s] - ms, mu[d] - md
            out["mean"][s, d] = ms
            out["var"][s, d] = tot(cs * cs) / n
            out["xcov"][s, d] = tot(cs * cd) / n
            t, df = v[s] - v[d], mu[s] - mu[d]
            out["assoc"][s, d] = tot(0.5 * ((t * iv[s]) * (t * iv[d]) + (df * df) * (iv[s] + iv[d]))) / n
            if s == d:
                out["post_var"][s] = tot(v[s]) / n
                out["kl"][s] = tot(0.5 * (mu[s] * mu[s] + v[s] - lv[s] - 1.0)) / n
                cw = cs if ws is None else cs * ws
                out["cov"][s] = cw.T @ cs / n
    return out


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--nz", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    M = 2
    line = {"n_mod": M, "repeats": args.repeats, "cases": []}
    for nz in args.nz:
        model = AssocVariationalAutoEncoder([arch("image", 784, 64, nz), arch("joint", 147, 64, nz)], binary=[True, False],
                                            transfer_fct="relu", batch_size=16, compute_dtype="fp32", seed=0)
        gen = torch.Generator(device="cuda").manual_seed(nz)
        for N in args.rows:
            post = [(torch.randn((N, nz), device="cuda", generator=gen), torch.rand((N, nz), device="cuda", generator=gen) * 7.0 - 6.0)
                    for _ in range(M)]
            flags = torch.rand((N, M), device="cuda", generator=gen) < 0.7
            for present in (None, flags):
                cands = {"latent_stats": lambda: model.latent_stats(post, present),
                         "torch_float64": lambda: compose(post, present, torch.float64),
                         "torch_float32": lambda: compose(post, present, torch.float32)}
                for _ in range(2):
                    for f in cands.values():
                        f()
                torch.cuda.synchronize()
                ts = {k: [] for k in cands}
                for _ in range(args.repeats):                                                  # interleaved
                    for k, f in cands.items():
                        ts[k].append(once(f))
                a, b = cands["latent_stats"](), cands["torch_float64"]()
                diff = max(float(((a[k] - b[k]).abs() / (1.0 + b[k].abs())).max().item()) for k in a if k != "count")
                med = {k: float(np.median(v)) for k, v in ts.items()}
                read_bytes = M * N * nz * 4 * 2 * 2 + (0 if present is None else 3 * N * M)   # every (mu, lv) twice: its own item, the pair's
                line["cases"].append({
                    "n_z": nz, "rows": N, "present": present is not None,
                    **{k + "_ms": round(v, 4) for k, v in med.items()},
                    **{k + "_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in ts.items()},
                    "float64_over_call": round(med["torch_float64"] / med["latent_stats"], 2),
                    "float32_over_call": round(med["torch_float32"] / med["latent_stats"], 2),
                    "call_read_GBps": round(read_bytes / (med["latent_stats"] * 1e-3) / 1e9, 1),
                    "counts_equal": bool((a["count"] == b["count"]).all().item()), "max_diff_to_float64": diff})
            del post, flags
            torch.cuda.empty_cache()
        # per-launch device times of one call at the largest size (timing mode records every launch with its own events)
        L, h = model._L, model._h
        N = max(args.rows)
        post = [(torch.randn((N, nz), device="cuda", generator=gen), torch.rand((N, nz), device="cuda", generator=gen) * 7.0 - 6.0)
                for _ in range(M)]
        L.avae_timing_enable(h, 1)
        model.latent_stats(post)
        buf = C.create_string_buffer(1 << 16)
        L.avae_timing_report(h, buf, len(buf))
        L.avae_timing_enable(h, 0)
        line["per_launch_nz%d_rows%d" % (nz, N)] = {
            nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2)}
            for nm, c, a, _ in (ln.split() for ln in buf.value.decode().splitlines()) if nm.startswith("latent_stats")}
        del model, post
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
