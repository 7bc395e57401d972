#!/usr/bin/env python3
"""Cost of one iteration of embed_latents() (avae_embed_iterate: k_embed_forces + k_embed_update, no host round trip) and of one
calibration (avae_embed_calibrate) against the same definition written densely with torch in fp32 on the same device: N
posteriors in {4096, 16384, 65536}, n_z in {20, 64}, both metrics.  The data are 10 clusters (centres N(0, 9), within-cluster
scale U(0.3, 1), lv ~ U(-6, 1)); the calls only see latents, so the model is a small one.

The dense form keeps D, P and the map's W as N x N fp32 matrices (plus temporaries) and is run only where three of them fit
--dense-bytes (4 GiB: N = 16,384 and below); its calibration runs --dense-tries fixed bisection steps for all rows at once (the
library stops row by row, at 15 to 25 tries on this data), so the two calibrations are reported side by side, not as a ratio.

hipEvent timing after a warm-up of all candidates, the median of --repeats calls with the candidates interleaved, the spread
(min, max) beside it.  The library's iteration is a call of --iters iterations minus a call of none (the evaluating pass and the
Python marshalling, reported beside it), per iteration; the calibration likewise; avae_timing_report gives the device time of every launch
of one more call.  Also the library's rate in GFLOP/s at n_z (L2) or 3 n_z (SYMKL) fused multiply-adds plus 30 flops per pair.
No ratio is a condition.  One JSON line; --out FILE also writes it there."""
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


def dense_distances(mu, lv, metric):
    if metric == "l2":
        return torch.cdist(mu, mu).square_()
    v, iv = torch.exp(lv), torch.exp(-lv)
    # sum_j (v_i - v_j)^2 iv_i iv_j + (mu_i - mu_j)^2 (iv_i + iv_j), expanded into matrix products
    a = v @ iv.T
    D = a + a.T - 2.0 * mu.shape[1]
    m2 = mu * mu
    b = (m2 * iv).sum(dim=1)
    c = m2 @ iv.T
    e = (mu * iv) @ mu.T
    D += b[:, None] + b[None, :] + c + c.T - 2.0 * (e + e.T)
    return D.mul_(0.5).clamp_(min=0.0)


def dense_calibrate(D, perplexity, tries):
    N = D.shape[0]
    D = D.clone()
    D.fill_diagonal_(float("inf"))
    m = D.min(dim=1).values
    T = D - m[:, None]
    beta = torch.ones(N, device=D.device)
    lo, hi = torch.zeros_like(beta), torch.full_like(beta, float("inf"))
    target = float(np.log(perplexity))
    for _ in range(tries):
        Ex = torch.exp(-beta[:, None] * T)
        s0 = Ex.sum(dim=1)
        H = torch.log(s0) + beta * torch.nan_to_num(T * Ex).sum(dim=1) / s0
        up = H > target
        lo, hi = torch.where(up, beta, lo), torch.where(up, hi, beta)
        beta = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2), torch.where(lo == 0, beta / 2, (beta + lo) / 2))
    Ex = torch.exp(-beta[:, None] * T)
    return beta, m, Ex.sum(dim=1)


def dense_iteration(P, y, vel, gain, alpha, mom, lr):
    d2 = torch.cdist(y, y).square_()
    W = 1.0 / (1.0 + d2)
    W.fill_diagonal_(0.0)
    Z = W.sum()
    PW = P * W
    A = PW.sum(dim=1, keepdim=True) * y - PW @ y
    W2 = W * W
    R = W2.sum(dim=1, keepdim=True) * y - W2 @ y
    grad = 4.0 * (alpha * A - R / Z)
    kl = (torch.xlogy(P, P) - P * torch.log(W.clamp_min(1e-38))).sum() + torch.log(Z)
    gain = torch.where((grad > 0) != (vel > 0), gain + 0.2, gain * 0.8).clamp_min(0.01)
    vel = mom * vel - lr * gain * grad
    return y + vel, vel, gain, kl


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(model, fn):
    """device time per launch of one call of fn, from avae_timing_report: {name: [calls, avg_ms]}"""
    L, h = model._L, model._h
    L.avae_timing_enable(h, 1)
    fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    L.avae_timing_report(h, buf, len(buf))
    L.avae_timing_enable(h, 0)
    out = {}
    for row in buf.value.decode().splitlines():
        f = row.split()
        if len(f) >= 3 and f[0].startswith("embed_"):
            out[f[0]] = [int(f[1]), round(float(f[2]), 4)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[4096, 16384, 65536])
    ap.add_argument("--nz", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--metrics", nargs="*", default=["symkl", "l2"])
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dense-bytes", type=int, default=4 << 30)
    ap.add_argument("--dense-tries", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"repeats": args.repeats, "iters": args.iters, "perplexity": args.perplexity, "dense_tries": args.dense_tries, "cases": []}
    for nz in args.nz:
        model = AssocVariationalAutoEncoder([arch("image", 784, 64, nz), arch("joint", 147, 64, nz)], binary=[True, False],
                                            transfer_fct="relu", batch_size=16, compute_dtype="fp32", seed=0)
        gen = torch.Generator(device="cuda").manual_seed(nz)
        centres = 3.0 * torch.randn((10, nz), device="cuda", generator=gen)
        scale = torch.rand((10, nz), device="cuda", generator=gen) * 0.7 + 0.3
        for N in args.rows:
            label = torch.randint(0, 10, (N,), device="cuda", generator=gen)
            mu = centres[label] + scale[label] * torch.randn((N, nz), device="cuda", generator=gen)
            lv = torch.rand((N, nz), device="cuda", generator=gen) * 7.0 - 6.0
            for metric in args.metrics:
                kw = dict(perplexity=args.perplexity, metric=metric)
                first = model.embed_latents((mu, lv), n_iters=0, **kw)             # calibrates
                f_cal = lambda: model.embed_latents((mu, lv), n_iters=0, **kw)                               # noqa: E731
                f_it = lambda: model.embed_latents((mu, lv), n_iters=args.iters, state=first["state"], **kw)  # noqa: E731
                f_ev = lambda: model.embed_latents((mu, lv), n_iters=0, state=first["state"], **kw)           # noqa: E731
                dense = 3 * N * N * 4 <= args.dense_bytes
                cands = {"cal": f_cal, "it": f_it, "ev": f_ev}
                if dense:
                    D = dense_distances(mu, lv, metric)
                    beta, m, s0 = dense_calibrate(D, args.perplexity, args.dense_tries)
                    Ec = torch.exp(-beta[:, None] * (D - m[:, None])) / (2.0 * N * s0[:, None])
                    Ec.fill_diagonal_(0.0)
                    Pm = Ec + Ec.T
                    del Ec
                    y0 = first["embedding"].clone()
                    st = (y0, torch.zeros_like(y0), torch.ones_like(y0))
                    cands["dense_it"] = lambda: dense_iteration(Pm, *st, 12.0, 0.5, max(N / 48.0, 50.0))     # noqa: E731
                    cands["dense_cal"] = lambda: dense_calibrate(dense_distances(mu, lv, metric), args.perplexity, args.dense_tries)  # noqa: E731
                for _ in range(2):
                    for f in cands.values():
                        f()
                torch.cuda.synchronize()
                t = {k: [] for k in cands}
                for _ in range(args.repeats):                                                                 # interleaved
                    for k, f in cands.items():
                        t[k].append(once(f))
                med = {k: float(np.median(x)) for k, x in t.items()}
                it_ms = (med["it"] - med["ev"]) / args.iters                     # the call's evaluating pass and marshalling taken out
                flops = ((1 if metric == "l2" else 3) * 2 * nz + 30) * float(N) * N
                case = {"n_z": nz, "rows": N, "metric": metric, "iteration_ms": round(it_ms, 4),
                        "calibration_ms": round(med["cal"] - med["ev"], 4), "evaluation_call_ms": round(med["ev"], 4),
                        "iteration_call_min_max": [round(min(t["it"]), 4), round(max(t["it"]), 4)],
                        "calibration_call_min_max": [round(min(t["cal"]), 4), round(max(t["cal"]), 4)],
                        "iteration_gflops": round(flops * 1e-9 / (it_ms * 1e-3), 1),
                        "launches_iterate": launches(model, f_it), "launches_calibrate": launches(model, f_cal)}
                if dense:
                    case.update({"dense_iteration_ms": round(med["dense_it"], 4), "dense_calibration_ms": round(med["dense_cal"], 4),
                                 "ratio_iteration": round(med["dense_it"] / it_ms, 2),
                                 "dense_iteration_min_max": [round(min(t["dense_it"]), 4), round(max(t["dense_it"]), 4)]})
                    del D, Pm
                line["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
            del mu, lv
        del model
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
