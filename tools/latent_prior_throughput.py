#!/usr/bin/env python3
"""Cost of fit_latent_prior() per EM iteration (avae_gmm_fit: two launches per iteration, no host round trip) and of
latent_prior_score() (avae_gmm_score) against the EM a user writes in torch on the same device, device tensors in and out:
N posteriors in {4096, 65536, 1048576}, K in {10, 64} components, n_z in {20, 64}.  The data are K clusters (centres N(0, 9),
within-cluster scale U(0.3, 1), lv ~ U(-6, 1)); the calls only see latents, so the model is a small one.

Two compositions, both fp32, both the library's update (shifted sums about the current mean):
  broadcast   per chunk of rows the [c, K, n_z] tensor of squared deviations, c the largest chunk whose broadcast stays within
              --chunk-bytes (1 GiB); torch.logsumexp over K; the sums as reductions of [c, K, n_z] products;
  loop over K the same with a host loop over the components: [N, n_z] temporaries only, 2 K passes over the data.
Neither synchronises inside an iteration; both pay their launches.

hipEvent timing after a warm-up of all candidates, the median of --repeats calls with the candidates interleaved, the spread of
each (min, max) beside it.  The library is timed over --iters iterations (the call also runs its last scoring pass and the Python
marshalling: they are inside the figure), the compositions over --cmp-iters; reported per iteration.  Per case also: the
score call in milliseconds, the ratios composition / library, and the largest difference of the library's and the broadcast
composition's parameters after --cmp-iters iterations from the same start (|err| for weights, |err| / (|ref| + 1) for means and
log-variances), and the library's rate in GFLOP/s at 12 flops per (row, component, dimension): 5 in the exponent's chain, 7 in the sums.
No ratio is a condition.  One JSON line; --out FILE also writes it there."""
import argparse
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

LOG_2PI = math.log(2.0 * math.pi)


def arch(scope, n_in, h, n_z):
    return dict(scope=scope, hidden_conv=False, n_hidden_recog_1=h, n_hidden_recog_2=h, n_hidden_gener_1=h, n_hidden_gener_2=h,
                n_input=n_in, n_z=n_z)


def update(w, m, s, R, S1, S2, var_floor):
    q = S1 / R[:, None]
    return R / R.sum(), m + q, torch.log(torch.clamp(S2 / R[:, None] - q * q, min=var_floor))


def em_broadcast(mu, v, w, m, s, n_iters, chunk_bytes, var_floor=1e-6):
    N, nz = mu.shape
    K = w.shape[0]
    c = max(1, int(chunk_bytes // (K * nz * 4)))
    for _ in range(n_iters):
        iv, ck = torch.exp(-s), torch.log(w) - 0.5 * (s + LOG_2PI).sum(dim=1)
        R, S1, S2 = torch.zeros_like(w), torch.zeros_like(m), torch.zeros_like(m)
        for r0 in range(0, N, c):
            d = mu[r0:r0 + c, None, :] - m[None]
            q = d * d + v[r0:r0 + c, None, :]
            E = ck[None] - 0.5 * (q * iv[None]).sum(dim=2)
            r = torch.exp(E - torch.logsumexp(E, dim=1, keepdim=True))
            R += r.sum(dim=0)
            S1 += (r[:, :, None] * d).sum(dim=0)
            S2 += (r[:, :, None] * q).sum(dim=0)
        w, m, s = update(w, m, s, R, S1, S2, var_floor)
    return w, m, s


def em_loop(mu, v, w, m, s, n_iters, var_floor=1e-6):
    N, nz = mu.shape
    K = w.shape[0]
    for _ in range(n_iters):
        iv, ck = torch.exp(-s), torch.log(w) - 0.5 * (s + LOG_2PI).sum(dim=1)
        E = torch.empty((N, K), device=mu.device)
        for k in range(K):
            d = mu - m[k]
            E[:, k] = ck[k] - 0.5 * ((d * d + v) * iv[k]).sum(dim=1)
        r = torch.exp(E - torch.logsumexp(E, dim=1, keepdim=True))
        R, S1, S2 = r.sum(dim=0), torch.empty_like(m), torch.empty_like(m)
        for k in range(K):
            d = mu - m[k]
            S1[k] = (r[:, k, None] * d).sum(dim=0)
            S2[k] = (r[:, k, None] * (d * d + v)).sum(dim=0)
        w, m, s = update(w, m, s, R, S1, S2, var_floor)
    return w, m, s


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
    ap.add_argument("--components", type=int, nargs="*", default=[10, 64])
    ap.add_argument("--nz", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cmp-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"repeats": args.repeats, "iters": args.iters, "composition_iters": args.cmp_iters,
            "composition_chunk_bytes": args.chunk_bytes, "cases": []}
    for nz in args.nz:
        model = AssocVariationalAutoEncoder([arch("image", 784, 64, nz), arch("joint", 147, 64, nz)], binary=[True, False],
                                            transfer_fct="relu", batch_size=16, compute_dtype="fp32", seed=0)
        gen = torch.Generator(device="cuda").manual_seed(nz)
        for K in args.components:
            centres = 3.0 * torch.randn((K, nz), device="cuda", generator=gen)
            scale = torch.rand((K, nz), device="cuda", generator=gen) * 0.7 + 0.3
            for N in args.rows:
                label = torch.randint(0, K, (N,), device="cuda", generator=gen)
                mu = centres[label] + scale[label] * torch.randn((N, nz), device="cuda", generator=gen)
                lv = torch.rand((N, nz), device="cuda", generator=gen) * 7.0 - 6.0
                v = torch.exp(lv)
                init = model.fit_latent_prior((mu, lv), n_components=K, n_iters=0, seed=1)
                init = {k: init[k] for k in ("weights", "means", "logvars")}
                start = lambda: (init["weights"].clone(), init["means"].clone(), init["logvars"].clone())   # noqa: E731
                f_lib = lambda: model.fit_latent_prior((mu, lv), n_components=K, n_iters=args.iters, init=init)      # noqa: E731
                f_bc = lambda: em_broadcast(mu, v, *start(), args.cmp_iters, args.chunk_bytes)                       # noqa: E731
                f_lp = lambda: em_loop(mu, v, *start(), args.cmp_iters)                                              # noqa: E731
                f_sc = lambda: model.latent_prior_score((mu, lv), init, responsibilities=True)                       # noqa: E731
                for f in (f_lib, f_bc, f_lp, f_sc, f_lib, f_bc, f_lp, f_sc):
                    f()
                torch.cuda.synchronize()
                t = {"lib": [], "bc": [], "lp": [], "sc": []}
                for _ in range(args.repeats):                                                                        # interleaved
                    t["lib"].append(once(f_lib) / args.iters)
                    t["bc"].append(once(f_bc) / args.cmp_iters)
                    t["lp"].append(once(f_lp) / args.cmp_iters)
                    t["sc"].append(once(f_sc))
                a = model.fit_latent_prior((mu, lv), n_components=K, n_iters=args.cmp_iters, init=init)
                b = f_bc()
                rel = lambda x, y: float(((x.double() - y.double()).abs() / (y.double().abs() + 1)).max().item())    # noqa: E731
                diff = max(float((a["weights"].double() - b[0].double()).abs().max().item()), rel(a["means"], b[1]), rel(a["logvars"], b[2]))
                med = {k: float(np.median(x)) for k, x in t.items()}
                line["cases"].append({
                    "n_z": nz, "components": K, "rows": N,
                    "fit_ms_per_iteration": round(med["lib"], 4), "broadcast_ms_per_iteration": round(med["bc"], 4),
                    "loop_ms_per_iteration": round(med["lp"], 4), "score_ms": round(med["sc"], 4),
                    "ratio_broadcast": round(med["bc"] / med["lib"], 2), "ratio_loop": round(med["lp"] / med["lib"], 2),
                    "fit_min_max": [round(min(t["lib"]), 4), round(max(t["lib"]), 4)],
                    "broadcast_min_max": [round(min(t["bc"]), 4), round(max(t["bc"]), 4)],
                    "loop_min_max": [round(min(t["lp"]), 4), round(max(t["lp"]), 4)],
                    "score_min_max": [round(min(t["sc"]), 4), round(max(t["sc"]), 4)],
                    "fit_gflops": round(12e-9 * N * K * nz / (med["lib"] * 1e-3), 1),
                    "largest_parameter_difference": diff})
                print(json.dumps(line["cases"][-1]), file=sys.stderr, flush=True)
                del mu, lv, v
        del model
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
