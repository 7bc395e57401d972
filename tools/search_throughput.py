#!/usr/bin/env python3
"""Cost of the black-box search (avae_search_sample / avae_search_update), device tensors in and out, hipEvent
timing after a warm-up, the median of 7 repeats with the candidates interleaved.

1. One sample + update pair at P in {1, 256, 4096}, R in {10, 20, 64}, n in {20, 147} (PI-BB weights, the default bounds) against
   the same definition written with torch in fp32: ``randn``, the exponential weights, two ``einsum``s and the bounds.
2. ``refine_motion`` on C2 at P = 64 and P = 4096 in both spaces, ``--iters`` iterations, split with avae_timing_report into the
   two search launches and the cost pipeline (every other launch of the call: decode, motion_eval, motion_fk, stroke_render,
   encode; the P rows priced before and after the loop included).

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
from vae_assoc_amd import _capi
from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
from vae_assoc_amd.motion import MotionBasis
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, search_args

D, KB = 7, 21


def torch_pair(mean, var, cost_fn, R, h=10.0, rel_lower=0.1):
    """one PI-BB iteration in fp32: draw, price, weight, refit, bound -> (mean, var)"""
    x = mean[:, None, :] + var.sqrt()[:, None, :] * torch.randn((mean.shape[0], R, mean.shape[1]), device=mean.device)
    c = cost_fn(x)
    lo, hi = c.amin(1, keepdim=True), c.amax(1, keepdim=True)
    w = torch.exp(-h * (c - lo) / (hi - lo + 1e-6))
    w = w / w.sum(1, keepdim=True)
    m1 = torch.einsum("pr,prn->pn", w, x)
    v1 = torch.einsum("pr,prn->pn", w, (x - mean[:, None, :]) ** 2)
    return m1, torch.maximum(v1, rel_lower * v1.amax(1, keepdim=True))


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


def timing(model):
    """avae_timing_report -> {launch name: (calls, total ms)}"""
    buf = C.create_string_buffer(1 << 16)
    _capi.check(model._h, model._L.avae_timing_report(model._h, buf, len(buf)), "avae_timing_report")
    out = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        if len(f) >= 3 and f[0] != "_null_kernel":
            out[f[0]] = (int(f[1]), int(f[1]) * float(f[2]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 256, 4096])
    ap.add_argument("--rollouts", type=int, nargs="*", default=[10, 20, 64])
    ap.add_argument("--dims", type=int, nargs="*", default=[20, 147])
    ap.add_argument("--refine-problems", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    line = {"config": label, "repeats": args.repeats, "pair": {}, "refine_motion": {}}
    cost_fn = lambda x: torch.linalg.vector_norm(x, dim=-1)
    for P in args.problems:
        for R in args.rollouts:
            for n in args.dims:
                x0 = torch.randn((P, n), device="cuda", generator=torch.Generator("cuda").manual_seed(P + R + n))
                st, opt, _, _, _, _, _ = search_args(x0, 0.01, R, 1, 10, "PI-BB", "PI-BB", 1.0, (0.1,), 0.0, None, 0, None, model.device)
                x = torch.empty((P, R, n), device="cuda")
                hist = torch.empty((3, P), device="cuda")

                def pair():
                    model._search_sample(st, R, 0, 0, None, x)
                    model._search_update(st, x, cost_fn(x), opt, hist[0], hist[1], hist[2])
                    st["var"].fill_(0.01)                                                  # (keep the problem alive over the repeats)
                mean, var = x0.clone(), torch.full_like(x0, 0.01)
                line["pair"]["P%d_R%d_n%d" % (P, R, n)] = race(pair, lambda: torch_pair(mean, var, cost_fn, R), args.repeats)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_chain.json")) as f:
        fx = json.load(f)
    chain = KinematicChain(fx["joints"])
    mean = np.zeros((D, KB))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(D * KB, 0.012))
    canvas = StrokeCanvas()
    for P in args.refine_problems:
        z = torch.randn((P, model.n_z), device="cuda", generator=torch.Generator("cuda").manual_seed(P))
        img = model.draw_motion(model.generate(z)[1], basis, chain, canvas)["image"]
        for space in ("latent", "params"):
            run = lambda: model.refine_motion(img, basis, chain, canvas, space=space, n_iters=args.iters, tol=0.0)
            run()
            torch.cuda.synchronize()
            wall = float(np.median([once(run) for _ in range(args.repeats)]))
            _capi.check(model._h, model._L.avae_timing_enable(model._h, 1), "avae_timing_enable")
            run()
            torch.cuda.synchronize()
            t = timing(model)
            _capi.check(model._h, model._L.avae_timing_enable(model._h, 0), "avae_timing_enable")
            search = sum(ms for k, (_, ms) in t.items() if k.startswith("search_"))
            total = sum(ms for _, ms in t.values())
            line["refine_motion"]["P%d_%s" % (P, space)] = {
                "iters": args.iters, "call_ms": round(wall, 3), "ms_per_iter": round(wall / args.iters, 3),
                "kernel_ms": round(total, 3), "search_kernel_ms": round(search, 4), "search_share": round(search / total, 5),
                "launches": {k: [c, round(ms, 4)] for k, (c, ms) in sorted(t.items(), key=lambda kv: -kv[1][1])}}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
