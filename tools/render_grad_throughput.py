#!/usr/bin/env python3
"""Cost of the gradients through the writing chain (avae_stroke_render_vjp / avae_motion_fk_vjp / avae_motion_eval_vjp /
avae_rows_adam), device tensors in and out, hipEvent timing after a warm-up, the median of 7 repeats with the
candidates interleaved.  N in {64, 4096} motions of T = 100 points on the fixture arm, 28 x 28 pictures at ss = 4.

1. ``writing_cost_grad`` against the same definition written with torch in fp32 and differentiated by torch autograd (in chunks
   of ``--torch-chunk`` rows: a chunk's [rows, 99, 112, 112] distance tensors are what fits).
2. ``writing_cost_grad`` against ``writing_cost`` with the latent weight 0: the price of the gradient over the price of the cost.
3. One ``descend_motion`` iteration against one ``refine_motion(space='params')`` iteration at 10 rollouts, each as
   (call with 5 iterations - call with 1) / 4.
4. What the two refinements reach: ``--letters`` seeded letters (drawings of decoded motions), the start those parameters
   perturbed, ``--renders`` drawings per picture each -- that many descent steps, a tenth as many search iterations of 10
   rollouts -- and the ``img_l2`` before and after, both priced by ``w0 (img_l2 + w1 height_l2)`` alone and neither anchored to
   the first trajectory's start (``anchor_start=False``: the two then move the same parameters).

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
from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
from vae_assoc_amd.motion import MotionBasis
from vae_assoc_amd.vae_assoc import (AssocVariationalAutoEncoder, chain_matrices, descend_motion, motion_matrices,
                                     writing_cost_grad)

D, KB = 7, 21
W = (0.3, 10.0)


def torch_cost(p, mats, frames, axes, plane, canvas, target):
    """writing_cost_grad's cost in torch fp32 -> [rows]; differentiable in ``p``"""
    N, T = p.shape[0], mats["phi"].shape[0]
    theta = (p * mats["scale"] + mats["shift"]).reshape(N, D, KB)
    q = torch.einsum("tk,ndk->ntd", mats["phi"], theta)
    q = torch.minimum(torch.maximum(q, mats["limits"][:, 0]), mats["limits"][:, 1])
    v = frames[D, :, 3].expand(N, T, 3)
    for j in range(D - 1, -1, -1):
        a, s, c = axes[j], torch.sin(q[..., j:j + 1]), torch.cos(q[..., j:j + 1])
        w = v * c + torch.cross(a.expand_as(v), v, dim=-1) * s + a * ((v * a).sum(-1, keepdim=True) * (1.0 - c))
        v = w @ frames[j, :, :3].T + frames[j, :, 3]
    height = (v @ plane[2]).mean(1, keepdim=True).detach()
    height_l2 = torch.sqrt((((v @ plane[2]) - height) ** 2).sum(1))
    cc = (v - v.mean(1, keepdim=True)) @ plane[:2].T                                        # [N, T, 2]
    r, n = canvas.half_width, canvas.size * canvas.supersample
    lo, hi = cc.amin(1) - r, cc.amax(1) + r
    ctr, Wd = (lo + hi) / 2.0, (1.0 + canvas.margin) * (hi - lo).amax(1)
    delta = Wd / n
    alpha = (torch.arange(n, device=p.device) + 0.5) / n - 0.5
    u = ctr[:, 0, None] + Wd[:, None] * alpha                                              # [N, n]
    vv = ctr[:, 1, None] - Wd[:, None] * alpha
    A, Bv = cc[:, :-1], cc[:, 1:] - cc[:, :-1]                                             # [N, S, 2]
    len2 = (Bv ** 2).sum(-1).clamp_min(1e-30)
    px = u[:, None, None, :] - A[:, :, 0, None, None]                                      # [N, S, 1, n]
    py = vv[:, None, :, None] - A[:, :, 1, None, None]                                     # [N, S, n, 1]
    t = ((px * Bv[:, :, 0, None, None] + py * Bv[:, :, 1, None, None]) / len2[:, :, None, None]).clamp(0.0, 1.0)
    d2 = ((px - t * Bv[:, :, 0, None, None]) ** 2 + (py - t * Bv[:, :, 1, None, None]) ** 2).amin(1)
    cov = (0.5 + (r - torch.sqrt(d2.clamp_min(1e-30))) / delta[:, None, None]).clamp(0.0, 1.0)
    H, ss = canvas.size, canvas.supersample
    image = cov.reshape(N, H, ss, H, ss).mean((2, 4)).reshape(N, H * H)
    img_l2 = torch.sqrt(((image - target) ** 2).sum(1))
    return W[0] * (img_l2 + W[1] * height_l2)


def torch_grad(p, mats, frames, axes, plane, canvas, target, chunk):
    out = torch.empty_like(p)
    for r0 in range(0, p.shape[0], chunk):
        x = p[r0:r0 + chunk].detach().requires_grad_(True)
        torch_cost(x, mats, frames, axes, plane, canvas, target[r0:r0 + chunk]).sum().backward()
        out[r0:r0 + chunk] = x.grad
    return out


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def race(f_a, f_b, repeats, names):
    for f in (f_a, f_b, f_a, f_b):
        f()
    torch.cuda.synchronize()
    t_a, t_b = [], []
    for _ in range(repeats):                                                               # interleaved
        t_a.append(once(f_a))
        t_b.append(once(f_b))
    ms_a, ms_b = float(np.median(t_a)), float(np.median(t_b))
    return {names[0] + "_ms": round(ms_a, 4), names[1] + "_ms": round(ms_b, 4), "ratio": round(ms_b / ms_a, 3),
            names[0] + "_ms_min_max": [round(min(t_a), 4), round(max(t_a), 4)],
            names[1] + "_ms_min_max": [round(min(t_b), 4), round(max(t_b), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch-chunk", type=int, default=16)
    ap.add_argument("--letters", type=int, default=64)
    ap.add_argument("--renders", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_chain.json")) as f:
        fx = json.load(f)
    chain = KinematicChain(fx["joints"])
    mean = np.zeros((D, KB))
    mean[:, -1] = fx["seed_pos"]
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(D * KB, 0.012))
    canvas = StrokeCanvas()
    mats, (frames, axes) = motion_matrices(basis, model.device), chain_matrices(chain, model.device)
    plane = torch.as_tensor(canvas.plane, dtype=torch.float32, device=model.device)
    line = {"config": label, "repeats": args.repeats, "T": basis.n_points, "H": canvas.size, "ss": canvas.supersample,
            "grad_vs_torch": {}, "grad_vs_cost": {}, "iteration": {}}

    def letters(N, seed):
        gen = torch.Generator("cuda").manual_seed(seed)
        true = torch.randn((N, D * KB), device="cuda", generator=gen)
        start = true + 0.25 * torch.randn((N, D * KB), device="cuda", generator=gen)
        return true, start, model.draw_motion(true, basis, chain, canvas)["image"]

    for N in args.rows:
        true, start, img = letters(N, N)
        lib = lambda: writing_cost_grad(model, start, basis, chain, canvas, img, weights=W)
        ref = lambda: torch_grad(start, mats, frames, axes, plane, canvas, img, args.torch_chunk)
        r = race(lib, ref, args.repeats, ("library", "torch"))
        g_lib, g_ref = lib()["grad"], ref()
        top = g_ref.abs().amax(1).clamp_min(1e-30)
        r["median_row_err"] = float(((g_lib - g_ref).abs().amax(1) / top).median())         # (two fp32 paths; rows on a kink differ)
        line["grad_vs_torch"]["N%d" % N] = r
        cost = lambda: model.writing_cost(start, basis, chain, canvas, img, weights=W + (0.0,))
        line["grad_vs_cost"]["N%d" % N] = race(lib, cost, args.repeats, ("grad", "cost"))

        def per_iter(call):
            f1, f5 = (lambda: call(1)), (lambda: call(5))
            for f in (f1, f5):
                f()
            torch.cuda.synchronize()
            t1, t5 = [], []
            for _ in range(args.repeats):
                t1.append(once(f1))
                t5.append(once(f5))
            return (float(np.median(t5)) - float(np.median(t1))) / 4.0
        d_ms = per_iter(lambda k: descend_motion(model, img, basis, chain, canvas, init=start, n_iters=k, lr=args.lr, weights=W))
        s_ms = per_iter(lambda k: model.refine_motion(img, basis, chain, canvas, space="params", init=start, n_rollouts=10, n_iters=k,
                                                      weights=W + (0.0,), tol=0.0))
        line["iteration"]["N%d" % N] = {"descend_ms": round(d_ms, 4), "refine_R10_ms": round(s_ms, 4), "ratio": round(s_ms / d_ms, 3)}

    true, start, img = letters(args.letters, 7)
    K = args.renders
    first = model.writing_cost(start, basis, chain, canvas, img, weights=W + (0.0,))
    des = descend_motion(model, img, basis, chain, canvas, init=start, n_iters=K, lr=args.lr, weights=W, anchor_start=False)
    ref = model.refine_motion(img, basis, chain, canvas, space="params", init=start, n_rollouts=10, n_iters=K // 10, weights=W + (0.0,),
                              tol=0.0, anchor_start=False)
    best = model.draw_motion(des["best_params"], basis, chain, canvas, target=img)
    ref_best = model.draw_motion(ref["best_x"], basis, chain, canvas, target=img)

    def stats(t):
        t = t.float()
        return {"mean": round(float(t.mean()), 4), "median": round(float(t.median()), 4), "max": round(float(t.max()), 4)}
    line["reach"] = {"letters": args.letters, "renders_per_picture": K, "lr": args.lr,
                     "start_img_l2": stats(first["img_l2"]), "descend_img_l2": stats(des["img_l2"]),
                     "descend_best_img_l2": stats(best["img_l2"]), "refine_img_l2": stats(ref["final"]["img_l2"]),
                     "refine_best_img_l2": stats(ref_best["img_l2"]), "refine_best_cost": stats(ref["best_cost"]),
                     "start_cost": stats(first["cost"]), "descend_cost": stats(des["cost"]), "descend_best_cost": stats(des["best_cost"]),
                     "refine_cost": stats(ref["final"]["cost"])}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
