#!/usr/bin/env python3
"""Cost of pen-path kinematics and stroke rendering (avae_motion_fk / avae_stroke_render) and of
draw_motion(), device tensors in and out: the 7-joint arm of tests/golden/baxter_right_chain.json, the reference's sigmoid basis
(100 phase points) around the writer's seed pose, the reference's canvas (28 x 28, half width 0.0625, margin 0.6), N rows in
{64, 4096} (64: the reference's rollout scale), ss in {4, 8}, hipEvent timing after a warm-up, the median of 7 repeats with the
candidates interleaved,

against the same definition written with torch in fp32: forward kinematics as a batched chain of 4 x 4 matrix products, the
renderer as a [samples, segments] broadcast of the point-segment distance with ``amin`` over the segments and ``mean`` over a
pixel's samples, in row chunks (--chunk-floats).

One JSON line; --out FILE also writes it there.  ``evals_per_s`` prices the library's render call at the definition's N (H ss)^2
(T - 1) point-segment distances, of which the kernel skips those of pixels that hold no ink."""
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
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, chain_matrices, motion_matrices

D, KB, T = 7, 21, 100


def torch_fk(traj, frames, axes):
    """[N, T, D] -> [N, T, 3]: T(q) = F_0 Rot_0 F_1 ... F_D as batched 4 x 4 products"""
    q = traj.reshape(-1, traj.shape[-1])
    M = q.shape[0]
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=q.device)
    F = torch.cat([frames, bottom.expand(frames.shape[0], 1, 4)], 1)
    eye = torch.eye(3, device=q.device)
    Tm = F[0].expand(M, 4, 4)
    for j in range(axes.shape[0]):
        a = axes[j]
        K = torch.stack([torch.stack([a.new_zeros(()), -a[2], a[1]]), torch.stack([a[2], a.new_zeros(()), -a[0]]),
                         torch.stack([-a[1], a[0], a.new_zeros(())])])
        c, s = torch.cos(q[:, j])[:, None, None], torch.sin(q[:, j])[:, None, None]
        R = torch.zeros((M, 4, 4), device=q.device)
        R[:, :3, :3] = c * eye + s * K + (1.0 - c) * torch.outer(a, a)
        R[:, 3, 3] = 1.0
        Tm = Tm @ R @ F[j + 1]
    return Tm[:, :3, 3].reshape(traj.shape[:-1] + (3,))


def torch_render(path, plane, r, margin, H, ss, chunk_floats):
    """[N, T, 3] -> (image [N, H * H], window [N, 3]) in row chunks"""
    N, Tn = path.shape[:2]
    n = H * ss
    c = (path - path.mean(1, keepdim=True)) @ plane[:2].T
    lo, hi = c.amin(1) - r, c.amax(1) + r
    ctr = (lo + hi) * 0.5
    W = (1.0 + margin) * (hi - lo).amax(1)
    delta = W / n
    k = torch.arange(n, device=path.device) + 0.5
    u = ctr[:, :1] - 0.5 * W[:, None] + k[None, :] * delta[:, None]
    v = ctr[:, 1:] + 0.5 * W[:, None] - k[None, :] * delta[:, None]
    a, d = c[:, :-1], c[:, 1:] - c[:, :-1]
    len2 = (d * d).sum(-1)
    inv = torch.where(len2 > 0, 1.0 / len2, torch.zeros_like(len2))
    rows = max(1, chunk_floats // (n * n * (Tn - 1)))
    out = []
    for r0 in range(0, N, rows):
        sl = slice(r0, r0 + rows)
        px = u[sl, None, :, None] - a[sl, None, None, :, 0]                    # [rows, 1, n, S]
        py = v[sl, :, None, None] - a[sl, None, None, :, 1]                    # [rows, n, 1, S]
        dx, dy, iv = d[sl, None, None, :, 0], d[sl, None, None, :, 1], inv[sl, None, None, :]
        t = ((px * dx + py * dy) * iv).clamp(0.0, 1.0)
        ex, ey = px - t * dx, py - t * dy
        dist = (ex * ex + ey * ey).amin(-1).sqrt()
        cov = (0.5 + (r - dist) / delta[sl, None, None]).clamp(0.0, 1.0)
        out.append(cov.view(-1, H, ss, H, ss).mean((2, 4)).flatten(1))
    return torch.cat(out), torch.cat([ctr, W[:, None]], 1)


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
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--ss", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-floats", type=int, default=1 << 26, help="distance floats the torch composition holds at a time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_chain.json")) as f:
        fx = json.load(f)
    chain = KinematicChain(fx["joints"])
    mean = np.zeros((D, KB))
    mean[:, -1] = fx["seed_pos"]
    # a spread of 0.012 rad per basis weight: strokes of a letter's size, 3 to 6 plane units across, 30 to 60 pixels of ink
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(D * KB, 0.012))
    m = motion_matrices(basis, model.device)
    frames, axes = chain_matrices(chain, model.device)
    line = {"config": label, "chain": "baxter right arm, 7 joints", "points": T, "repeats": args.repeats, "cases": {}}
    for N in args.rows:
        p = torch.randn((N, D * KB), device="cuda", generator=torch.Generator("cuda").manual_seed(N))
        traj = model.motion_eval(p, basis)["trajectory"]
        path = model.motion_fk(traj, chain)
        case = {"motion_fk": race(lambda: model.motion_fk(traj, chain), lambda: torch_fk(traj, frames, axes), args.repeats),
                "fk_max_abs_diff": float((path - torch_fk(traj, frames, axes)).abs().max())}
        for ss in args.ss:
            canvas = StrokeCanvas(supersample=ss)
            plane = torch.as_tensor(canvas.plane.astype(np.float32)).cuda()
            H, r, mg = canvas.size, canvas.half_width, canvas.margin

            def composed():
                theta = (p * m["scale"] + m["shift"]).unflatten(-1, (D, KB))
                q = torch.einsum("tk,ndk->ntd", m["phi"], theta)
                q = torch.minimum(torch.maximum(q, m["limits"][:, 0]), m["limits"][:, 1])
                return torch_render(torch_fk(q, frames, axes), plane, r, mg, H, ss, args.chunk_floats)
            sub = {"render_strokes": race(lambda: model.render_strokes(path, canvas),
                                          lambda: torch_render(path, plane, r, mg, H, ss, args.chunk_floats), args.repeats),
                   "draw_motion": race(lambda: model.draw_motion(p, basis, chain, canvas), composed, args.repeats)}
            a, b = model.render_strokes(path, canvas), torch_render(path, plane, r, mg, H, ss, args.chunk_floats)
            sub["image_max_abs_diff"] = float((a["image"] - b[0]).abs().max())
            sub["mean_ink_pixels"] = round(float(a["image"].sum(1).mean()), 1)
            sub["evals_per_s"] = float("%.3g" % (N * (H * ss) ** 2 * (T - 1) / (sub["render_strokes"]["library_ms"] * 1e-3)))
            case["ss%d" % ss] = sub
        line["cases"]["N%d" % N] = case
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
