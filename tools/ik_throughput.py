#!/usr/bin/env python3
"""Cost of inverse kinematics (avae_motion_ik) and of strokes_to_motion(), device tensors in and out: the
7-joint arm of tests/golden/baxter_right_chain.json seeded at the writer's seed pose, N letter-like strokes of 100 points spanning
+-1.5 plane units on the reference's writing block, N in {64, 4096, 65536}, position only and with the seed pose's orientation as
goal, the default options; hipEvent timing after a warm-up, the median of 7 repeats with the candidates interleaved,

against the same definition written with torch in fp32: the chain walked with batched [N, 3, 3] products, ``torch.linalg.cholesky``
and ``cholesky_solve`` on [N, m, m], a host loop over the time points and a fixed number of steps per point equal to the largest
``iterations`` the kernel reports (no statuses, no early stop: every row takes every step).

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
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, chain_matrices

D, KB, T = 7, 21, 100


def letters(N, seed=0):
    """[N, T, 2] smooth strokes in plane units, scaled to span +-1.5"""
    rng = np.random.default_rng(seed)
    tau = np.linspace(0.0, 1.0, T)
    f, ph, amp = rng.uniform(0.5, 2.5, (N, 2, 3, 1)), rng.uniform(0, 2 * np.pi, (N, 2, 3, 1)), rng.uniform(0.2, 1.0, (N, 2, 3, 1))
    uv = (amp * np.sin(2 * np.pi * f * tau + ph)).sum(2).transpose(0, 2, 1)
    return 1.5 * uv / np.abs(uv).max(axis=(1, 2), keepdims=True)


def torch_walk(q, frames, axes):
    """[N, D] -> (p [N, 3], R [N, 3, 3], J [N, 6, D])"""
    N = q.shape[0]
    R = torch.eye(3, device=q.device).expand(N, 3, 3)
    p = torch.zeros((N, 3), device=q.device)
    eye = torch.eye(3, device=q.device)
    o, z = [], []
    for j in range(axes.shape[0]):
        p = p + R @ frames[j, :, 3]
        R = R @ frames[j, :, :3]
        a = axes[j]
        o.append(p)
        z.append(R @ a)
        zero = a.new_zeros(())
        K = torch.stack([torch.stack([zero, -a[2], a[1]]), torch.stack([a[2], zero, -a[0]]), torch.stack([-a[1], a[0], zero])])
        c, s = torch.cos(q[:, j])[:, None, None], torch.sin(q[:, j])[:, None, None]
        R = R @ (c * eye + s * K + (1.0 - c) * torch.outer(a, a))
    p = p + R @ frames[-1, :, 3]
    R = R @ frames[-1, :, :3]
    o, z = torch.stack(o, 1), torch.stack(z, 1)
    J = torch.cat([torch.linalg.cross(z, p[:, None, :] - o), z], dim=2).transpose(1, 2)
    return p, R, J


def torch_ik(path, frames, axes, seed, goal, limits, steps, damping=0.01, max_step=0.5):
    """[N, T, 3] -> [N, T, D]: ``steps`` damped least-squares steps at every point, every row"""
    q = seed.clone()
    out = torch.empty(path.shape[:2] + (q.shape[1],), device=path.device)
    m = 3 if goal is None else 6
    lam = damping * damping * torch.eye(m, device=path.device)
    for t in range(path.shape[1]):
        for _ in range(steps):
            p, R, J = torch_walk(q, frames, axes)
            e = path[:, t] - p
            if goal is not None:
                e = torch.cat([e, 0.5 * torch.linalg.cross(R, goal.expand_as(R), dim=1).sum(2)], dim=1)
            J = J[:, :m]
            L = torch.linalg.cholesky(J @ J.transpose(1, 2) + lam)
            dq = (J.transpose(1, 2) @ torch.cholesky_solve(e[:, :, None], L))[:, :, 0]
            big = dq.abs().amax(1, keepdim=True)
            dq = torch.where(big > max_step, dq * (max_step / big), dq)
            q = torch.minimum(torch.maximum(q + dq, limits[:, 0]), limits[:, 1])
        out[:, t] = q
    return out


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def race(f_lib, f_torch, repeats):
    for f in (f_lib, f_torch):
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
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 4096, 65536])
    ap.add_argument("--pipeline-rows", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_chain.json")) as f:
        fx = json.load(f)
    chain, canvas = KinematicChain(fx["joints"]), StrokeCanvas()
    frames, axes = chain_matrices(chain, model.device)
    limits = torch.as_tensor(chain.limits.astype(np.float32)).cuda()
    seed_pos = np.asarray(fx["seed_pos"])
    goal = torch.as_tensor(chain.pose(seed_pos)[1].astype(np.float32)).cuda()
    line = {"config": label, "chain": "baxter right arm, 7 joints", "points": T, "repeats": args.repeats, "cases": {}}
    for N in args.rows:
        path = torch.as_tensor(canvas.lift(letters(N, N), fx["block_center"]).astype(np.float32)).cuda()
        seed = torch.as_tensor(np.tile(seed_pos.astype(np.float32), (N, 1))).cuda()
        case = {}
        for name, orient in (("position", None), ("goal", goal)):
            res = model.motion_ik(path, chain, seed, orientation=orient)
            steps = int(res["iterations"].max())
            ref = torch_ik(path, frames, axes, seed, orient, limits, steps)
            sub = race(lambda: model.motion_ik(path, chain, seed, orientation=orient),
                       lambda: torch_ik(path, frames, axes, seed, orient, limits, steps), args.repeats)
            sub.update(steps=steps, converged=float(res["converged"].float().mean()), mean_iterations=round(float(res["iterations"].float().mean()), 3),
                       max_abs_diff=float((res["trajectory"] - ref).abs().max()), residual_max=float(res["residual"].max()),
                       points_per_s=float("%.3g" % (N * T / (sub["library_ms"] * 1e-3))))
            case[name] = sub
        line["cases"]["N%d" % N] = case
    N = args.pipeline_rows
    mean = np.zeros((D, KB))
    mean[:, -1] = seed_pos
    basis = MotionBasis(limits=chain.limits, param_mean=mean.reshape(-1), param_std=np.full(D * KB, 0.012))
    strokes = torch.as_tensor(letters(N, 1)).cuda()

    def pipeline():
        return model.strokes_to_motion(strokes, basis, chain, canvas, fx["block_center"], seed_pos, orientation="seed")
    out = pipeline()
    torch.cuda.synchronize()
    ts = [once(pipeline) for _ in range(args.repeats)]
    line["strokes_to_motion"] = {"rows": N, "ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                                 "converged": float(out["converged"].float().mean()), "fit_rmse_max": float(out["fit_rmse"].max()),
                                 "tip_error_max": float(out["tip_error"].max()),
                                 "note": "the strokes start on the device; the lift runs on the host in float64, so the figure holds one "
                                         "round trip of [N, T, 2] and one upload of [N, T, 3]"}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
