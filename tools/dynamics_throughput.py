#!/usr/bin/env python3
"""Cost of avae_motion_dynamics against the same definition written with batched torch in fp32 -- recursive
Newton-Euler as a Python loop over the joints, every tensor batched over the points -- device tensors in and out, hipEvent timing
after a warm-up, the median of 7 repeats with the two interleaved.  N in {64, 4096} trajectories of T = 100 points on the fixture
arm (D = 7), speeds and accelerations given; two output sets: the torque alone, and the torque with the inertia matrix (D more
unit-acceleration passes on either side).

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
from vae_assoc_amd._pen_api import _motion_dynamics
from vae_assoc_amd.kinematics import KinematicChain
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, chain_bodies, chain_matrices

GRAVITY = (0.0, 0.0, -9.81)


def cross(a, b):
    return torch.linalg.cross(a, b, dim=-1)


def torch_world(q, frames, axes, bodies):
    """the walk with the bodies carried along -> (o, z, r [n, D, 3], I [n, D, 3, 3])"""
    n, D = q.shape
    R = torch.eye(3, device=q.device).expand(n, 3, 3)
    p = torch.zeros((n, 3), device=q.device)
    eye = torch.eye(3, device=q.device)
    o, z, r, tens = [], [], [], []
    for j in range(D):
        p = p + R @ frames[j, :, 3]
        R = R @ frames[j, :, :3]
        a = axes[j]
        o.append(p)
        z.append(R @ a)
        K = torch.stack([torch.stack([a.new_zeros(()), -a[2], a[1]]), torch.stack([a[2], a.new_zeros(()), -a[0]]),
                         torch.stack([-a[1], a[0], a.new_zeros(())])])
        c, s = torch.cos(q[:, j])[:, None, None], torch.sin(q[:, j])[:, None, None]
        R = R @ (c * eye + s * K + (1.0 - c) * torch.outer(a, a))
        b = bodies[j]
        L = torch.stack([torch.stack([b[4], b[5], b[6]]), torch.stack([b[5], b[7], b[8]]), torch.stack([b[6], b[8], b[9]])])
        r.append(R @ b[1:4])
        tens.append(R @ L @ R.transpose(1, 2))
    return torch.stack(o, 1), torch.stack(z, 1), torch.stack(r, 1), torch.stack(tens, 1)


def torch_pass(world, mass, v, a, g0):
    """recursive Newton-Euler -> tau [n, D]; ``v`` None: the terms in the angular velocity are left out"""
    o, z, r, tens = world
    n, D = a.shape
    w, dw, ao = torch.zeros_like(o[:, 0]), torch.zeros_like(o[:, 0]), g0.expand(n, 3)
    F, N = [], []
    for j in range(D):
        if j:
            d = o[:, j] - o[:, j - 1]
            ao = ao + cross(dw, d)
            if v is not None:
                ao = ao + cross(w, cross(w, d))
        dw = dw + z[:, j] * a[:, j, None]
        if v is not None:
            dw = dw + cross(w, z[:, j]) * v[:, j, None]
            w = w + z[:, j] * v[:, j, None]
        ac = ao + cross(dw, r[:, j])
        nj = (tens[:, j] @ dw[:, :, None])[:, :, 0]
        if v is not None:
            ac = ac + cross(w, cross(w, r[:, j]))
            nj = nj + cross(w, (tens[:, j] @ w[:, :, None])[:, :, 0])
        F.append(mass[j] * ac)
        N.append(nj)
    tau = [None] * D
    nn = f = None
    for j in range(D - 1, -1, -1):
        t = N[j] + cross(r[:, j], F[j])
        nn, f = (t, F[j]) if nn is None else (t + nn + cross(o[:, j + 1] - o[:, j], f), f + F[j])
        tau[j] = (z[:, j] * nn).sum(-1)
    return torch.stack(tau, 1)


def torch_dynamics(t, v, a, frames, axes, bodies, g0, inertia):
    N, T, D = t.shape
    q, v, a = t.reshape(-1, D), v.reshape(-1, D), a.reshape(-1, D)
    world = torch_world(q, frames, axes, bodies)
    tau = torch_pass(world, bodies[:, 0], v, a, g0).reshape(N, T, D)
    if not inertia:
        return None, tau
    zero, eye = torch.zeros_like(g0), torch.eye(D, device=q.device)
    cols = [torch_pass(world, bodies[:, 0], None, eye[j].expand_as(q), zero) for j in range(D)]
    M = torch.stack(cols, 2)
    M = torch.triu(M) + torch.triu(M, 1).transpose(1, 2)
    return M.reshape(N, T, D, D), tau


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
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_dynamics.json")) as f:
        chain = KinematicChain(json.load(f)["joints"])
    D, T = chain.n_dof, args.points
    (frames, axes), bodies = chain_matrices(chain, model.device), chain_bodies(chain, model.device)
    g0 = -torch.tensor(GRAVITY, dtype=torch.float32, device=model.device)
    lim = torch.as_tensor(chain.limits, dtype=torch.float32, device=model.device)
    line = {"config": label, "repeats": args.repeats, "T": T, "D": D, "torque": {}, "torque_and_inertia": {}}
    for N in args.rows:
        gen = torch.Generator("cuda").manual_seed(N)
        t = lim[:, 0] + (lim[:, 1] - lim[:, 0]) * torch.rand((N, T, D), device="cuda", generator=gen)
        v = 4.0 * torch.rand((N, T, D), device="cuda", generator=gen) - 2.0
        a = 20.0 * torch.rand((N, T, D), device="cuda", generator=gen) - 10.0
        for key, inertia in (("torque", False), ("torque_and_inertia", True)):
            lib = lambda: _motion_dynamics(model, t, v, a, frames, axes, bodies, GRAVITY, inertia=inertia, gravity_torque=False,
                                           coriolis=False)
            ref = lambda: torch_dynamics(t, v, a, frames, axes, bodies, g0, inertia)
            r = race(lib, ref, args.repeats, ("library", "torch"))
            (M_lib, _, _, tau_lib), (M_ref, tau_ref) = lib(), ref()
            r["torque_err"] = float(((tau_lib - tau_ref).abs() / (tau_ref.abs() + 1.0)).max())      # (two fp32 paths)
            if inertia:
                r["inertia_err"] = float(((M_lib - M_ref).abs() / (M_ref.abs() + 1.0)).max())
            r["points_per_s"] = round(N * T / (r["library_ms"] * 1e-3))
            line[key]["N%d" % N] = r
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
