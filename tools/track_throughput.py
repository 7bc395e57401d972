#!/usr/bin/env python3
"""Cost of the iLQR joint-trajectory synthesis (avae_motion_track), device tensors in and out: the 7-joint arm
of tests/golden/baxter_right_chain.json seeded at the writer's seed pose, N letter-like strokes of 100 points on the reference's
writing block, the first guess ``motion_ik``'s, N in {64, 4096}, 25 forced tries (``tol = 0``) at the default weights; hipEvent timing
after a warm-up, the median of 7 repeats with the candidates interleaved,

against the same definition written with torch in fp64: the chain walked with batched [N T, 3, 3] products, the Riccati recursion on
batched [N, 14, 14] matrices with dense A and B, ``torch.linalg.cholesky_ex`` and ``cholesky_solve`` on [N, 7, 7], a host loop over
the time points and the tries, every row taking every try (a rejected try is masked out).

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
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder, chain_matrices

D, T, DT, R_EFFORT = 7, 100, 0.01, 0.01
W = (10.0, 10.0, 50.0)


def letters(N, seed=0):
    """[N, T, 2] smooth strokes in plane units, scaled to span +-1.5"""
    rng = np.random.default_rng(seed)
    tau = np.linspace(0.0, 1.0, T)
    f, ph, amp = rng.uniform(0.5, 2.5, (N, 2, 3, 1)), rng.uniform(0, 2 * np.pi, (N, 2, 3, 1)), rng.uniform(0.2, 1.0, (N, 2, 3, 1))
    uv = (amp * np.sin(2 * np.pi * f * tau + ph)).sum(2).transpose(0, 2, 1)
    return 1.5 * uv / np.abs(uv).max(axis=(1, 2), keepdims=True)


def torch_walk(q, frames, axes):
    """[M, D] -> (p [M, 3], J_v [M, 3, D]) in q's dtype"""
    M = q.shape[0]
    eye = torch.eye(3, device=q.device, dtype=q.dtype)
    R, p = eye.expand(M, 3, 3), torch.zeros((M, 3), device=q.device, dtype=q.dtype)
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
    o, z = torch.stack(o, 1), torch.stack(z, 1)
    return p, torch.linalg.cross(z, p[:, None, :] - o).transpose(1, 2)


def torch_points(x, u, path, frames, axes, w, Se, linearise):
    """-> (J [N], l_q [N, T, D], l_qq [N, T, D, D])"""
    N = x.shape[0]
    p, Jv = torch_walk(x[:, :, :D].reshape(-1, D), frames, axes)
    e = p - path.reshape(-1, 3)
    c = ((w * e) ** 2).sum(1).reshape(N, T)
    c = c + torch.nn.functional.pad(torch.einsum("nti,ij,ntj->nt", u, Se, u), (0, 1))
    if not linearise:
        return c.sum(1), None, None
    JT = Jv.transpose(1, 2)
    lq = 2.0 * (JT @ (w * w * e)[:, :, None])[:, :, 0]
    lqq = 2.0 * (JT @ ((w * w)[:, None] * Jv))
    return c.sum(1), lq.reshape(N, T, D), lqq.reshape(N, T, D, D)


def torch_track(path, init, frames, axes, tries, lam0=1.0, factor=10.0, lam_min=1e-6):
    """[N, T, 3], [N, T, D] -> (trajectory [N, T, D], cost [N], accepted [N]) in fp64: ``tries`` tries for every row"""
    dev, f64 = path.device, torch.float64
    path, init, frames, axes = path.to(f64), init.to(f64), frames.to(f64), axes.to(f64)
    N = path.shape[0]
    dt = float(np.float32(DT))
    w = torch.tensor(W, device=dev, dtype=f64)
    Se = float(np.float32(R_EFFORT)) * torch.eye(D, device=dev, dtype=f64)
    A = torch.eye(2 * D, device=dev, dtype=f64)
    A[:D, D:] = dt * torch.eye(D, device=dev, dtype=f64)
    B = torch.zeros((2 * D, D), device=dev, dtype=f64)
    B[D:] = dt * torch.eye(D, device=dev, dtype=f64)
    eye = torch.eye(D, device=dev, dtype=f64)
    v0 = torch.zeros_like(init)
    v0[:, 1:] = (init[:, 1:] - init[:, :-1]) / dt
    u = (v0[:, 1:] - v0[:, :-1]) / dt

    def rollout_first(u):
        x = torch.zeros((N, T, 2 * D), device=dev, dtype=f64)
        x[:, 0, :D] = init[:, 0]
        for t in range(T - 1):
            x[:, t + 1, :D] = x[:, t, :D] + dt * x[:, t, D:]
            x[:, t + 1, D:] = x[:, t, D:] + dt * u[:, t]
        return x
    x = rollout_first(u)
    J, lq, lqq = torch_points(x, u, path, frames, axes, w, Se, True)
    lam = torch.full((N,), lam0, device=dev, dtype=f64)
    acc = torch.zeros((N,), device=dev, dtype=torch.int32)
    ks, Ks = torch.empty((N, T - 1, D), device=dev, dtype=f64), torch.empty((N, T - 1, D, 2 * D), device=dev, dtype=f64)
    for _ in range(tries):
        vx = torch.cat([lq[:, T - 1], torch.zeros((N, D), device=dev, dtype=f64)], 1)
        V = torch.zeros((N, 2 * D, 2 * D), device=dev, dtype=f64)
        V[:, :D, :D] = lqq[:, T - 1]
        ok = torch.ones((N,), device=dev, dtype=torch.bool)
        for t in range(T - 2, -1, -1):
            Qx = vx @ A
            Qx[:, :D] += lq[:, t]
            Qu = 2.0 * (u[:, t] @ Se) + vx @ B
            Qxx = A.T @ V @ A
            Qxx[:, :D, :D] += lqq[:, t]
            Qux = B.T @ V @ A
            Quu = 2.0 * Se + B.T @ V @ B + lam[:, None, None] * eye
            L, info = torch.linalg.cholesky_ex(Quu)
            ok &= info == 0
            sol = -torch.cholesky_solve(torch.cat([Qu[:, :, None], Qux], 2), L)
            k, K = sol[:, :, 0], sol[:, :, 1:]
            ks[:, t], Ks[:, t] = k, K
            KT = K.transpose(1, 2)
            vx = Qx + (KT @ (Quu @ k[:, :, None] + Qu[:, :, None]))[:, :, 0] + (Qux.transpose(1, 2) @ k[:, :, None])[:, :, 0]
            V = Qxx + KT @ (Quu @ K + Qux) + Qux.transpose(1, 2) @ K
            V = 0.5 * (V + V.transpose(1, 2))
        xn, un = torch.empty_like(x), torch.empty_like(u)
        xn[:, 0] = x[:, 0]
        for t in range(T - 1):
            un[:, t] = u[:, t] + ks[:, t] + (Ks[:, t] @ (xn[:, t] - x[:, t])[:, :, None])[:, :, 0]
            xn[:, t + 1, :D] = xn[:, t, :D] + dt * xn[:, t, D:]
            xn[:, t + 1, D:] = xn[:, t, D:] + dt * un[:, t]
        Jn, _, _ = torch_points(xn, un, path, frames, axes, w, Se, False)
        accept = ok & (Jn < J)
        x, u = torch.where(accept[:, None, None], xn, x), torch.where(accept[:, None, None], un, u)
        J = torch.where(accept, Jn, J)
        lam = torch.where(accept, torch.clamp(lam / factor, min=lam_min), lam * factor)
        acc += accept.to(torch.int32)
        J, lq, lqq = torch_points(x, u, path, frames, axes, w, Se, True)
    return x[:, :, :D], J, acc


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
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--tries", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    with open(os.path.join(ROOT, "tests", "golden", "baxter_right_chain.json")) as f:
        fx = json.load(f)
    chain, canvas = KinematicChain(fx["joints"]), StrokeCanvas()
    frames, axes = chain_matrices(chain, model.device)
    seed_pos = np.asarray(fx["seed_pos"])
    line = {"config": label, "chain": "baxter right arm, 7 joints", "points": T, "tries": args.tries, "repeats": args.repeats,
            "cases": {}}
    for N in args.rows:
        path = torch.as_tensor(canvas.lift(letters(N, N), fx["block_center"]).astype(np.float32)).cuda()
        seed = torch.as_tensor(np.tile(seed_pos.astype(np.float32), (N, 1))).cuda()
        init = model.motion_ik(path, chain, seed, orientation="seed")["trajectory"]

        def lib():
            return model.motion_track(path, chain, init=init, n_iters=args.tries, tol=0.0)
        res = lib()
        ref_traj, ref_cost, ref_acc = torch_track(path, init, frames, axes, args.tries)
        sub = race(lib, lambda: torch_track(path, init, frames, axes, args.tries), args.repeats)
        same = res["accepted"] == ref_acc
        sub.update(mean_iterations=round(float(res["iterations"].float().mean()), 3),
                   mean_accepted=round(float(res["accepted"].float().mean()), 3), same_decisions=float(same.float().mean()),
                   max_abs_diff_same_rows=float((res["trajectory"].double() - ref_traj)[same].abs().max()) if bool(same.any()) else None,
                   cost0_mean=float(res["cost0"].mean()), cost_mean=float(res["cost"].mean()), torch_cost_mean=float(ref_cost.mean()),
                   track_rmse_max=float(res["track_rmse"].max()), status_counts=torch.bincount(res["status"].long(), minlength=4).tolist(),
                   rows_per_s=float("%.3g" % (N / (sub["library_ms"] * 1e-3))))
        line["cases"]["N%d" % N] = sub
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
