#!/usr/bin/env python3
"""Cost of the sigma-lognormal calls (avae_lognormal_eval / _sample / _fit), device tensors in and out:
N strokes of C time-separated components at T = 100 points, N in {64, 4096}, C in {3, 8}, S in {10, 100} samples per stroke,
40 fit tries from a 10 % perturbation of the true parameters; hipEvent timing after a warm-up, the median of 7 repeats with the
candidates interleaved,

against the same definition written with torch: eval and sample as one broadcast [N, C, T] expression and ``cumsum`` in fp32
(the sampler's normals from ``torch.randn``), the fit as the same Levenberg-Marquardt with an fp32 Jacobian, ``J^T J`` and
``torch.linalg.cholesky`` in float64 and a host loop over the tries (every row takes every try: no statuses, no early stop).

One JSON line; --out FILE also writes it there."""
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
import bench
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder

T, DT = 100, 0.01


def separated(N, C, seed):
    """[N, C, 6] components separated in time (the generator of tests/lognormal_reference.py)"""
    rng = np.random.default_rng(seed)
    centre = ((np.arange(C) + 0.5) / C) * 0.8 + 0.08
    sigma = rng.uniform(0.15, 0.4, (N, C))
    width = rng.uniform(0.8, 1.3, (N, C)) * 0.9 / C
    mu = np.log(width / (np.exp(3.0 * sigma) - np.exp(-3.0 * sigma)))
    ths = rng.uniform(-3.0, 3.0, (N, C))
    return np.stack([rng.uniform(0.3, 1.5, (N, C)), centre - np.exp(mu - sigma * sigma), mu, sigma, ths,
                     ths + rng.uniform(-1.5, 1.5, (N, C))], axis=2).astype(np.float32)


def torch_components(p, t, jac):
    """p [N, C, 6], t [T] -> v [N, T, 2] (and JV [N, T, 2, 6 C])"""
    D, t0, mu, sigma, ths, the = (p[:, :, j:j + 1] for j in range(6))
    tau = t - t0
    sg = sigma.clamp_min(1e-6)
    on = tau >= 1e-6
    tc = tau.clamp_min(1e-6)
    z = (torch.log(tc) - mu) / sg
    u = torch.where(on, torch.exp(-0.5 * z * z) / (sg * math.sqrt(2 * math.pi) * (tc + 1e-5)), torch.zeros_like(z))
    amp = D * u
    a = amp.abs()
    E = torch.erf(z)
    q = the - ths
    phi = ths + 0.5 * q * (1 + E)
    sn, cs = torch.sin(phi), torch.cos(phi)
    v = torch.stack([(a * cs).sum(1), (a * sn).sum(1)], dim=2)
    if not jac:
        return v, None
    s = torch.sign(amp)
    sa = s * amp
    K = -(q / math.sqrt(math.pi)) * torch.exp(-z * z)
    H = 0.5 * (1 + E)
    zero = torch.zeros_like(z)
    da = [s * u, sa * (1 / (tc + 1e-5) + z / (sg * tc)), sa * z / sg, sa * (z * z - 1) / sg, zero, zero]
    dphi = [zero, K * torch.where(on, 1 / (sg * tc), zero), K / sg, K * z / sg, 1 - H, H]
    jx = torch.stack([da[j] * cs - a * sn * dphi[j] for j in range(6)], dim=2)          # [N, C, 6, T]
    jy = torch.stack([da[j] * sn + a * cs * dphi[j] for j in range(6)], dim=2)
    N, C = p.shape[0], p.shape[1]
    return v, torch.stack([jx.reshape(N, 6 * C, -1), jy.reshape(N, 6 * C, -1)], dim=1).permute(0, 3, 1, 2)


def torch_eval(p, start, t):
    v, _ = torch_components(p, t, False)
    return start[:, None, :] + DT * torch.cumsum(v, dim=1), v


def torch_sample(p, start, t, S, shift_mean=True):
    N, C = p.shape[0], p.shape[1]
    n = torch.randn((N, S, C, 3), device=p.device) / 3.0
    q = p[:, None].expand(N, S, C, 6).clone()
    D, ths, the = p[:, None, :, 0], p[:, None, :, 4], p[:, None, :, 5]
    q[..., 0] = D + n[..., 0] * 0.2 * D
    q[..., 4] = ths + n[..., 1] * (math.pi / 9)
    q[..., 5] = the + n[..., 1] * (math.pi / 9) + n[..., 2] * 0.1 * (the - ths)
    path = torch_eval(q.reshape(N * S, C, 6), start.repeat_interleave(S, 0), t)[0].reshape(N, S, -1, 2)
    return path - path.mean(dim=2, keepdim=True) if shift_mean else path


def torch_fit(target, init, start, t, n_iters, wp=1.0, wv=1e-3):
    N, C = init.shape[0], init.shape[1]
    P = 6 * C
    prev = torch.cat([start[:, None, :], target[:, :-1]], dim=1)
    V = (target - prev) / DT

    def loss_of(p, jac):
        v, JV = torch_components(p, t, jac)
        pos = start[:, None, :] + DT * torch.cumsum(v, dim=1)
        ep, ev = (pos - target).double(), (v - V).double()
        L = wp * (ep ** 2).sum((1, 2)) + wv * (ev ** 2).sum((1, 2))
        if not jac:
            return L, None, None
        A = (DT * torch.cumsum(JV, dim=1)).double().reshape(N, -1, P)
        B = JV.double().reshape(N, -1, P)
        M = wp * A.transpose(1, 2) @ A + wv * B.transpose(1, 2) @ B
        gr = wp * (A.transpose(1, 2) @ ep.reshape(N, -1, 1)) + wv * (B.transpose(1, 2) @ ev.reshape(N, -1, 1))
        return L, M, gr
    p = init.clone()
    lam = torch.full((N,), 1e-3, dtype=torch.float64, device=p.device)
    eye = torch.eye(P, dtype=torch.float64, device=p.device)
    for _ in range(n_iters):
        L, M, gr = loss_of(p, True)
        d = torch.diagonal(M, dim1=1, dim2=2)
        M = M + torch.diag_embed(lam[:, None] * d + 1e-12 * (d.amax(1, keepdim=True) + 1.0))
        Lc, info = torch.linalg.cholesky_ex(M)
        x = torch.cholesky_solve(gr, torch.where((info == 0)[:, None, None], Lc, eye))[:, :, 0]
        new = (p.reshape(N, P).double() - x).float().reshape(N, C, 6)
        new[:, :, 3] = new[:, :, 3].clamp(1e-3, 3.0)
        Ln = loss_of(new, False)[0]
        acc = (Ln < L) & (info == 0)
        p = torch.where(acc[:, None, None], new, p)
        lam = torch.where(acc, (lam / 3).clamp_min(1e-9), (4 * lam).clamp_max(1e9))
    return p, loss_of(p, False)[0]


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
    ap.add_argument("--components", type=int, nargs="*", default=[3, 8])
    ap.add_argument("--samples", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--fit-iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    t = torch.arange(T, device=model.device, dtype=torch.float32) * DT
    line = {"config": label, "points": T, "fit_iters": args.fit_iters, "repeats": args.repeats, "cases": {}}
    for N in args.rows:
        for C in args.components:
            true = torch.as_tensor(separated(N, C, N + C)).cuda()
            noise = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, (N, C, 6)).astype(np.float32)).cuda()
            init = (true * (1 + 0.1 * noise)).contiguous()
            start = torch.tensor([0.1, -0.2], device=model.device).expand(N, 2).contiguous()
            count = torch.full((N,), C, dtype=torch.int32, device=model.device)
            target = model.lognormal_eval(true, T, start=start, dt=DT)["path"]
            case = {}
            ref = torch_eval(true, start, t)[0]
            sub = race(lambda: model.lognormal_eval(true, T, start=start, dt=DT), lambda: torch_eval(true, start, t), args.repeats)
            sub["max_abs_diff"] = float((target - ref).abs().max())
            case["eval"] = sub
            for S in args.samples:
                case["sample_S%d" % S] = race(
                    lambda: model.lognormal_augment(params=true, count=count, n_samples=S, start=start, dt=DT, n_points=T),
                    lambda: torch_sample(true, start, t, S), args.repeats)
            res = model.lognormal_fit(target, init=init, count=count, start=start, dt=DT, n_iters=args.fit_iters, tol=0.0)
            ref_p, ref_loss = torch_fit(target, init, start, t, args.fit_iters)
            sub = race(lambda: model.lognormal_fit(target, init=init, count=count, start=start, dt=DT, n_iters=args.fit_iters, tol=0.0),
                       lambda: torch_fit(target, init, start, t, args.fit_iters), args.repeats)
            sub.update(rmse_median=float(res["rmse"].median()), rmse_max=float(res["rmse"].max()),
                       loss_median=float(res["loss"].median()), torch_loss_median=float(ref_loss.median()),
                       mean_iterations=round(float(res["iterations"].float().mean()), 2),
                       status_counts=[int((res["status"] == k).sum()) for k in range(4)])
            case["fit"] = sub
            line["cases"]["N%d_C%d" % (N, C)] = case
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
