#!/usr/bin/env python3
"""Cost of letter thumbnails (avae_letter_thumbnail), device tensors in and out: grey 480 x 640 frames at
N in {1, 64, 4096}, RGBA 480 x 640 frames at N in {1, 64, 1024} and one grey 2048 x 2048 frame, each in the camera mode (threshold
108, inverted) and the drawing-pad mode (inverted), dark letters on white whose box is about a quarter of the frame; hipEvent
timing after a warm-up, the median of 7 repeats with the candidates interleaved,

against the same definition composed with torch: the grey formula in int32, ``any`` over rows and columns and ``argmax`` for the
box, ONE host read of the boxes, then per frame the two weight matrices and ``wy @ crop @ wx^T`` in float64 (exact: every partial
sum is an integer below 2^53).

Per case: both times and their ratio, whether the two pictures agree bit by bit, the two kernels' own device times from
avae_timing_report, and the bytes of frame data per second of k_ink_box (the whole frame is read once) against the 6.3 TB/s the
HBM of an MI355X sustains.  One JSON line; --out FILE also writes it there."""
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
from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder

HBM_BYTES_PER_S = 6.3e12
MODES = {"camera": dict(threshold=108, invert=True), "canvas": dict(invert=True)}


def letters(N, Hf, Wf, Cn, seed):
    """dark ink (values 0 .. 99, 30 % of the pixels) inside a box of Hf / 2 x Wf / 2 somewhere in each white frame, made on the device"""
    gen = torch.Generator("cuda").manual_seed(seed)
    f = torch.full((N, Hf, Wf, Cn), 255, dtype=torch.uint8, device="cuda")
    h, w = Hf // 2, Wf // 2
    ys = torch.randint(0, Hf - h + 1, (N,), generator=gen, device="cuda").tolist()
    xs = torch.randint(0, Wf - w + 1, (N,), generator=gen, device="cuda").tolist()
    for n in range(N):
        ink = torch.randint(0, 100, (h, w, 1), generator=gen, device="cuda", dtype=torch.uint8)
        keep = torch.rand((h, w, 1), generator=gen, device="cuda") < 0.3
        f[n, ys[n]:ys[n] + h, xs[n]:xs[n] + w, :min(Cn, 3)] = torch.where(keep, ink, torch.full_like(ink, 255))
    if Cn == 4:
        f[..., 3] = torch.randint(0, 256, (N, Hf, Wf), generator=gen, device="cuda", dtype=torch.uint8)
    return f


def axis_weights(S, size, k0, n, device):
    """wx(j, k) for k0 <= k < k0 + n -> float64 [size, n]"""
    k = torch.arange(k0, k0 + n, device=device, dtype=torch.int64)[None, :]
    j = torch.arange(size, device=device, dtype=torch.int64)[:, None]
    return (torch.minimum((j + 1) * S, (k + 1) * size) - torch.maximum(j * S, k * size)).clamp_(min=0).to(torch.float64)


def torch_thumbnails(frames, size, threshold=None, invert=False):
    N, Hf, Wf, Cn = frames.shape
    if Cn == 1:
        v = frames[..., 0].to(torch.int32)
    else:
        c = frames.to(torch.int32)
        v = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    if threshold is not None:
        v = (v > threshold).to(torch.int32) * 255
    gv = 255 - v if invert else v
    mask = gv != 0
    rows, cols = mask.any(2), mask.any(1)
    first = torch.stack([cols.int().argmax(1), rows.int().argmax(1), Wf - 1 - cols.flip(1).int().argmax(1),
                         Hf - 1 - rows.flip(1).int().argmax(1), rows.any(1).int()], 1).cpu().numpy()          # the one host read
    image = torch.zeros((N, size * size), dtype=torch.float32, device=frames.device)
    for n in range(N):
        x0, y0, x1, y1, any_ink = (int(t) for t in first[n])
        if not any_ink:
            continue
        w, h = x1 - x0 + 1, y1 - y0 + 1
        L = max(w, h)
        b = 3 * L // 5
        S = L + b
        oy, ox = b // 2 + (L - h) // 2, b // 2 + (L - w) // 2
        crop = gv[n, y0:y0 + h, x0:x0 + w].to(torch.float64)
        sums = axis_weights(S, size, oy, h, frames.device) @ crop @ axis_weights(S, size, ox, w, frames.device).T
        image[n] = (sums / float(255 * S * S)).to(torch.float32).reshape(-1)
    return image


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


def launch_times(model, fn):
    L, h = model._L, model._h
    L.avae_timing_enable(h, 1)
    for _ in range(5):
        fn()
    buf = C.create_string_buffer(1 << 16)
    L.avae_timing_report(h, buf, len(buf))
    L.avae_timing_enable(h, 0)
    return {nm: {"calls": int(c), "avg_us": round(float(a) * 1e3, 2), "min_us": round(float(mn) * 1e3, 2)}
            for nm, c, a, mn in (ln.split() for ln in buf.value.decode().splitlines()) if nm in ("ink_box", "thumbnail")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["grey:480:640:1", "grey:480:640:64", "grey:480:640:4096", "rgba:480:640:1",
                                                   "rgba:480:640:64", "rgba:480:640:1024", "grey:2048:2048:1"],
                    help="format:Hf:Wf:N with format grey or rgba")
    ap.add_argument("--size", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    archs, B, dtype, label = bench.CONFIGS["c2"]
    model = AssocVariationalAutoEncoder(archs, transfer_fct="relu", batch_size=B, compute_dtype=dtype, seed=0, **bench.HYPER)
    line = {"size": args.size, "repeats": args.repeats, "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}
    for spec in args.cases:
        fmt, Hf, Wf, N = spec.split(":")
        Hf, Wf, N, Cn = int(Hf), int(Wf), int(N), 1 if fmt == "grey" else 4
        frames = letters(N, Hf, Wf, Cn, seed=N + Hf)
        case = {"frame_bytes": N * Hf * Wf * Cn}
        for name, mode in MODES.items():
            lib = lambda: model.letter_thumbnails(frames, size=args.size, **mode)      # noqa: E731
            ref = lambda: torch_thumbnails(frames, args.size, **mode)                   # noqa: E731
            sub = race(lib, ref, args.repeats)
            out = lib()
            sub["bitwise_equal"] = bool(torch.equal(out["image"].view(torch.int32), ref().view(torch.int32)))
            sub["mean_box"] = [round(float(t), 1) for t in out["box"][:, 2:].float().mean(0)]
            sub["launches"] = launch_times(model, lib)
            if "ink_box" in sub["launches"]:
                rate = case["frame_bytes"] / (sub["launches"]["ink_box"]["avg_us"] * 1e-6)
                sub["ink_box_bytes_per_s"] = float("%.3g" % rate)
                sub["ink_box_share_of_hbm"] = round(rate / HBM_BYTES_PER_S, 3)
            case[name] = sub
        line["cases"][spec] = case
        del frames
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
