"""fp64 statement of one training step with every training option set at once (include/avae.h: presence masks, avae_set_corruption,
avae_set_schedule, avae_set_grad_clip, avae_set_ema), composed from the references each option already has:

    x~       = denoise_reference.corrupt(x, seed, step counter before the step, modality)       (or the caller's ``X_in``)
    cost, g  = denoise_reference.denoise_cost_and_grads(..., present=P, assoc_lambda=lambda_t)
    c        = clip_reference.clip_factor(clip_reference.global_norm(g), max_norm)
    theta'   = the oracle's adam_step(theta, m, v, g * c, t, lr_eff_t)
    e'       = ema_reference.ema_step(e, theta', decay, warmup, t)

with t = the step's number (the counter after it), lambda_t = fl32(assoc_lambda * a_t) and lr_eff_t = fl32(learning_rate * l_t) of
schedule_reference.hyper.  There is no separate KL weight here (the oracle's backward folds KL and reconstruction under one weight):
the KL multiplier is schedule_reference.scheduled_cost's.  With an option off its stage is skipped, not run with a neutral value, so
the composition reduces exactly to the reference of whatever is left (tests/test_big_options_cpu.py)."""
import numpy as np

from clip_reference import clip_factor, global_norm
from conftest import make_arch
from denoise_reference import corrupt, denoise_cost_and_grads
from ema_reference import ema_step
from oracle import vae_assoc_oracle as O
from schedule_reference import hyper

# Net R of tests/test_gpu_big_options.py, the smallest shapes on the big nets' plan: tests/test_gpu_masked.py's BIG widths, n_z = 37
# (2 n_z > 64: the heads' 64x128 tiles; 37 % 4 != 0: the padded eps rows), B = 2817 = 11 * 256 + 1 (the first batch at which the loss
# launch takes the 8-wave 256x64 tiles, its last tile holding one live row)
NET_R = dict(archs=[make_arch("a", 784, 0, 0, 37, n_hidden=[64, 48]), make_arch("b", 147, 0, 0, 37, n_hidden=[64, 48])],
             binary=[True, False], weights=[5.0, 1.0], lam=0.5, B=2817)


def corrupted_inputs(X, seed, step, drop, noise, drop_value):
    """x~ of every modality at step counter ``step`` (the number of steps taken before), float64; X[m] None stays None"""
    per = lambda v, m: v[m] if isinstance(v, (list, tuple)) else v
    return [None if x is None else corrupt(x, seed, step, m, per(drop, m), per(noise, m), per(drop_value, m))[0]
            for m, x in enumerate(X)]


def composed_step(archs, theta, m, v, t, X, eps, binary, weights, lam, act, lr, present=None, X_in=None, corruption=None,
                  assoc=None, lr_schedule=None, max_norm=0.0, ema=None, quant=None, masks=None):
    """One step from (theta, m, v) and step counter ``t`` (steps taken so far) -> dict(cost, g (raw), norm, c, lambda_t, lr_t,
    theta, m, v, t, X_in, ema).  ``corruption``: dict(seed=, drop=, noise=, drop_value=) for the on-device draw, or ``X_in`` given
    directly; ``assoc`` / ``lr_schedule``: schedule specs (schedule_reference.schedule_value); ``ema``: dict(e=, decay=, warmup=)."""
    t1 = int(t) + 1
    if X_in is None:
        X_in = X if corruption is None else corrupted_inputs(X, corruption["seed"], int(t), corruption.get("drop", 0.0),
                                                             corruption.get("noise", 0.0), corruption.get("drop_value", 0.0))
    lam_t, lr_t = lam, lr
    if assoc is not None or lr_schedule is not None:
        _, l32, r32 = hyper(None, assoc, lr_schedule, lam, lr, t1)
        lam_t = float(l32) if assoc is not None else lam
        lr_t = float(r32) if lr_schedule is not None else lr
    cost, g = denoise_cost_and_grads(archs, theta, X, X_in, eps, binary, weights, lam_t, act, present=present, quant=quant, masks=masks)
    norm = global_norm(g)
    c = clip_factor(norm, float(max_norm))
    gc = g if c == 1.0 else g * c
    th1, m1, v1 = O.adam_step(np.asarray(theta, np.float64), np.asarray(m, np.float64), np.asarray(v, np.float64), gc, t1, lr_t)
    e1 = None if ema is None else ema_step(ema["e"], th1, ema["decay"], ema.get("warmup", False), t1)
    return dict(cost=cost, g=g, norm=norm, c=c, lambda_t=lam_t, lr_t=lr_t, theta=th1, m=m1, v=v1, t=t1, X_in=X_in, ema=e1)


def wrong_buffer_margin(archs, theta, X, X_in, eps, binary, weights, lam, act, present=None):
    """(true cost, the cost a step would report that charged its losses against the encoder's rows ``X_in`` instead of ``X``):
    a denoising test can only see that mistake if the two differ by far more than its cost tolerance"""
    true, _ = denoise_cost_and_grads(archs, theta, X, X_in, eps, binary, weights, lam, act, present=present)
    wrong, _ = denoise_cost_and_grads(archs, theta, X_in, X_in, eps, binary, weights, lam, act, present=present)
    return true, wrong
