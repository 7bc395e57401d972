"""Statement of parameter averaging (include/avae.h, avae_set_ema): TF-1's
``tf.train.ExponentialMovingAverage(decay[, num_updates])``,

    e <- e + (theta - e) * (1 - d_t),    d_t = min(decay, (1 + t) / (10 + t)) with warm-up, else decay

with t the number of the step whose update produced theta (1 for the first step of a fresh model).

``decay_t`` / ``one_minus_decay`` mirror the kernel's fp32 expression operation for operation in NumPy float32 (every operand and
every result a float32: IEEE add, divide and minimum round as the device's), so they give the kernel's bits.  ``ema_step`` is the
update in fp64 on that fp32 factor: what the kernel's difference and fused multiply-add round, twice."""
import numpy as np

F32 = np.float32


def decay_t(decay, warmup, step):
    """d_t as k_adam forms it: n = (float)step;  warmup ? fminf(decay, (1.0f + n) / (10.0f + n)) : decay"""
    d, n = F32(decay), F32(int(step))
    if not warmup:
        return d
    return min(d, (F32(1.0) + n) / (F32(10.0) + n))


def one_minus_decay(decay, warmup, step):
    """the factor of the update, 1.0f - d_t, as float32"""
    return F32(1.0) - decay_t(decay, warmup, step)


def ema_step(e, theta, decay, warmup, step):
    """fp64: the average after the update of step ``step`` moved the parameters to ``theta``"""
    e, theta = np.asarray(e, np.float64), np.asarray(theta, np.float64)
    return e + (theta - e) * float(one_minus_decay(decay, warmup, step))


def ema_run(e0, thetas, decay, warmup, first_step=1):
    """fp64: ``ema_step`` over consecutive steps first_step, first_step + 1, ..."""
    e = np.asarray(e0, np.float64)
    for i, th in enumerate(thetas):
        e = ema_step(e, th, decay, warmup, first_step + i)
    return e
