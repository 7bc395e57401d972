"""fp64 statement of global-norm gradient clipping and non-finite step skipping (include/avae.h, avae_set_grad_clip): the
oracle's ``cost_and_grads`` -> norm -> factor -> ``apply_gradients``.

    s = sum g^2;  norm = sqrt(s);  c = max_norm / norm if (max_norm > 0 and norm > max_norm) else 1;  Adam consumes g * c
    s not finite and skip_nonfinite: theta, m, v stay, the step counter still advances

The library forms s, norm and c in fp32 in a fixed order; this reference forms them in fp64, so a comparison of parameters goes
through the device's own recorded norm (tests/test_gpu_clip.py) while costs compare directly."""
import numpy as np


def global_norm(g):
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.sum(g * g)))


def clip_factor(norm, max_norm):
    """A select, not a min: NaN compares false and leaves c = 1; max_norm = inf never clips."""
    return max_norm / norm if (max_norm > 0.0 and norm > max_norm) else 1.0


def clipped_step(ref, X, eps, max_norm=0.0, skip_nonfinite=False, masks=None):
    """One step of oracle ``ref`` (an ``OracleAssocVAE``) with clipping -> dict(cost, g (raw), norm, c, gc (what Adam consumed, or
    None), skipped)."""
    with np.errstate(over="ignore", invalid="ignore"):
        cost, g, _ = ref.cost_and_grads(X, eps, masks=masks)
    norm = global_norm(g)
    if skip_nonfinite and not np.isfinite(norm * norm):
        ref.t += 1                      # a skipped step still consumes its step number
        return dict(cost=float(cost), g=g, norm=norm, c=1.0, gc=None, skipped=True)
    c = clip_factor(norm, float(max_norm))
    gc = g if c == 1.0 else g * c
    ref.apply_gradients(gc)
    return dict(cost=float(cost), g=g, norm=norm, c=c, gc=gc, skipped=False)
