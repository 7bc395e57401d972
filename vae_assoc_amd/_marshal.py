"""Turning the caller's arrays into what the C ABI of include/avae.h takes: float32 device tensors with unit column stride,
``c_void_p[M]`` pointers, ``c_int32[M]`` leading dimensions, uint8 presence bytes and dense eps blocks.

Every entry point of ``vae_assoc.AssocVariationalAutoEncoder`` marshals through these functions.  They take the device and the
widths as arguments and touch neither a model nor the library, so they run on CPU tensors (``device="cpu"``) in the tests."""
import ctypes as C

import numpy as np
import torch


def ptr(t):
    """Device pointer of an optional tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def ld_of(t):
    """Leading dimension of a [rows, cols] tensor for the library: its row stride, or the width where there is no second row
    (the stride of a single row is arbitrary)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def dev_array(a, cols, device):
    """-> (float32 tensor [rows, cols] on ``device`` with unit column stride, was_numpy).  A view whose rows do not overlap (a
    column slice of a wider matrix) passes through without a copy."""
    was_np = not torch.is_tensor(a)
    t = torch.as_tensor(np.asarray(a, dtype=np.float32) if was_np else a)
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("expected a [rows, %d] array, got %s" % (cols, tuple(t.shape)))
    t = t.to(device=device, dtype=torch.float32)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < cols):
        t = t.contiguous()
    return t, was_np


def dev_modalities(X, widths, device, rows=None, what=None, allow_none=False):
    """X, one [rows, widths[m]] array or tensor per modality -> (tensors, rows, was_numpy, ptrs, lds).

    ``rows`` is the row count every modality needs and ``what`` the words that name it in the error; without it the first given
    modality sets it.  ``allow_none``: ``X[m] = None`` is a modality without a source -> None in ``tensors``, a NULL pointer and
    ld 0 (otherwise None is refused like any other non-array).  ``was_numpy`` is that of the first given modality, ``rows`` and
    ``was_numpy`` are None when nothing was given."""
    M = len(widths)
    if len(X) != M:
        raise ValueError("expected a list of %d modalities, got %d" % (M, len(X)))
    ts, ptrs, lds, was_np, first = [], [], [], None, None
    for m, (x, cols) in enumerate(zip(X, widths)):
        if x is None and allow_none:
            ts.append(None)
            ptrs.append(None)
            lds.append(0)
            continue
        t, np_in = dev_array(x, cols, device)
        if was_np is None:
            was_np = np_in
        if rows is None:
            rows, first = t.shape[0], m
        elif t.shape[0] != rows:
            raise ValueError("modality %d: expected %d rows (%s), got %d"
                             % (m, rows, what if first is None else "as modality %d" % first, t.shape[0]))
        ts.append(t)
        ptrs.append(t.data_ptr())
        lds.append(ld_of(t))
    return ts, rows, was_np, (C.c_void_p * M)(*ptrs), (C.c_int32 * M)(*lds)


def dev_inputs(inputs, ts, widths, device, rows, what=None):
    """Explicit encoder inputs of the denoising calls: a list like ``X`` whose entries may be None (no explicit input for that
    modality), marshalled exactly as ``X`` is -> (tensors, ptrs, lds).  ``ts`` are ``X``'s tensors: an input for a modality whose
    ``X[m]`` is None has no target and is refused."""
    its, _, _, ptrs, lds = dev_modalities(inputs, widths, device, rows, what, allow_none=True)
    for m, (t, x) in enumerate(zip(its, ts)):
        if t is not None and x is None:
            raise ValueError("inputs[%d] is given while X[%d] is None: an encoder input needs its target" % (m, m))
    return its, ptrs, lds


def corruption_fields(drop, noise, drop_value, n_mod):
    """The arguments of ``set_corruption`` -> (drop_prob, noise_std, drop_value), three lists of ``n_mod`` floats.  Each argument
    is a scalar (every modality) or a list with one value per modality; ``drop=None`` is off (all zeros).  The ranges are
    avae_set_corruption's, checked here so that a bad value raises ``ValueError`` ahead of the library."""
    if drop is None:
        return [0.0] * n_mod, [0.0] * n_mod, [0.0] * n_mod

    def per_mod(v, name):
        vs = [v] * n_mod if np.isscalar(v) else list(v)
        if len(vs) != n_mod:
            raise ValueError("%s must be a scalar or a list of %d values, got %d" % (name, n_mod, len(vs)))
        return [float(np.float32(x)) for x in vs]
    p, s, d = per_mod(drop, "drop"), per_mod(noise, "noise"), per_mod(drop_value, "drop_value")
    for m in range(n_mod):
        if not 0.0 <= p[m] < 1.0:
            raise ValueError("drop[%d] (drop_prob) must be in [0, 1), got %r" % (m, p[m]))
        if not (np.isfinite(s[m]) and s[m] >= 0.0):
            raise ValueError("noise[%d] (noise_std) must be finite and >= 0, got %r" % (m, s[m]))
        if not np.isfinite(d[m]):
            raise ValueError("drop_value[%d] must be finite, got %r" % (m, d[m]))
    return p, s, d


def grad_clip_fields(max_norm, skip_nonfinite):
    """The arguments of ``set_grad_clip`` -> (max_norm as a float32-exact float, skip_nonfinite as 0 / 1).  ``max_norm`` None is 0
    (no clipping), ``float('inf')`` monitors only.  The range is avae_set_grad_clip's, checked here so that a bad value raises
    ``ValueError`` ahead of the library."""
    mx = 0.0 if max_norm is None else max_norm
    if isinstance(mx, (bool, np.bool_)) or not isinstance(mx, (int, float, np.integer, np.floating)):
        raise ValueError("max_norm must be a number >= 0 (0 = off, inf = monitor only), got %r" % (max_norm,))
    mx = float(np.float32(mx))
    if not mx >= 0.0:
        raise ValueError("max_norm must be >= 0 and not NaN (0 = off, inf = monitor only), got %r" % (max_norm,))
    return mx, 1 if skip_nonfinite else 0


def grad_clip_kwargs(grad_clip):
    """The ``grad_clip=`` keyword of the constructor and of ``train`` -> the keyword arguments of ``set_grad_clip``: None (off),
    a number (``max_norm``), or a dict with the keys ``max_norm`` and / or ``skip_nonfinite``."""
    if grad_clip is None:
        return {}
    if isinstance(grad_clip, dict):
        extra = set(grad_clip) - {"max_norm", "skip_nonfinite"}
        if extra:
            raise ValueError("grad_clip: unknown key(s) %s (max_norm, skip_nonfinite)" % ", ".join(sorted(map(str, extra))))
        kw = dict(grad_clip)
    else:
        kw = {"max_norm": grad_clip}
    grad_clip_fields(kw.get("max_norm", 0.0), kw.get("skip_nonfinite", False))
    return kw


def dev_row_args(X, widths, device, present=None):
    """Arguments of the row calls (any row count) -> (tensors, N, was_numpy, ptrs, lds, presence or None).  Unmasked, the first
    modality gives N.  Masked, ``present`` [N, M] does, ``X[m] = None`` is a modality absent on every row, and was_numpy is
    ``present``'s when every modality is None."""
    if present is None:
        return dev_modalities(X, widths, device) + (None,)
    p = dev_flags(present, len(widths), device)
    rows = int(p.shape[0])
    ts, _, was_np, ptrs, lds = dev_modalities(X, widths, device, rows, "present has %d" % rows, allow_none=True)
    return ts, rows, (not torch.is_tensor(present)) if was_np is None else was_np, ptrs, lds, p


def dev_flags(a, cols, device, rows=None, what=None, name="present"):
    """Presence / observation flags (bool or integer or float, array or tensor, any device; nonzero = set) -> contiguous uint8
    tensor [rows, cols] of ``a != 0`` on ``device``.  ``rows`` None accepts any row count; ``what`` names it in the error."""
    p = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    if p.dim() != 2 or p.shape[1] != cols or (rows is not None and p.shape[0] != rows):
        want = "rows" if rows is None else ("%d" % rows if what is None else "%d (%s)" % (rows, what))
        raise ValueError("%s must be [%s, %d], got %s" % (name, want, cols, tuple(p.shape)))
    return (p != 0).to(device=device, dtype=torch.uint8).contiguous()


def dev_dense(a, cols, device, rows=None, what=None, name="eps"):
    """Optional [rows, cols] block the library reads densely (eps, z) -> contiguous float32 tensor on ``device``, None -> None.
    ``rows`` None accepts any row count; ``what`` names it in the error."""
    if a is None:
        return None
    t, _ = dev_array(a, cols, device)
    if rows is not None and t.shape[0] != rows:
        raise ValueError("%s must be [%s, %d], got %s" % (name, "%d" % rows if what is None else "%d (%s)" % (rows, what), cols,
                                                         tuple(t.shape)))
    return t.contiguous()


def dev_dense3(a, shape, device, name="eps"):
    """Optional block of exactly ``shape`` (the [rows, K, n_z] eps of the log-likelihoods) -> contiguous float32 tensor."""
    if a is None:
        return None
    t = torch.as_tensor(a if torch.is_tensor(a) else np.asarray(a, dtype=np.float32))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be [%s], got %s" % (name, ", ".join("%d" % s for s in shape), tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous()
