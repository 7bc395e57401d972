"""Turning the caller's arrays into what the C ABI of include/avae.h takes: float32 device tensors with unit column stride,
``c_void_p[M]`` pointers, ``c_int32[M]`` leading dimensions, uint8 presence bytes and dense eps blocks.

Every entry point of ``vae_assoc.AssocVariationalAutoEncoder`` marshals through these functions.  They take the device and the
widths as arguments and touch neither a model nor the library, so they run on CPU tensors (``device="cpu"``) in the tests.

Next to the arrays stand the checks of one scalar that every validator words alike (``as_int``, ``as_index``, ``need_type``) and
the fields of the training options (corruption, clipping, averaging, schedules).  The validators of the entry points themselves
are in ``_args``.  This module imports nothing from the package but ``_capi``, and that only inside ``schedule_struct``."""
import ctypes as C

import numpy as np
import torch


def as_int(v, name, lo, hi=None):
    """A whole number in [lo, hi] (``hi`` None: no upper end) -> int.  ``bool`` and ``np.bool_`` are no numbers here."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError("%s must be an integer %s, got %r" % (name, ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi), v))
    return int(v)


def as_index(v, name, n):
    """An index into a list of ``n`` entries -> int"""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v < n:
        raise ValueError("%s must be an index in [0, %d), got %r" % (name, n, v))
    return int(v)


def need_type(obj, cls, name):
    if not isinstance(obj, cls):
        raise ValueError("%s must be a %s, got %r" % (name, cls.__name__, type(obj).__name__))


def to_device32(a, device):
    """Host array -> contiguous float32 tensor on ``device``"""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def ptr(t):
    """Device pointer of an optional tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def ld_of(t):
    """Leading dimension of a [rows, cols] tensor for the library: its row stride, or the width where there is no second row
    (the stride of a single row is arbitrary)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def row_chunks(N, chunk):
    """Rows [0, N) in chunks of at most ``chunk`` rows (at least 1) -> (r0, n, at) per chunk, in order: ``at(t)`` is the data
    pointer of rows r0 .. r0 + n of the tensor ``t``, None (NULL) for None.  ``N == 0`` yields nothing."""
    chunk = max(1, int(chunk))
    for r0 in range(0, N, chunk):
        n = min(chunk, N - r0)
        yield r0, n, lambda t, r0=r0, n=n: None if t is None else t[r0:r0 + n].data_ptr()


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


def ema_fields(decay, warmup=False):
    """The arguments of ``set_ema`` -> (decay as a float32-exact float, warmup as 0 / 1).  ``decay`` None or 0 switches averaging
    off.  The range is avae_set_ema's, checked here so that a bad value raises ``ValueError`` ahead of the library: the decay the
    kernel uses is the float32 value, so one that rounds to 1.0 is refused as well."""
    d = 0.0 if decay is None else decay
    if isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, float, np.integer, np.floating)):
        raise ValueError("decay must be a number in (0, 1) (None or 0 = off), got %r" % (decay,))
    d = float(np.float32(d))
    if not 0.0 <= d < 1.0:
        raise ValueError("decay must be in (0, 1) as float32 and not NaN (None or 0 = off), got %r" % (decay,))
    if not isinstance(warmup, (bool, np.bool_)) and warmup not in (0, 1):
        raise ValueError("warmup must be True or False, got %r" % (warmup,))
    return d, 1 if warmup else 0


def ema_kwargs(ema):
    """The ``ema=`` keyword of the constructor and of ``train`` -> the keyword arguments of ``set_ema``: None (off), a number
    (``decay``), or a dict with the keys ``decay`` and / or ``warmup``."""
    if ema is None:
        return {}
    if isinstance(ema, dict):
        extra = set(ema) - {"decay", "warmup"}
        if extra:
            raise ValueError("ema: unknown key(s) %s (decay, warmup)" % ", ".join(sorted(map(str, extra))))
        if "decay" not in ema:
            raise ValueError("ema: the dict needs a decay (decay, warmup)")
        kw = dict(ema)
    else:
        kw = {"decay": ema}
    ema_fields(kw["decay"], kw.get("warmup", False))
    return kw


SCHEDULE_NAMES = ("kl", "assoc", "lr")


def _is_number(x):
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))


def _whole(x, name):
    """A step count given as an int, or as a float that holds one."""
    if not _is_number(x) or not np.isfinite(x) or float(x) != int(x):
        raise ValueError("%s must be a whole number of steps, got %r" % (name, x))
    return int(x)


def schedule_spec(spec, name="schedule"):
    """One argument of ``set_schedule`` -> None (off), or a checked dict in one of the two canonical forms
    ``dict(knots=[(step, value), ...], period=int)`` / ``dict(decay_rate=, decay_steps=, staircase=)``.  A number is the constant
    multiplier (one knot).  The ranges are avae_set_schedule's, checked here so that a bad value raises ``ValueError`` -- naming
    the schedule and the field -- ahead of the library."""
    if spec is None:
        return None
    if _is_number(spec):
        spec = dict(knots=[(0, spec)])
    if not isinstance(spec, dict):
        raise ValueError("%s must be None, a number, dict(knots=, period=) or dict(decay_rate=, decay_steps=, staircase=), got %r"
                         % (name, spec))
    if "knots" in spec:
        extra = set(spec) - {"knots", "period"}
        if extra:
            raise ValueError("%s: unknown key(s) %s (knots, period)" % (name, ", ".join(sorted(map(str, extra)))))
        knots = list(spec["knots"])
        if not 1 <= len(knots) <= 8:
            raise ValueError("%s: knots (n_knots) must hold 1 to 8 (step, value) pairs, got %d" % (name, len(knots)))
        out, prev = [], -1
        for i, kv in enumerate(knots):
            if len(kv) != 2:
                raise ValueError("%s: knots[%d] must be a (step, value) pair, got %r" % (name, i, kv))
            st = _whole(kv[0], "%s: knots[%d] step (knot_step)" % (name, i))
            if st <= prev:
                raise ValueError("%s: knots[%d] step (knot_step) = %d must be %s" % (name, i, st, ">= 0" if i == 0 else
                                                                                     "above the previous knot's (strictly increasing)"))
            if not _is_number(kv[1]) or not (np.isfinite(kv[1]) and float(np.float32(kv[1])) >= 0.0 and np.isfinite(np.float32(kv[1]))):
                raise ValueError("%s: knots[%d] value (knot_value) must be finite and >= 0, got %r" % (name, i, kv[1]))
            out.append((st, float(np.float32(kv[1]))))
            prev = st
        period = spec.get("period")
        period = 0 if period is None else _whole(period, "%s: period" % name)
        if period < 0:
            raise ValueError("%s: period must be >= 0, got %d" % (name, period))
        if period > 0 and out[-1][0] >= period:
            raise ValueError("%s: the last knot's step (knot_step) = %d must be below period = %d" % (name, out[-1][0], period))
        return dict(knots=out, period=period)
    if "decay_rate" in spec or "decay_steps" in spec:
        extra = set(spec) - {"decay_rate", "decay_steps", "staircase"}
        if extra:
            raise ValueError("%s: unknown key(s) %s (decay_rate, decay_steps, staircase)" % (name, ", ".join(sorted(map(str, extra)))))
        rate, steps = spec.get("decay_rate"), spec.get("decay_steps")
        if not _is_number(rate) or not (np.isfinite(np.float32(rate)) and float(np.float32(rate)) > 0.0):
            raise ValueError("%s: decay_rate must be finite and > 0, got %r" % (name, rate))
        steps = _whole(steps, "%s: decay_steps" % name)
        if steps <= 0:
            raise ValueError("%s: decay_steps must be > 0, got %d" % (name, steps))
        return dict(decay_rate=float(np.float32(rate)), decay_steps=steps, staircase=bool(spec.get("staircase", False)))
    raise ValueError("%s: a dict needs knots= or decay_rate= / decay_steps=, got keys %s" % (name, sorted(map(str, spec))))


def schedule_struct(spec, name="schedule"):
    """One argument of ``set_schedule`` -> its ``avae_schedule`` (``_capi.Schedule``), or None for off."""
    from ._capi import SCHED_EXP, SCHED_PIECEWISE, Schedule
    spec = schedule_spec(spec, name)
    if spec is None:
        return None
    sc = Schedule()
    if "knots" in spec:
        sc.kind, sc.n_knots, sc.period = SCHED_PIECEWISE, len(spec["knots"]), spec["period"]
        for i, (st, v) in enumerate(spec["knots"]):
            sc.knot_step[i], sc.knot_value[i] = st, v
    else:
        sc.kind, sc.decay_rate, sc.decay_steps, sc.staircase = SCHED_EXP, spec["decay_rate"], spec["decay_steps"], int(spec["staircase"])
    return sc


def schedule_in_steps(spec, steps_per_unit, name="schedule"):
    """A schedule whose knot steps, period and ``decay_steps`` count units of ``steps_per_unit`` steps (epochs) -> the same
    schedule in steps, checked.  Fractions of a unit are fine where they come to whole steps."""
    if spec is None or _is_number(spec):
        return schedule_spec(spec, name)
    if not isinstance(spec, dict):
        return schedule_spec(spec, name)           # (raises)
    if steps_per_unit < 1:
        raise ValueError("%s: an epoch of this data set holds no step" % name)
    out = dict(spec)

    def conv(x, what):
        if not _is_number(x) or not np.isfinite(x):
            raise ValueError("%s: %s must be a number of epochs, got %r" % (name, what, x))
        return _whole(round(float(x) * steps_per_unit, 9), "%s: %s in steps" % (name, what))
    if "knots" in out:
        out["knots"] = [(conv(kv[0], "knots[%d] step" % i), kv[1]) if len(kv) == 2 else kv for i, kv in enumerate(out["knots"])]
        if out.get("period") is not None:
            out["period"] = conv(out["period"], "period")
    if out.get("decay_steps") is not None:
        out["decay_steps"] = conv(out["decay_steps"], "decay_steps")
    return schedule_spec(out, name)


def schedule_kwargs(schedule, steps_per_epoch=None):
    """The ``schedule=`` keyword of the constructor and of ``train`` -> the keyword arguments of ``set_schedule``: None (off) or a
    dict with the keys ``kl``, ``assoc``, ``lr`` (each an argument of ``set_schedule``) and ``unit`` ('step', the default, or
    'epoch').  With ``steps_per_epoch`` given, a schedule in epochs is converted to steps; without it the schedules are only
    checked, as they stand (the ranges are the same in either unit)."""
    if schedule is None:
        return {}
    if not isinstance(schedule, dict):
        raise ValueError("schedule must be None or a dict with the keys kl, assoc, lr and unit, got %r" % (schedule,))
    extra = set(schedule) - set(SCHEDULE_NAMES) - {"unit"}
    if extra:
        raise ValueError("schedule: unknown key(s) %s (kl, assoc, lr, unit)" % ", ".join(sorted(map(str, extra))))
    unit = schedule.get("unit", "step")
    if unit not in ("step", "epoch"):
        raise ValueError("schedule: unit must be 'step' or 'epoch', got %r" % (unit,))
    kw = {}
    for name in SCHEDULE_NAMES:
        if schedule.get(name) is None:
            continue
        if unit == "epoch":
            kw[name] = schedule_in_steps(schedule[name], 1 if steps_per_epoch is None else steps_per_epoch, name)
        else:
            kw[name] = schedule_spec(schedule[name], name)
    return kw


def linear_warmup(n_steps, start=0.0):
    """Multiplier rising linearly from ``start`` at the first step to 1 after ``n_steps`` steps, 1 from then on (KL warm-up)."""
    return dict(knots=[(0, start), (n_steps, 1.0)], period=None)


def cyclical(period, ramp=0.5, start=0.0):
    """Cyclical annealing: every ``period`` steps the multiplier rises linearly from ``start`` to 1 over the first ``ramp``
    fraction of the cycle and stays at 1 for the rest.  (In steps, ``period * ramp`` must be a whole number; in epochs --
    ``train(schedule=dict(..., unit='epoch'))`` -- it must come to whole steps.)"""
    up = period * ramp
    if not 0 < up < period:
        raise ValueError("cyclical: ramp must be in (0, 1) and period positive, got ramp %r, period %r" % (ramp, period))
    if float(up) == int(up):
        up = int(up)
    return dict(knots=[(0, start), (up, 1.0)], period=period)


def exponential_decay(rate, steps, staircase=False):
    """Multiplier ``rate ** (step / steps)`` (``rate ** (step // steps)`` with ``staircase``): tf.train.exponential_decay."""
    return dict(decay_rate=rate, decay_steps=steps, staircase=bool(staircase))


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


def dev_frames(a, device, name="frames"):
    """uint8 frames ``[N, Hf, Wf]`` or ``[N, Hf, Wf, C]`` -> (uint8 tensor [N, Hf, Wf, C] on ``device``, row stride, frame stride
    in bytes, was_numpy).  A tensor whose pixels are dense (channel stride 1, pixel stride C) and whose rows and frames do not
    overlap passes through with its strides -- a crop of wider frames, padded rows -- without a copy; anything else is copied
    once.  Other dtypes are refused: the thresholds and the grey formula are those of 8-bit pixels."""
    was_np = not torch.is_tensor(a)
    t = torch.as_tensor(np.asarray(a)) if was_np else a
    if t.dtype != torch.uint8:
        raise ValueError("%s must be uint8 (8-bit pixels, 0 .. 255), got %s: scale and round float frames first"
                         % (name, str(t.dtype).replace("torch.", "")))
    if t.dim() == 3:
        t = t.unsqueeze(3)
    if t.dim() != 4:
        raise ValueError("%s must be [N, Hf, Wf] or [N, Hf, Wf, C], got %s" % (name, tuple(t.shape)))
    t = t.to(device)
    N, Hf, Wf, Cn = (int(s) for s in t.shape)
    if N and Hf and Wf and Cn:
        row = t.stride(1) if Hf > 1 else Wf * Cn          # (the stride of a single row or frame is arbitrary)
        frame = t.stride(0) if N > 1 else (Hf - 1) * row + Wf * Cn
        dense = (Cn == 1 or t.stride(3) == 1) and (Wf == 1 or t.stride(2) == Cn)
        if not dense or row < Wf * Cn or frame < (Hf - 1) * row + Wf * Cn:
            t = t.contiguous()
            row, frame = Wf * Cn, Hf * Wf * Cn
    else:
        row, frame = Wf * Cn, Hf * Wf * Cn
    return t, row, frame, was_np


def dev_block3(a, tail, device, name, rows=None):
    """[rows, tail[0], tail[1]] block (None in ``tail`` = any size) -> (contiguous float32 tensor on ``device``, was_numpy)"""
    was_np = not torch.is_tensor(a)
    t = torch.as_tensor(np.asarray(a, dtype=np.float32) if was_np else a)
    ok = t.dim() == 3 and all(w is None or t.shape[i + 1] == w for i, w in enumerate(tail))
    if not ok or (rows is not None and t.shape[0] != rows):
        want = ", ".join(["rows" if rows is None else "%d" % rows] + ["any" if w is None else "%d" % w for w in tail])
        raise ValueError("%s must be [%s], got %s" % (name, want, tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous(), was_np
