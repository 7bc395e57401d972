"""One validator per entry point of ``vae_assoc.AssocVariationalAutoEncoder``: the caller's arguments checked and marshalled
into what the method hands to the library.

Every error of shape, type or range is a ``ValueError`` raised here, ahead of any launch.  The functions take the device, the
widths and ``n_z`` as arguments and touch neither a model nor the library, so they run on CPU tensors (``device="cpu"``) in the
tests.  Arrays go through ``_marshal``; the limits are ``_capi``'s."""
import numpy as np
import torch

from . import _capi
from ._marshal import (_is_number, as_index, as_int, dev_array, dev_block3, dev_dense, dev_dense3, dev_flags, dev_frames,
                       dev_modalities, dev_row_args, need_type, to_device32)
from .kinematics import KinematicChain, StrokeCanvas
from .motion import MotionBasis


def metric_id(metric):
    """'symkl' or 'l2' in any case -> the library's metric id"""
    if not isinstance(metric, str) or metric.lower() not in _capi.METRIC_IDS:
        raise ValueError("metric must be 'symkl' or 'l2', got %r" % (metric,))
    return _capi.METRIC_IDS[metric.lower()]


def impute_args(X, present, n_samples, eps, widths, n_z, device):
    """The arguments of ``impute`` checked and marshalled -> (tensors, N, was_numpy, ptrs, lds, presence or None, K, eps or None)."""
    K = as_int(n_samples, "n_samples", 0)
    if present is None:
        ts, rows, was_np, ptrs, lds = dev_modalities(X, widths, device, allow_none=True)
        if rows is None:
            raise ValueError("every modality is None and there is no present array: the row count is unknown")
        p = None
    else:
        ts, rows, was_np, ptrs, lds, p = dev_row_args(X, widths, device, present)
    if K == 0 and eps is not None:
        raise ValueError("eps needs n_samples >= 1 (n_samples = 0 decodes the fused mean, without noise)")
    e = dev_dense3(eps, (rows, K, n_z), device)
    return ts, rows, was_np, ptrs, lds, p, K, e


def topk_args(query, gallery, k, metric, n_z, device):
    """The arguments of ``latent_topk`` checked and marshalled -> (q_mu, q_logvar or None, g_mu, g_logvar or None, k, metric id,
    was_numpy).  ``query`` and ``gallery`` are ``(mu, logvar)`` pairs of ``[rows, n_z]`` arrays or tensors; ``logvar`` may be None
    under ``metric="l2"``, which never reads it."""
    mid = metric_id(metric)
    k = as_int(k, "k", 1, _capi.TOPK_MAX)
    out, was_np = [], None
    for name, pair in (("query", query), ("gallery", gallery)):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("%s must be a (mu, logvar) pair, got %r" % (name, type(pair).__name__))
        mu, lv = pair
        if mu is None:
            raise ValueError("%s: mu is None" % name)
        if lv is None and mid == _capi.METRIC_SYMKL:
            raise ValueError("%s: logvar is None, and metric='symkl' reads the log-variances (metric='l2' does not)" % name)
        try:
            t = dev_dense(mu, n_z, device, name="%s mu" % name)
            if was_np is None:
                was_np = not torch.is_tensor(mu)
            rows = t.shape[0]
            lt = None if mid == _capi.METRIC_L2 else dev_dense(lv, n_z, device, rows, "as mu", name="%s logvar" % name)
        except ValueError as e:
            raise ValueError("%s: %s" % (name, e))
        out += [t, lt]
    return out[0], out[1], out[2], out[3], k, mid, was_np


def agg_args(z, gallery, exclude, marginals, n_z, device):
    """The arguments of ``aggregate_log_density`` checked and marshalled -> (z, g_mu, g_logvar, exclude or None, marginals,
    was_numpy).  ``z`` is ``[N, n_z]``, ``gallery`` a ``(mu, logvar)`` pair of ``[G, n_z]`` arrays or tensors, ``exclude`` None or
    ``[N]`` integers."""
    if z is None:
        raise ValueError("z is None")
    if not isinstance(gallery, (tuple, list)) or len(gallery) != 2:
        raise ValueError("gallery must be a (mu, logvar) pair, got %r" % type(gallery).__name__)
    mu, lv = gallery
    if mu is None or lv is None:
        raise ValueError("gallery: %s is None: the density reads both" % ("mu" if mu is None else "logvar"))
    zt = dev_dense(z, n_z, device, name="z")
    try:
        gm = dev_dense(mu, n_z, device, name="mu")
        gl = dev_dense(lv, n_z, device, gm.shape[0], "as mu", name="logvar")
    except ValueError as e:
        raise ValueError("gallery: %s" % e)
    ex = None
    if exclude is not None:
        ex = torch.as_tensor(exclude if torch.is_tensor(exclude) else np.asarray(exclude))
        if ex.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError("exclude must hold integers (gallery row numbers), got %s" % ex.dtype)
        if tuple(ex.shape) != (zt.shape[0],):
            raise ValueError("exclude must be [%d] (one gallery row per row of z), got %s" % (zt.shape[0], tuple(ex.shape)))
        big = torch.iinfo(torch.int32).max
        ex = ex.to(device=device, dtype=torch.int64).clamp(-1, big).to(torch.int32).contiguous()      # (anything outside the gallery excludes nothing)
    return zt, gm, gl, ex, bool(marginals), not torch.is_tensor(z)


def _is_pair(x):
    """a ``(mu, logvar)`` pair of arrays or tensors (``logvar`` may be None), as opposed to a list of such pairs"""
    return isinstance(x, (tuple, list)) and len(x) == 2 and hasattr(x[0], "shape") and (x[1] is None or hasattr(x[1], "shape"))


def _pairs(posteriors):
    """one ``(mu, logvar)`` pair or a non-empty list of them -> the list"""
    pairs = [posteriors] if _is_pair(posteriors) else posteriors
    if not isinstance(pairs, (list, tuple)) or not pairs or not all(_is_pair(p) for p in pairs):
        raise ValueError("posteriors must be a (mu, logvar) pair or a non-empty list of such pairs, got %r" % type(posteriors).__name__)
    return pairs


def posterior_rows(posteriors, n_z, device, need_logvar):
    """A ``(mu, logvar)`` pair of ``[N, n_z]`` arrays or tensors, or a list of such pairs whose rows are concatenated in list order
    -> (mu, logvar (None unless ``need_logvar``: it is not looked at then), the mask [N] of the rows without a non-finite entry,
    was_numpy of the first mu).  With ``need_logvar`` every pair has to hold one: a missing one is for the caller to refuse, in its
    own words, ahead of this call."""
    pairs = _pairs(posteriors)
    mus, lvs = [], []
    for i, (mu, lv) in enumerate(pairs):
        try:
            t = dev_dense(mu, n_z, device, name="mu")
            mus.append(t)
            if need_logvar:
                lvs.append(dev_dense(lv, n_z, device, t.shape[0], "as mu", name="logvar"))
        except ValueError as e:
            raise ValueError("posteriors[%d]: %s" % (i, e))
    mu = mus[0] if len(mus) == 1 else torch.cat(mus).contiguous()
    lv = None if not lvs else (lvs[0] if len(lvs) == 1 else torch.cat(lvs).contiguous())
    fin = torch.isfinite(mu).all(dim=1)
    if lv is not None:
        fin &= torch.isfinite(lv).all(dim=1)
    return mu, lv, fin, not torch.is_tensor(pairs[0][0])


def prior_arrays(prior, n_z, device, name="prior", n_components=None):
    """A mixture prior checked and marshalled -> (weights [K], means [K, n_z], logvars [K, n_z] contiguous float32 tensors on
    ``device``, was_numpy).  ``prior`` is a dict with the keys ``weights``, ``means`` and ``logvars`` (what ``fit_latent_prior``
    returns; further keys are ignored)."""
    if not isinstance(prior, dict) or any(k not in prior for k in ("weights", "means", "logvars")):
        raise ValueError("%s must be a dict with the keys weights, means and logvars, got %r"
                         % (name, sorted(prior) if isinstance(prior, dict) else type(prior).__name__))
    w, was_np = prior["weights"], not torch.is_tensor(prior["weights"])
    w = torch.as_tensor(np.asarray(w, dtype=np.float32) if was_np else w).to(device=device, dtype=torch.float32).contiguous()
    if w.dim() != 1 or not 1 <= w.shape[0] <= _capi.GMM_MAX_COMPONENTS:
        raise ValueError("%s: weights must be [K] with 1 <= K <= %d, got %s" % (name, _capi.GMM_MAX_COMPONENTS, tuple(w.shape)))
    K = int(w.shape[0])
    if n_components is not None and K != n_components:
        raise ValueError("%s: weights must be [%d] (n_components), got %s" % (name, n_components, tuple(w.shape)))
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not float(w.sum()) > 0:
        raise ValueError("%s: weights must be finite, non-negative and not all zero" % name)
    try:
        m = dev_dense(prior["means"], n_z, device, K, "as weights", name="means")
        lv = dev_dense(prior["logvars"], n_z, device, K, "as weights", name="logvars")
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e))
    if m is None or lv is None:
        raise ValueError("%s: %s is None" % (name, "means" if m is None else "logvars"))
    return w, m, lv, was_np


def latent_prior_args(posteriors, n_components, n_iters, init, seed, var_floor, n_z, device):
    """The arguments of ``fit_latent_prior`` checked and marshalled -> (mu, logvar or None, K, n_iters, var_floor, init, seed_rows,
    was_numpy).  ``posteriors`` is a ``(mu, logvar)`` pair of ``[N, n_z]`` arrays or tensors (``logvar`` may be None: points) or
    a list of such pairs, whose rows are concatenated in list order (every pair with a logvar, or none).  ``init`` comes back as
    the ``(weights, means, logvars)`` tensors of the given dict (copies: the fit works in place) and ``seed_rows`` as None, or,
    for ``init=None``, ``init`` is None and ``seed_rows`` a LongTensor of the K rows the means start from:
    ``np.random.default_rng(seed).permutation(F)[:K]`` over the F rows without a non-finite entry, in row order."""
    K = as_int(n_components, "n_components", 1, _capi.GMM_MAX_COMPONENTS)
    n_iters = as_int(n_iters, "n_iters", 0)
    try:
        vf = float(var_floor)
    except (TypeError, ValueError):
        raise ValueError("var_floor must be a positive finite number, got %r" % (var_floor,))
    if not (vf > 0.0 and np.isfinite(vf) and float(np.float32(vf)) > 0.0 and np.isfinite(np.float32(vf))):
        raise ValueError("var_floor must be a positive finite number (in float32), got %r" % (var_floor,))
    pairs = _pairs(posteriors)
    if len({p[1] is None for p in pairs}) != 1:
        raise ValueError("posteriors: every pair needs a logvar, or none may have one (points)")
    mu, lv, fin, was_np = posterior_rows(pairs, n_z, device, pairs[0][1] is not None)
    if init is not None:
        w, m, s, _ = prior_arrays(init, n_z, device, name="init", n_components=K)
        return mu, lv, K, n_iters, vf, (w.clone(), m.clone(), s.clone()), None, was_np
    seed = as_int(seed, "seed", 0)
    rows = torch.nonzero(fin).reshape(-1).cpu()
    F = int(rows.shape[0])
    if K > F:
        raise ValueError("n_components = %d is more than the %d rows without a non-finite entry that the means are drawn from" % (K, F))
    pick = np.random.default_rng(seed).permutation(F)[:K]
    return mu, lv, K, n_iters, vf, None, rows[torch.from_numpy(pick.astype(np.int64))], was_np


def embed_args(posteriors, perplexity, n_iters, metric, learning_rate, early_exaggeration, exaggeration_iters, momentum, init,
               seed, state, n_z, device):
    """The arguments of ``embed_latents`` checked and marshalled -> dict(mu, logvar (None under ``metric="l2"``), metric id, rows,
    n_used, perplexity, n_iters, learning_rate, early_exaggeration, exaggeration_iters, momentum, y, vel, gain, it0, calibration
    (None: to be computed), was_numpy).  ``posteriors`` is a ``(mu, logvar)`` pair of ``[N, n_z]`` arrays or tensors or a list of
    such pairs, concatenated in list order, as in ``latent_prior_args``; ``logvar=None`` needs ``metric="l2"``.  ``y`` is a copy of
    ``init`` or, for ``init=None``, ``np.random.default_rng(seed).normal(0, 1e-4, (N, 2))``; ``state`` (what ``embed_latents``
    returned) replaces velocity, gains, iteration number and calibration, and ``init`` then defaults to its embedding.
    ``learning_rate="auto"`` is ``max(F / 48, 50)`` over the F rows without a non-finite entry."""
    mid = metric_id(metric)
    n_iters = as_int(n_iters, "n_iters", 0)
    exaggeration_iters = as_int(exaggeration_iters, "exaggeration_iters", 0)

    def number(x, name, lo=None):
        try:
            v = float(x)
        except (TypeError, ValueError):
            v = float("nan")
        if isinstance(x, bool) or not np.isfinite(v) or not np.isfinite(np.float32(v)) or (lo is not None and not v > lo):
            raise ValueError("%s must be a finite number%s, got %r" % (name, "" if lo is None else " > %g" % lo, x))
        return v
    ee = number(early_exaggeration, "early_exaggeration", 0.0)
    if not isinstance(momentum, (tuple, list)) or len(momentum) != 2:
        raise ValueError("momentum must be a pair (during the early exaggeration, after it), got %r" % (momentum,))
    mom = (number(momentum[0], "momentum[0]"), number(momentum[1], "momentum[1]"))
    pairs = _pairs(posteriors)
    if mid == _capi.METRIC_SYMKL and any(p[1] is None for p in pairs):
        raise ValueError("posteriors: logvar is None, and metric='symkl' reads the log-variances (metric='l2' does not)")
    mu, lv, fin, was_np = posterior_rows(pairs, n_z, device, mid == _capi.METRIC_SYMKL)
    N = int(mu.shape[0])
    if N > _capi.EMBED_MAX_ROWS:
        raise ValueError("%d rows are more than the %d one map takes (the work is quadratic in the rows)" % (N, _capi.EMBED_MAX_ROWS))
    F = int(fin.sum().item())
    perp = number(perplexity, "perplexity")
    if N < 2 or not 1.0 <= perp <= F - 1:
        raise ValueError("perplexity = %r must be in [1, F - 1] for the F = %d rows without a non-finite entry (of %d rows)"
                         % (perplexity, F, N))
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError("learning_rate must be 'auto' or a positive number, got %r" % (learning_rate,))
        lr = max(F / 48.0, 50.0)
    else:
        lr = number(learning_rate, "learning_rate", 0.0)

    def map_array(x, name):
        t = dev_dense(x, 2, device, N, "as the posteriors", name=name)
        if t is None:
            raise ValueError("%s is None" % name)
        return t.clone()

    def row_vector(x, name):
        t = torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x, dtype=np.float32)).to(device=device, dtype=torch.float32)
        if tuple(t.shape) != (N,):
            raise ValueError("%s must be [%d] (as the posteriors), got %s" % (name, N, tuple(t.shape)))
        return t.contiguous().clone()
    it0, calib, vel, gain = 0, None, None, None
    if state is not None:
        keys = ("velocity", "gains", "iteration", "beta", "shift", "norm")
        if not isinstance(state, dict) or any(k not in state for k in keys + ("embedding",)):
            raise ValueError("state must be the state dict embed_latents returned (keys embedding, %s), got %r"
                             % (", ".join(keys), sorted(state) if isinstance(state, dict) else type(state).__name__))
        it0 = as_int(state["iteration"], "state: iteration", 0)
        try:
            vel, gain = map_array(state["velocity"], "velocity"), map_array(state["gains"], "gains")
            calib = tuple(row_vector(state[k], k) for k in ("beta", "shift", "norm"))
            if init is None:
                init = state["embedding"]
        except ValueError as e:
            raise ValueError("state: %s" % e)
    if init is None:
        seed = as_int(seed, "seed", 0)
        y = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1e-4, (N, 2)).astype(np.float32)).to(device)
    else:
        try:
            y = map_array(init, "init")
        except ValueError as e:
            raise ValueError("init: %s" % e)
    if vel is None:
        vel = torch.zeros((N, 2), dtype=torch.float32, device=device)
        gain = torch.ones((N, 2), dtype=torch.float32, device=device)
    return {"mu": mu, "logvar": lv, "metric": mid, "rows": N, "n_used": F, "perplexity": perp, "n_iters": n_iters,
            "learning_rate": lr, "early_exaggeration": ee, "exaggeration_iters": exaggeration_iters, "momentum": mom,
            "y": y, "vel": vel, "gain": gain, "it0": it0, "calibration": calib, "was_numpy": was_np}


def latent_score_args(z, prior, n_z, device):
    """The arguments of ``latent_prior_score`` checked and marshalled -> (mu, logvar or None, weights, means, logvars,
    was_numpy).  ``z`` is a ``[N, n_z]`` array or tensor (points) or a ``(mu, logvar)`` pair."""
    if z is None:
        raise ValueError("z is None")
    mu, lv = z if _is_pair(z) else (z, None)
    try:
        mt = dev_dense(mu, n_z, device, name="mu" if _is_pair(z) else "z")
        lt = dev_dense(lv, n_z, device, mt.shape[0], "as mu", name="logvar")
    except ValueError as e:
        raise ValueError("z: %s" % e)
    w, m, s, _ = prior_arrays(prior, n_z, device)
    return mt, lt, w, m, s, not torch.is_tensor(mu)


def latent_stats_args(posteriors, present, n_z, device):
    """The arguments of ``latent_stats`` checked and marshalled -> (mus, logvars, rows, presence or None, was_numpy): two lists
    over the modalities of ``[rows, n_z]`` tensors, None where the modality is absent everywhere.  ``posteriors`` is a list of 1 to
    4 ``(mu, logvar)`` pairs or None; ``present`` [rows, M] flags or None."""
    if not isinstance(posteriors, (list, tuple)) or not 1 <= len(posteriors) <= _capi.AVAE_MAX_MODALITIES:
        raise ValueError("posteriors must be a list over 1 to %d modalities of (mu, logvar) pairs or None, got %r"
                         % (_capi.AVAE_MAX_MODALITIES, type(posteriors).__name__ if not isinstance(posteriors, (list, tuple))
                            else len(posteriors)))
    M = len(posteriors)
    p = None if present is None else dev_flags(present, M, device)
    rows, what = (None, None) if p is None else (int(p.shape[0]), "as present")
    mus, lvs, was_np = [], [], None
    for m, pair in enumerate(posteriors):
        if pair is None:
            mus.append(None)
            lvs.append(None)
            continue
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("posteriors[%d] must be a (mu, logvar) pair or None, got %r" % (m, type(pair).__name__))
        mu, lv = pair
        if mu is None:
            raise ValueError("posteriors[%d]: mu is None (None in place of the pair marks a modality absent everywhere)" % m)
        if lv is None:
            raise ValueError("posteriors[%d]: logvar is None: a mu needs its logvar" % m)
        try:
            t = dev_dense(mu, n_z, device, rows, what, name="mu")
            if rows is None:
                rows, what = t.shape[0], "as posteriors[%d]" % m
            lt = dev_dense(lv, n_z, device, rows, "as mu", name="logvar")
        except ValueError as e:
            raise ValueError("posteriors[%d]: %s" % (m, e))
        if was_np is None:
            was_np = not torch.is_tensor(mu)
        mus.append(t)
        lvs.append(lt)
    if rows is None:
        raise ValueError("every modality is None and there is no present array: the row count is unknown")
    return mus, lvs, rows, p, (not torch.is_tensor(present)) if was_np is None else was_np


# ---------------------------------------------------------------------------------------------------- motion decoding
def _fits_params(basis, modality, widths):
    if basis.n_params != widths[modality]:
        raise ValueError("basis.n_params = %d must be n_input = %d of modality %d" % (basis.n_params, widths[modality], modality))


def motion_matrices(basis, device, anchor=None, rows=None, T=None):
    """A ``MotionBasis`` (and an optional anchor) -> the device matrices of the motion calls: dict of ``phi [T, Kb]``, ``scale``,
    ``shift [P]`` or None, ``limits [D, 2]`` or None, ``gain [T, n_c]`` and ``target [rows, D, n_c]`` or None, ``nc``.  ``anchor`` is
    None or ``dict(phases=[...], target=[rows, D, n_c])``: the trajectories are those of the parameters projected onto
    ``features(phases) theta == target`` (1 to 4 phases).  The matrices are cached on the basis per device, phases and T."""
    need_type(basis, MotionBasis, "basis")
    phases = target = None
    if anchor is not None:
        if not isinstance(anchor, dict) or set(anchor) != {"phases", "target"}:
            raise ValueError("anchor must be None or dict(phases=, target=)")
        phases = np.atleast_1d(np.asarray(anchor["phases"], dtype=np.float64))
        basis.constraint(phases)                       # (checks the phases)
        target, _ = dev_block3(anchor["target"], (basis.n_dof, len(phases)), device, "anchor target", rows)
    key = ("device", str(device), None if phases is None else phases.tobytes(), T)
    if key not in basis._cache:
        def up(a):
            return None if a is None else to_device32(a, device)
        phi, gain = basis.eval_matrices(phases, T)
        sc, sh = basis.scale_shift()
        basis._cache[key] = dict(phi=up(phi), gain=up(gain), scale=up(sc), shift=up(sh), limits=up(basis.limits))
    out = dict(basis._cache[key])
    out.update(target=target, nc=0 if phases is None else len(phases))
    return out


def motion_eval_args(params, basis, anchor, reference, reference_params, device):
    """The arguments of ``motion_eval`` checked and marshalled -> (params [N, P], matrices, reference trajectory or None, reference
    parameters or None, was_numpy)."""
    need_type(basis, MotionBasis, "basis")
    if reference is not None and reference_params is not None:
        raise ValueError("reference and reference_params are both given: pass one reference")
    p, was_np = dev_array(params, basis.n_params, device)
    p = p.contiguous()
    rows = p.shape[0]
    mats = motion_matrices(basis, device, anchor, rows)
    ref = None if reference is None else dev_block3(reference, (basis.n_points, basis.n_dof), device, "reference", rows)[0]
    refp = dev_dense(reference_params, basis.n_params, device, rows, "as params", name="reference_params")
    return p, mats, ref, refp, was_np


def motion_fit_args(trajectories, basis, device):
    """The arguments of ``motion_fit`` -> (trajectories [N, T, D], pinv [Kb, T], scale, shift, was_numpy)."""
    need_type(basis, MotionBasis, "basis")
    t, was_np = dev_block3(trajectories, (None, basis.n_dof), device, "trajectories")
    T = int(t.shape[1])
    if not 1 <= T <= _capi.MOTION_MAX_POINTS:
        raise ValueError("trajectories must hold 1 to %d time points, got %d" % (_capi.MOTION_MAX_POINTS, T))
    key = ("device pinv", str(device), T)
    if key not in basis._cache:
        basis._cache[key] = to_device32(basis.pinv(T), device)
    mats = motion_matrices(basis, device)
    return t, basis._cache[key], mats["scale"], mats["shift"], was_np


def motion_moments_args(samples, basis, anchor, device):
    """The arguments of ``motion_moments`` -> (samples [N, S, P], matrices, was_numpy)."""
    need_type(basis, MotionBasis, "basis")
    t, was_np = dev_block3(samples, (None, basis.n_params), device, "samples")
    if t.shape[1] < 1:
        raise ValueError("samples must hold at least one sample per row, got %s" % (tuple(t.shape),))
    return t, motion_matrices(basis, device, anchor, int(t.shape[0])), was_np


def predict_motion_args(X, basis, modality, present, n_samples, eps, anchor, widths, n_z, device):
    """The arguments of ``predict_motion`` -> (``impute_args``' tuple with K = 0 and the eps block [N, S, n_z] or None in its last
    two places, matrices)."""
    need_type(basis, MotionBasis, "basis")
    as_index(modality, "modality", len(widths))
    _fits_params(basis, modality, widths)
    ts, rows, was_np, xp, lds, p, S, e = impute_args(X, present, n_samples, eps, widths, n_z, device)
    return (ts, rows, was_np, xp, lds, p, S, e), motion_matrices(basis, device, anchor, rows)


# ---------------------------------------------------------------------------------------------------- pen path and drawing
def _same_joints(basis, chain):
    if chain.n_dof != basis.n_dof:
        raise ValueError("chain.n_dof = %d must be basis.n_dof = %d" % (chain.n_dof, basis.n_dof))


def _check_writer(basis, chain, canvas):
    """the three objects a composed writer call takes, and that basis and chain speak of the same joints"""
    need_type(basis, MotionBasis, "basis")
    need_type(chain, KinematicChain, "chain")
    need_type(canvas, StrokeCanvas, "canvas")
    _same_joints(basis, chain)


def _fits_pixels(canvas, image_modality, widths):
    if canvas.n_pixels != widths[image_modality]:
        raise ValueError("the canvas draws %d pixels, modality %d holds %d" % (canvas.n_pixels, image_modality, widths[image_modality]))


def chain_matrices(chain, device):
    """A ``KinematicChain`` -> (``frames [n_dof + 1, 3, 4]``, ``axes [n_dof, 3]``) as float32 tensors on ``device``, cached on the
    chain per device."""
    need_type(chain, KinematicChain, "chain")
    key = ("device", str(device))
    if key not in chain._cache:
        chain._cache[key] = tuple(torch.as_tensor(a).to(device) for a in chain.packed())
    return chain._cache[key]


def motion_fk_args(trajectories, chain, device):
    """The arguments of ``motion_fk`` -> (trajectories [N, T, n_dof], frames, axes, was_numpy)."""
    frames, axes = chain_matrices(chain, device)
    t, was_np = dev_block3(trajectories, (None, chain.n_dof), device, "trajectories")
    if not 1 <= t.shape[1] <= _capi.MOTION_MAX_POINTS:
        raise ValueError("trajectories must hold 1 to %d time points, got %d" % (_capi.MOTION_MAX_POINTS, t.shape[1]))
    return t, frames, axes, was_np


def canvas_args(canvas, rows, target, height, device):
    """A ``StrokeCanvas`` and the optional inputs of a drawing of ``rows`` rows -> (plane [3, 3], target [rows, H * H] or None,
    height [rows] or None) on ``device`` (the plane cached on the canvas per device).  ``target`` may be one picture ``[H * H]`` for
    every row, ``height`` one number."""
    need_type(canvas, StrokeCanvas, "canvas")
    key = ("device", str(device))
    if key not in canvas._cache:
        canvas._cache[key] = to_device32(canvas.plane, device)
    plane = canvas._cache[key]
    if target is not None:
        t = target if torch.is_tensor(target) else torch.as_tensor(np.asarray(target, dtype=np.float32))
        if t.dim() == 1:
            t = t.reshape(1, -1).expand(rows, -1)
        target = dev_dense(t, canvas.n_pixels, device, rows, "as the paths", name="target")
    if height is not None:
        h = height if torch.is_tensor(height) else torch.as_tensor(np.asarray(height, dtype=np.float32))
        if h.dim() == 0:
            h = h.reshape(1).expand(rows)
        if h.dim() != 1 or h.shape[0] != rows:
            raise ValueError("height must be a number or [%d] (as the paths), got %s" % (rows, tuple(h.shape)))
        height = h.to(device=device, dtype=torch.float32).contiguous()
    return plane, target, height


def render_args(path, canvas, target, height, device):
    """The arguments of ``render_strokes`` -> (path [N, T, 3], plane [3, 3], target [N, H * H] or None, height [N] or None,
    was_numpy)."""
    p, was_np = dev_block3(path, (None, 3), device, "path")
    if not 1 <= p.shape[1] <= _capi.MOTION_MAX_POINTS:
        raise ValueError("path must hold 1 to %d points, got %d" % (_capi.MOTION_MAX_POINTS, p.shape[1]))
    return (p,) + canvas_args(canvas, int(p.shape[0]), target, height, device) + (was_np,)


THUMBNAIL_CAMERA = dict(threshold=108, invert=True)     # the reference's camera path (drawing_pad.py:185-193)
THUMBNAIL_CANVAS = dict(invert=True)                    # its drawing pad (drawing_pad.py:282-299)


def letter_thumbnail_args(frames, size, threshold, invert, channel_order, device):
    """The arguments of ``letter_thumbnails`` -> (frames uint8 [N, Hf, Wf, C], row stride, frame stride, flags, threshold (-1:
    none), size, was_numpy)."""
    size = as_int(size, "size", 1, _capi.THUMB_MAX_SIZE)
    thr = -1 if threshold is None else as_int(threshold, "threshold", 0, 255)
    if not isinstance(invert, (bool, np.bool_)):
        raise ValueError("invert must be True or False, got %r" % (invert,))
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("channel_order must be 'rgb' or 'bgr', got %r" % (channel_order,))
    t, row, frame, was_np = dev_frames(frames, device)
    N, Hf, Wf, Cn = (int(s) for s in t.shape)
    if Cn not in (1, 3, 4):
        raise ValueError("frames must hold 1, 3 or 4 channels (grey, RGB, RGBA), got %d" % Cn)
    if not (1 <= Hf <= _capi.THUMB_MAX_FRAME and 1 <= Wf <= _capi.THUMB_MAX_FRAME):
        raise ValueError("frames must be 1 to %d pixels high and wide, got %d x %d" % (_capi.THUMB_MAX_FRAME, Hf, Wf))
    flags = (_capi.THUMB_INVERT if invert else 0) | (_capi.THUMB_BGR if channel_order == "bgr" else 0)
    return t, row, frame, flags, thr, size, was_np


def occlude_quadrant(images, quadrant):
    """The drawing pad's incomplete picture (drawing_pad.py:324-328): square pictures ``[N, H * H]`` (H even) with one quadrant
    set to 0 -> (the occluded pictures, the ``observed`` element mask ``complete()`` takes: uint8 [N, H * H], 0 inside the
    quadrant).  ``quadrant = (row half, column half)``, each 0 or 1 -- the reference's ``fraction_idx`` -- for every row, or an
    ``[N, 2]`` array with one pair per row.  NumPy in gives NumPy out, tensors in give tensors on the same device."""
    was_np = not torch.is_tensor(images)
    x = torch.as_tensor(np.asarray(images)) if was_np else images
    H = int(round(float(x.shape[1]) ** 0.5)) if x.dim() == 2 else 0
    if x.dim() != 2 or H * H != x.shape[1] or H % 2:
        raise ValueError("images must be [N, H * H] with H even, got %s" % (tuple(x.shape),))
    q = torch.as_tensor(np.asarray(quadrant) if not torch.is_tensor(quadrant) else quadrant.cpu().numpy())
    if q.dim() == 1:
        q = q.reshape(1, -1).expand(x.shape[0], -1)
    if tuple(q.shape) != (x.shape[0], 2) or q.dtype not in (torch.int32, torch.int64, torch.uint8, torch.bool) \
            or bool(((q != 0) & (q != 1)).any()):
        raise ValueError("quadrant must be (row half, column half) with halves 0 or 1, or [%d, 2] of them, got %r" % (x.shape[0], quadrant))
    q = q.to(device=x.device, dtype=torch.int64)
    half = torch.arange(H, device=x.device) // (H // 2)                                   # 0 for the first half, 1 for the second
    inside = (half[None, :, None] == q[:, 0, None, None]) & (half[None, None, :] == q[:, 1, None, None])      # [N, H, H]
    observed = (~inside).reshape(x.shape[0], H * H)
    out, observed = x * observed.to(x.dtype), observed.to(torch.uint8)
    return (out.numpy(), observed.numpy()) if was_np else (out, observed)


def draw_args(params, basis, chain, canvas, anchor, target, height, device):
    """The arguments of ``draw_motion`` -> (params [N, P], matrices, frames, axes, plane, target, height, was_numpy)"""
    p, mats, _, _, was_np = motion_eval_args(params, basis, anchor, None, None, device)
    frames, axes = chain_matrices(chain, device)
    _same_joints(basis, chain)
    return (p, mats, frames, axes) + canvas_args(canvas, int(p.shape[0]), target, height, device) + (was_np,)


def writing_cost_args(weights, image_modality, canvas, widths):
    """``writing_cost``'s own arguments checked -> the three weights as floats"""
    need_type(canvas, StrokeCanvas, "canvas")
    as_index(image_modality, "image_modality", len(widths))
    _fits_pixels(canvas, image_modality, widths)
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError("weights must be three numbers (image, height, latent), got %r" % (weights,))
    if len(w) != 3 or not all(np.isfinite(w)):
        raise ValueError("weights must be three finite numbers (image, height, latent), got %r" % (weights,))
    return w


# ---------------------------------------------------------------------------------------------------- black-box search
SEARCH_STATE_KEYS = ("mean", "var", "n_applied", "frozen", "best_cost", "best_x", "iteration")


def search_args(x0, var0, n_rollouts, n_iters, eliteness, weighting, cov_update, learning_rate, covar_bounds, tol, project, seed,
                state, device):
    """The arguments of ``search`` checked and marshalled -> (state: a fresh one from ``x0`` / ``var0`` or a copy of ``state``,
    ``_capi.SearchOptions``, n_rollouts, n_iters, (A, b, G, g) or None, seed, was_numpy).  Values of device tensors are not
    looked at: that would be a host round trip."""
    def number(v, name, lo=None, hi=None):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        if (lo is not None and v < lo) or (hi is not None and v > hi):
            raise ValueError("%s must be in [%s, %s], got %r" % (name, "-inf" if lo is None else lo, "inf" if hi is None else hi, v))
        return float(v)
    R = as_int(n_rollouts, "n_rollouts", 1, _capi.SEARCH_MAX_ROLLOUTS)
    n_iters = as_int(n_iters, "n_iters", 0, 1 << 30)
    seed = as_int(seed, "seed", 0, (1 << 64) - 1)
    if weighting not in _capi.SEARCH_IDS:
        raise ValueError("weighting must be 'PI-BB', 'CEM' or 'CMA-ES', got %r" % (weighting,))
    if cov_update not in ("PI-BB", "CEM"):
        raise ValueError("cov_update must be 'PI-BB' or 'CEM', got %r" % (cov_update,))
    opt = _capi.SearchOptions()
    opt.weighting, opt.cov_update = _capi.SEARCH_IDS[weighting], _capi.SEARCH_IDS[cov_update]
    opt.eliteness = number(eliteness, "eliteness", 0.0)
    if weighting != "PI-BB" and (opt.eliteness < 1 or opt.eliteness != int(opt.eliteness)):
        raise ValueError("eliteness must be a whole number >= 1 with %s weighting (the candidates kept), got %r" % (weighting, eliteness))
    opt.learning_rate = number(learning_rate, "learning_rate", 0.0, 1.0)
    opt.tol = number(tol, "tol", 0.0)
    bounds = [] if covar_bounds is None else list(np.atleast_1d(covar_bounds))
    if len(bounds) > 3:
        raise ValueError("covar_bounds must be None or up to three numbers (relative lower, absolute lower, absolute upper), got %r"
                         % (covar_bounds,))
    bounds = [number(b, "covar_bounds[%d]" % i) for i, b in enumerate(bounds)] + [-1.0] * (3 - len(bounds))
    if bounds[0] > 1.0:
        raise ValueError("covar_bounds[0] (the relative lower bound) must be <= 1, got %r" % (bounds[0],))
    opt.rel_lower, opt.abs_lower, opt.abs_upper = [b if b >= 0 else -1.0 for b in bounds]

    def f32(a, name):
        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float32))
        if t.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
            raise ValueError("%s must hold floating-point values, got %s" % (name, t.dtype))
        return t.to(device=device, dtype=torch.float32)
    if state is None:
        if x0 is None or var0 is None:
            raise ValueError("x0 and var0 are needed where there is no state to continue")
        was_np = not torch.is_tensor(x0)
        mean = f32(x0, "x0")
        if mean.dim() != 2 or not 1 <= mean.shape[1] <= _capi.SEARCH_MAX_DIMS:
            raise ValueError("x0 must be [P, n] with n in [1, %d], got %s" % (_capi.SEARCH_MAX_DIMS, tuple(mean.shape)))
        P, n = int(mean.shape[0]), int(mean.shape[1])
        if not torch.is_tensor(var0) and not (np.all(np.isfinite(var0)) and np.all(np.asarray(var0) >= 0)):
            raise ValueError("var0 must be finite and >= 0")
        if isinstance(var0, (int, float, np.integer, np.floating)):      # (filled on the device: no copy from the host)
            var = torch.full((), float(var0), dtype=torch.float32, device=device)
        else:
            var = f32(var0, "var0")
        if tuple(var.shape) not in ((), (n,), (P, n)):
            raise ValueError("var0 must be a number, [%d] or [%d, %d], got %s" % (n, P, n, tuple(var.shape)))
        st = dict(mean=mean.clone().contiguous(), var=var.expand(P, n).clone().contiguous(),
                  n_applied=torch.zeros(P, dtype=torch.int32, device=device), frozen=torch.zeros(P, dtype=torch.int32, device=device),
                  best_cost=torch.full((P,), float("inf"), dtype=torch.float32, device=device),
                  best_x=torch.zeros((P, n), dtype=torch.float32, device=device), iteration=0)
    else:
        if not isinstance(state, dict) or set(state) != set(SEARCH_STATE_KEYS):
            raise ValueError("state must be the dict a search returned (keys %s)" % ", ".join(SEARCH_STATE_KEYS))
        was_np = False
        if not torch.is_tensor(state["mean"]) or state["mean"].dim() != 2:
            raise ValueError("state['mean'] must be a [P, n] tensor")
        P, n = int(state["mean"].shape[0]), int(state["mean"].shape[1])
        st = {"iteration": as_int(state["iteration"], "state['iteration']", 0)}
        for k, shape, dt in (("mean", (P, n), torch.float32), ("var", (P, n), torch.float32), ("best_x", (P, n), torch.float32),
                             ("best_cost", (P,), torch.float32), ("n_applied", (P,), torch.int32), ("frozen", (P,), torch.int32)):
            t = state[k]
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
                raise ValueError("state[%r] must be a %s tensor of shape %s" % (k, dt, shape))
            st[k] = t.to(device).clone().contiguous()
    if st["iteration"] + n_iters >= 1 << 31:
        raise ValueError("the run's iterations must stay below 2^31")
    proj = None
    if project is not None:
        if not isinstance(project, (tuple, list)) or len(project) != 2:
            raise ValueError("project must be None or (A [G, g, g], b [P, n])")
        A, b = f32(project[0], "project A").contiguous(), f32(project[1], "project b").contiguous()
        if A.dim() != 3 or A.shape[1] != A.shape[2] or A.shape[0] * A.shape[1] != n or not 1 <= A.shape[1] <= _capi.SEARCH_MAX_GROUP:
            raise ValueError("project A must be [G, g, g] with G * g = n = %d and g <= %d, got %s"
                             % (n, _capi.SEARCH_MAX_GROUP, tuple(A.shape)))
        if tuple(b.shape) != (P, n):
            raise ValueError("project b must be [%d, %d], got %s" % (P, n, tuple(b.shape)))
        proj = (A, b, int(A.shape[0]), int(A.shape[1]))
    return st, opt, R, n_iters, proj, seed, was_np


def refine_motion_args(basis, chain, space, n_rollouts, modality, search_options, widths):
    """``refine_motion``'s own arguments checked -> (n_rollouts with the space's default, the options passed on to ``search``)"""
    need_type(basis, MotionBasis, "basis")
    need_type(chain, KinematicChain, "chain")
    _same_joints(basis, chain)
    if space not in ("latent", "params"):
        raise ValueError("space must be 'latent' or 'params', got %r" % (space,))
    as_index(modality, "modality", len(widths))
    _fits_params(basis, modality, widths)
    allowed = {"eliteness", "weighting", "cov_update", "learning_rate", "covar_bounds", "tol", "seed"}
    extra = set(search_options) - allowed
    if extra:
        raise ValueError("unknown option(s) %s (search takes %s)" % (", ".join(sorted(map(str, extra))), ", ".join(sorted(allowed))))
    if n_rollouts is None:
        n_rollouts = 10 if space == "latent" else 20
    return n_rollouts, dict(search_options)


# ---------------------------------------------------------------------------------------------------- gradients of the writing chain
def _row_values(v, rows, device, name):
    """An optional per-row number: None, one number for every row or ``[rows]`` -> contiguous float32 tensor [rows] or None"""
    if v is None:
        return None
    t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32))
    if t.dim() == 0:
        t = t.reshape(1).expand(rows)
    if t.dim() != 1 or t.shape[0] != rows:
        raise ValueError("%s must be a number or [%d] (as the paths), got %s" % (name, rows, tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def render_vjp_args(path, canvas, target, height, g_image, g_img_l2, g_height_l2, device):
    """The arguments of ``render_strokes_vjp`` -> (path [N, T, 3], plane, target, height, g_image [N, H * H], g_img_l2 [N],
    g_height_l2 [N] (each or None), was_numpy).  A cotangent of a distance needs that distance's input."""
    p, plane, tg, hg, was_np = render_args(path, canvas, target, height, device)
    rows = int(p.shape[0])
    if g_image is None and g_img_l2 is None and g_height_l2 is None:
        raise ValueError("g_image, g_img_l2 and g_height_l2 are all None: there is nothing to differentiate")
    if g_img_l2 is not None and tg is None:
        raise ValueError("g_img_l2 needs target: img_l2 is the distance from it")
    if g_height_l2 is not None and hg is None:
        raise ValueError("g_height_l2 needs height: height_l2 is the distance from it")
    gi = dev_dense(g_image, canvas.n_pixels, device, rows, "as the paths", name="g_image")
    return p, plane, tg, hg, gi, _row_values(g_img_l2, rows, device, "g_img_l2"), _row_values(g_height_l2, rows, device, "g_height_l2"), was_np


def motion_fk_vjp_args(trajectories, chain, grad_path, device):
    """The arguments of ``motion_fk_vjp`` -> (trajectories [N, T, n_dof], frames, axes, grad_path [N, T, 3], was_numpy)."""
    t, frames, axes, was_np = motion_fk_args(trajectories, chain, device)
    if grad_path is None:
        raise ValueError("grad_path is None: the cotangent of the pen path is needed")
    g, _ = dev_block3(grad_path, (int(t.shape[1]), 3), device, "grad_path", int(t.shape[0]))
    return t, frames, axes, g, was_np


def motion_eval_vjp_args(params, basis, anchor, grad_trajectory, device):
    """The arguments of ``motion_eval_vjp`` -> (params [N, P], matrices, grad_trajectory [N, n_points, n_dof], was_numpy)."""
    p, mats, _, _, was_np = motion_eval_args(params, basis, anchor, None, None, device)
    if grad_trajectory is None:
        raise ValueError("grad_trajectory is None: the cotangent of the trajectory is needed")
    g, _ = dev_block3(grad_trajectory, (basis.n_points, basis.n_dof), device, "grad_trajectory", int(p.shape[0]))
    return p, mats, g, was_np


def cost_weights(weights):
    """The two weights of the differentiable writing cost ``w0 (img_l2 + w1 height_l2)`` -> floats"""
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError("weights must be two numbers (image, height), got %r" % (weights,))
    if len(w) != 2 or not all(np.isfinite(w)):
        raise ValueError("weights must be two finite numbers (image, height), got %r" % (weights,))
    return w


ADAM_STATE_KEYS = ("m", "v", "t", "best_x", "best_cost")


def adam_options(lr, betas, eps, max_norm):
    """The options of ``rows_adam`` checked -> (lr, beta1, beta2, eps, max_norm; 0 = no clipping) as floats"""
    def number(v, name):
        if not _is_number(v) or not np.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        return float(v)
    lr = number(lr, "lr")
    if lr < 0:
        raise ValueError("lr must be >= 0, got %r" % (lr,))
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
    b1, b2 = number(betas[0], "betas[0]"), number(betas[1], "betas[1]")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or float(np.float32(b1)) >= 1.0 or float(np.float32(b2)) >= 1.0:
        raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
    eps = number(eps, "eps")
    if eps <= 0:
        raise ValueError("eps must be > 0, got %r" % (eps,))
    mn = 0.0
    if max_norm is not None:
        mn = number(max_norm, "max_norm")
        if mn <= 0:
            raise ValueError("max_norm must be None or > 0, got %r" % (max_norm,))
    return lr, b1, b2, eps, mn


def rows_adam_args(x, grad, state, cost, device):
    """The arrays of ``rows_adam`` -> (x [P, n] (a copy), grad [P, n], state: a fresh one or a copy of ``state``, cost [P] or None,
    was_numpy).  Values of device tensors are not looked at."""
    was_np = not torch.is_tensor(x)
    xt = torch.as_tensor(np.asarray(x, dtype=np.float32)) if was_np else x
    if xt.dim() != 2 or not 1 <= xt.shape[1] <= _capi.ROWS_ADAM_MAX_DIMS:
        raise ValueError("x must be [P, n] with n in [1, %d], got %s" % (_capi.ROWS_ADAM_MAX_DIMS, tuple(xt.shape)))
    xt = xt.to(device=device, dtype=torch.float32).clone().contiguous()
    P, n = int(xt.shape[0]), int(xt.shape[1])
    g = dev_dense(grad, n, device, P, "as x", name="grad")
    if g is None:
        raise ValueError("grad is None: the step needs the gradient")
    c = _row_values(cost, P, device, "cost")
    if state is None:
        st = dict(m=torch.zeros((P, n), dtype=torch.float32, device=device), v=torch.zeros((P, n), dtype=torch.float32, device=device),
                  t=torch.zeros(P, dtype=torch.int32, device=device), best_x=xt.clone(),
                  best_cost=torch.full((P,), float("inf"), dtype=torch.float32, device=device))
    else:
        if not isinstance(state, dict) or set(state) != set(ADAM_STATE_KEYS):
            raise ValueError("state must be the dict a rows_adam step returned (keys %s)" % ", ".join(ADAM_STATE_KEYS))
        st = {}
        for k, shape, dt in (("m", (P, n), torch.float32), ("v", (P, n), torch.float32), ("best_x", (P, n), torch.float32),
                             ("best_cost", (P,), torch.float32), ("t", (P,), torch.int32)):
            t = state[k]
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
                raise ValueError("state[%r] must be a %s tensor of shape %s" % (k, dt, shape))
            st[k] = t.to(device).clone().contiguous()
    return xt, g, st, c, was_np


DESCENT_STATE_KEYS = ("params", "adam", "height", "anchor", "iteration")


def descend_motion_args(basis, chain, canvas, n_iters, lr, max_norm, anchor_start, weights, modality, image_modality, widths):
    """``descend_motion``'s own arguments checked -> (n_iters, Adam options, the two weights)"""
    _check_writer(basis, chain, canvas)
    as_index(modality, "modality", len(widths))
    as_index(image_modality, "image_modality", len(widths))
    _fits_params(basis, modality, widths)
    _fits_pixels(canvas, image_modality, widths)
    if basis.n_params > _capi.ROWS_ADAM_MAX_DIMS:
        raise ValueError("basis.n_params = %d must be at most %d" % (basis.n_params, _capi.ROWS_ADAM_MAX_DIMS))
    if not isinstance(anchor_start, (bool, np.bool_)):
        raise ValueError("anchor_start must be True or False, got %r" % (anchor_start,))
    return as_int(n_iters, "n_iters", 0, 1 << 30), adam_options(lr, (0.9, 0.999), 1e-8, max_norm), cost_weights(weights)


def descent_state(state, P, basis, device):
    """The ``state`` a ``descend_motion`` returned, checked -> a copy of it on ``device``"""
    if not isinstance(state, dict) or set(state) != set(DESCENT_STATE_KEYS):
        raise ValueError("state must be the dict a descend_motion returned (keys %s)" % ", ".join(DESCENT_STATE_KEYS))
    n, D = basis.n_params, basis.n_dof
    out = {"iteration": as_int(state["iteration"], "state['iteration']", 0)}
    for k, shape in (("params", (P, n)), ("height", (P,))):
        t = state[k]
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError("state[%r] must be a float32 tensor of shape %s" % (k, shape))
        out[k] = t.to(device).clone().contiguous()
    a = state["anchor"]
    if a is not None and (not torch.is_tensor(a) or tuple(a.shape) != (P, D, 1) or a.dtype != torch.float32):
        raise ValueError("state['anchor'] must be None or a float32 tensor of shape %s" % ((P, D, 1),))
    out["anchor"] = None if a is None else a.to(device).clone().contiguous()
    out["adam"] = rows_adam_args(out["params"], out["params"], state["adam"], None, device)[2]
    return out


# ---------------------------------------------------------------------------------------------------- inverse kinematics
IK_MAX_ITERS = _capi.IK_MAX_ITERS


def motion_pose_args(trajectories, chain, jacobian, device):
    """The arguments of ``motion_pose`` -> (trajectories [N, T, n_dof], frames, axes, want_jacobian, was_numpy)."""
    if not isinstance(jacobian, (bool, np.bool_)):
        raise ValueError("jacobian must be True or False, got %r" % (jacobian,))
    t, frames, axes, was_np = motion_fk_args(trajectories, chain, device)
    return t, frames, axes, bool(jacobian), was_np


# ---------------------------------------------------------------------------------------------------- rigid-body dynamics
def chain_bodies(chain, device):
    """A ``KinematicChain`` with inertial data -> ``bodies [n_dof, 10]`` as a float32 tensor on ``device``, cached on the chain per
    device"""
    need_type(chain, KinematicChain, "chain")
    if not chain.has_inertia:
        raise ValueError("chain carries no inertial data for every moving link (mass, com, com_rpy, inertia): dynamics need them")
    key = ("device bodies", str(device))
    if key not in chain._cache:
        chain._cache[key] = torch.as_tensor(chain.bodies()).to(device)
    return chain._cache[key]


def _gravity3(gravity):
    try:
        g = np.array(gravity, dtype=np.float64)
    except (TypeError, ValueError):
        g = np.zeros(0)
    with np.errstate(over="ignore"):
        ok = g.shape == (3,) and np.isfinite(g).all() and np.isfinite(g.astype(np.float32)).all()
    if not ok:
        raise ValueError("gravity must be three finite numbers (m / s^2, base frame), got %r" % (gravity,))
    return tuple(float(x) for x in g.astype(np.float32))


def _step(dt, allow_none):
    if dt is None and allow_none:
        return None
    if not _is_number(dt) or not np.isfinite(dt) or not float(np.float32(dt)) > 0.0 or not np.isfinite(np.float32(dt)):
        raise ValueError("dt must be a finite number > 0 as float32, got %r" % (dt,))
    return float(np.float32(dt))


def motion_dynamics_args(trajectories, chain, velocities, accelerations, dt, gravity, inertia, device):
    """The arguments of ``motion_dynamics`` -> (trajectories [N, T, n_dof], velocities and accelerations (the same shape, or None),
    dt or None, frames, axes, bodies, gravity (three floats), effort limits [n_dof] on ``device`` or None, want_inertia,
    was_numpy).  ``dt`` asks for finite differences and goes with neither ``velocities`` nor ``accelerations``."""
    bodies = chain_bodies(chain, device)
    if not isinstance(inertia, (bool, np.bool_)):
        raise ValueError("inertia must be True or False, got %r" % (inertia,))
    t, frames, axes, was_np = motion_fk_args(trajectories, chain, device)
    dt = _step(dt, True)
    if dt is not None and (velocities is not None or accelerations is not None):
        raise ValueError("dt asks for finite differences of the trajectory: leave velocities and accelerations out with it")
    rest = []
    for x, name in ((velocities, "velocities"), (accelerations, "accelerations")):
        if x is not None:
            x = dev_block3(x, (int(t.shape[1]), chain.n_dof), device, name, rows=int(t.shape[0]))[0]
        rest.append(x)
    lim = chain.effort_limits
    if lim is not None:
        key = ("device effort", str(device))
        if key not in chain._cache:
            chain._cache[key] = to_device32(lim, device)
        lim = chain._cache[key]
    return t, rest[0], rest[1], dt, frames, axes, bodies, _gravity3(gravity), lim, bool(inertia), was_np


def motion_effort_args(trajectories, chain, dt, device):
    """The arguments of ``motion_effort`` -> (trajectories [N, T, n_dof], dt, frames, axes, bodies, was_numpy)"""
    bodies = chain_bodies(chain, device)
    t, frames, axes, was_np = motion_fk_args(trajectories, chain, device)
    return t, _step(dt, False), frames, axes, bodies, was_np


def ik_options(n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5):
    """The solver options of ``motion_ik`` checked -> (n_iters, tol, rot_tol, damping, max_step), the four numbers as the float32
    values the kernel uses.  The ranges are avae_motion_ik's."""
    n_iters = as_int(n_iters, "n_iters", 0, IK_MAX_ITERS)

    def number(v, name, positive):
        if not _is_number(v) or not np.isfinite(v) or not np.isfinite(np.float32(v)):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        v = float(np.float32(v))
        if (positive and not v > 0.0) or v < 0.0:
            raise ValueError("%s must be %s as float32, got %r" % (name, "> 0" if positive else ">= 0", v))
        return v
    return (n_iters, number(tol, "tol", False), number(rot_tol, "rot_tol", False), number(damping, "damping", True),
            number(max_step, "max_step", True))


def motion_ik_args(path, chain, seed, orientation, n_iters, tol, rot_tol, damping, max_step, limits, device):
    """The arguments of ``motion_ik`` -> (path [N, T, 3], frames, axes, seed [N, n_dof], orientation, limits [n_dof, 2] or None,
    options, was_numpy).  ``orientation`` comes back as None, a
    ``[1, 3, 3]`` or ``[N, 3, 3]`` tensor, or the string 'seed' where the seed is a device tensor (its pose is then taken on the
    device); a seed given as host data is folded here, in float64."""
    frames, axes = chain_matrices(chain, device)
    D = chain.n_dof
    p, was_np = dev_block3(path, (None, 3), device, "path")
    N = int(p.shape[0])
    if not 1 <= p.shape[1] <= _capi.MOTION_MAX_POINTS:
        raise ValueError("path must hold 1 to %d points, got %d" % (_capi.MOTION_MAX_POINTS, p.shape[1]))
    opts = ik_options(n_iters, tol, rot_tol, damping, max_step)
    if seed is None:
        raise ValueError("seed is None: the solver needs the angles to start from ([%d] or [%d, %d])" % (D, N, D))
    seed_on_host = not torch.is_tensor(seed)
    s = torch.as_tensor(np.asarray(seed, dtype=np.float64)) if seed_on_host else seed
    if tuple(s.shape) not in ((D,), (N, D)):
        raise ValueError("seed must be [%d] or [%d, %d], got %s" % (D, N, D, tuple(s.shape)))
    seed64 = s.numpy() if seed_on_host else None
    s = s.to(device=device, dtype=torch.float32)
    s = (s.reshape(1, D).expand(N, D) if s.dim() == 1 else s).contiguous()
    orient = None
    if isinstance(orientation, str):
        if orientation != "seed":
            raise ValueError("orientation must be None, 'seed', [3, 3] or [%d, 3, 3], got %r" % (N, orientation))
        if seed_on_host:
            rot = chain.pose(np.where(np.isfinite(seed64), seed64, 0.0))[1]
            orient = to_device32(rot.reshape(-1, 3, 3), device)
        else:
            orient = "seed"
    elif orientation is not None:
        o = orientation if torch.is_tensor(orientation) else torch.as_tensor(np.asarray(orientation, dtype=np.float32))
        if tuple(o.shape) not in ((3, 3), (N, 3, 3)):
            raise ValueError("orientation must be None, 'seed', [3, 3] or [%d, 3, 3], got shape %s" % (N, tuple(o.shape)))
        orient = o.to(device=device, dtype=torch.float32).reshape(-1, 3, 3).contiguous()
    return p, frames, axes, s, orient, _device_limits(chain, limits, device), opts, was_np


def _device_limits(chain, limits, device):
    """``limits``: True (the chain's own, if every joint has them), None / False or [n_dof, 2] -> float32 tensor on ``device``
    (cached on the chain) or None"""
    D = chain.n_dof
    lim = None
    if limits is True:
        lim = chain.limits
    elif limits is not None and limits is not False:
        lim = np.asarray(limits.cpu() if torch.is_tensor(limits) else limits, dtype=np.float64)
        if lim.shape != (D, 2) or np.isnan(lim).any() or (lim[:, 0] > lim[:, 1]).any():
            raise ValueError("limits must be True, None or [%d, 2] (lower <= upper), got %r" % (D, limits))
    if lim is not None:
        key = ("device limits", str(device), lim.tobytes())
        if key not in chain._cache:
            chain._cache[key] = to_device32(lim, device)
        lim = chain._cache[key]
    return lim


IK_OPTION_NAMES = ("orientation", "n_iters", "tol", "rot_tol", "damping", "max_step", "limits")
IK_DEFAULTS = dict(orientation=None, n_iters=20, tol=1e-5, rot_tol=1e-4, damping=0.01, max_step=0.5, limits=True)


def split_ik_options(options, also=()):
    """``**options`` of a composed call -> (motion_ik's own with their defaults filled in, the rest); a key that is neither an
    inverse-kinematics option nor one of ``also`` is refused."""
    extra = set(options) - set(IK_OPTION_NAMES) - set(also)
    if extra:
        raise ValueError("unknown option(s) %s (%s)" % (", ".join(sorted(map(str, extra))), ", ".join(IK_OPTION_NAMES + tuple(also))))
    ik = dict(IK_DEFAULTS)
    ik.update({k: v for k, v in options.items() if k in IK_OPTION_NAMES})
    return ik, {k: v for k, v in options.items() if k not in IK_OPTION_NAMES}


def strokes_to_motion_args(strokes, basis, chain, canvas, center, seed, height, options, device):
    """The arguments of ``strokes_to_motion`` -> (``motion_ik_args``' tuple for the lifted path [N, T, 3], was_numpy of the
    strokes).  The lift runs on the host in float64 and is
    rounded once."""
    _check_writer(basis, chain, canvas)
    s = np.asarray(strokes.cpu() if torch.is_tensor(strokes) else strokes, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 2 or not 1 <= s.shape[1] <= _capi.MOTION_MAX_POINTS:
        raise ValueError("strokes must be [N, T, 2] with T in [1, %d], got %s" % (_capi.MOTION_MAX_POINTS, s.shape))
    ik, _ = split_ik_options(options)
    path = np.ascontiguousarray(canvas.lift(s, center, height), dtype=np.float32)
    if basis.n_points != s.shape[1]:
        raise ValueError("basis.n_points = %d must be the strokes' %d points" % (basis.n_points, s.shape[1]))
    args = motion_ik_args(path, chain, seed, ik["orientation"], ik["n_iters"], ik["tol"], ik["rot_tol"], ik["damping"],
                          ik["max_step"], ik["limits"], device)
    return args[:-1], not torch.is_tensor(strokes)


SEARCH_OPTION_NAMES = ("eliteness", "weighting", "cov_update", "learning_rate", "covar_bounds", "tol_search", "seed")


def refine_pen_path_args(basis, chain, canvas, n_rollouts, options, widths, image_modality, modality):
    """``refine_pen_path``'s own arguments checked -> (motion_ik's options with their defaults, search's options).  The search's
    ``tol`` is spelled ``tol_search`` here: ``tol`` is the solver's."""
    _check_writer(basis, chain, canvas)
    as_index(image_modality, "image_modality", len(widths))
    as_index(modality, "modality", len(widths))
    _fits_pixels(canvas, image_modality, widths)
    _fits_params(basis, modality, widths)
    as_int(n_rollouts, "n_rollouts", 1)
    if np.linalg.matrix_rank(canvas.plane) < 3:
        raise ValueError("plane is singular: its rows u, v, n do not span the space")
    ik, rest = split_ik_options(options, SEARCH_OPTION_NAMES)
    ik_options(ik["n_iters"], ik["tol"], ik["rot_tol"], ik["damping"], ik["max_step"])
    search = {("tol" if k == "tol_search" else k): v for k, v in rest.items()}
    return ik, search


# ---------------------------------------------------------------------------------------------------- iLQR trajectory synthesis
TRACK_MAX_ITERS = _capi.TRACK_MAX_ITERS
TRACK_FACTOR, TRACK_LAM_MIN, TRACK_LAM_MAX = 10.0, 1e-6, 1e6           # the damping's schedule: motion_track does not expose it
TRACK_WORKSPACE_BYTES = 512 << 20                                      # the bound of motion_track's workspace (one row at least)
TRACK_DEFAULTS = dict(dt=0.01, track_weights=(10.0, 10.0, 50.0), effort_weight=0.01, effort=None, limits=True, limit_weight=0.0,
                      n_iters=25, lam0=1.0, tol=1e-6)
TRACK_OPTION_NAMES = tuple(TRACK_DEFAULTS)
SOLVERS = ("ik", "ilqr")


def track_options(dt=0.01, track_weights=(10.0, 10.0, 50.0), effort_weight=0.01, limit_weight=0.0, n_iters=25, lam0=1.0, tol=1e-6):
    """The solver options of ``motion_track`` checked -> (dt, (w0, w1, w2), effort_weight, limit_weight, n_iters, lam0, tol), the
    first four as the float32 values the kernel uses.  The ranges are avae_motion_track's."""
    dt = _ln_number(dt, "dt", True)
    try:
        w = tuple(track_weights)
    except TypeError:
        w = ()
    if len(w) != 3:
        raise ValueError("track_weights must be three numbers >= 0, got %r" % (track_weights,))
    w = tuple(_ln_number(v, "track_weights[%d]" % i, False) for i, v in enumerate(w))
    R = _ln_number(effort_weight, "effort_weight", False)
    wl = _ln_number(limit_weight, "limit_weight", False)
    n_iters = as_int(n_iters, "n_iters", 0, TRACK_MAX_ITERS)
    if not _is_number(lam0) or not TRACK_LAM_MIN <= float(lam0) <= TRACK_LAM_MAX:
        raise ValueError("lam0 must be a number in [%g, %g], got %r" % (TRACK_LAM_MIN, TRACK_LAM_MAX, lam0))
    if not _is_number(tol) or not np.isfinite(tol) or tol < 0:
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    return dt, w, R, wl, n_iters, float(lam0), float(tol)


def split_track_options(options):
    """``track_options`` of a composed call (None or a dict) -> motion_track's options with their defaults filled in; an unknown
    key is refused"""
    if options is None:
        options = {}
    if not isinstance(options, dict):
        raise ValueError("track_options must be None or a dict, got %r" % (type(options).__name__,))
    extra = set(options) - set(TRACK_OPTION_NAMES)
    if extra:
        raise ValueError("unknown option(s) %s (motion_track takes %s)" % (", ".join(sorted(map(str, extra))),
                                                                          ", ".join(TRACK_OPTION_NAMES)))
    return dict(TRACK_DEFAULTS, **options)


def check_solver(solver, options):
    """``solver`` and ``track_options`` of ``strokes_to_motion`` / ``refine_pen_path`` -> motion_track's options (checked) under
    'ilqr', None under 'ik'"""
    if solver not in SOLVERS:
        raise ValueError("solver must be 'ik' or 'ilqr', got %r" % (solver,))
    if solver == "ik":
        if options is not None:
            raise ValueError("track_options goes with solver='ilqr'")
        return None
    tr = split_track_options(options)
    track_options(tr["dt"], tr["track_weights"], tr["effort_weight"], tr["limit_weight"], tr["n_iters"], tr["lam0"], tr["tol"])
    return tr


def track_rows_per_call(T, D):
    """rows one avae_motion_track call takes under ``TRACK_WORKSPACE_BYTES`` (the plan's bytes per row: avae_motion_track_plan)"""
    per_row = (T * (10 * D * D + 58 * D) + 255) // 256 * 256
    return max(1, TRACK_WORKSPACE_BYTES // per_row), per_row


def motion_track_args(path, chain, init, dt, track_weights, effort_weight, effort, limits, limit_weight, n_iters, lam0, tol, device):
    """The arguments of ``motion_track`` but the first guess's own -> (path [N, T, 3], frames, axes, init [N, T, n_dof] or None,
    effort [n_dof, n_dof] or None, limits [n_dof, 2] or None, options, was_numpy)."""
    frames, axes = chain_matrices(chain, device)
    D = chain.n_dof
    p, was_np = dev_block3(path, (None, 3), device, "path")
    N, T = int(p.shape[0]), int(p.shape[1])
    if not 1 <= T <= _capi.MOTION_MAX_POINTS:
        raise ValueError("path must hold 1 to %d points, got %d" % (_capi.MOTION_MAX_POINTS, T))
    opts = track_options(dt, track_weights, effort_weight, limit_weight, n_iters, lam0, tol)
    q0 = None if init is None else dev_block3(init, (T, D), device, "init", rows=N)[0]
    E = None
    if effort is not None:
        E = effort if torch.is_tensor(effort) else torch.as_tensor(np.asarray(effort, dtype=np.float32))
        if tuple(E.shape) != (D, D) or not bool(torch.isfinite(E.to(torch.float32)).all()):
            raise ValueError("effort must be a finite [%d, %d] matrix, got shape %s" % (D, D, tuple(E.shape)))
        E = E.to(device=device, dtype=torch.float32).contiguous()
    return p, frames, axes, q0, E, _device_limits(chain, limits, device), opts, was_np


# ---------------------------------------------------------------------------------------------------- sigma-lognormal strokes
LN_MAX_C, LN_MAX_T, LN_MAX_ITERS = _capi.LOGNORMAL_MAX_COMPONENTS, _capi.LOGNORMAL_MAX_POINTS, _capi.LOGNORMAL_MAX_ITERS


def _ln_number(v, name, positive):
    """a finite float32 number, > 0 (``positive``) or >= 0 -> the float32 value as a float"""
    if not _is_number(v) or not np.isfinite(v) or not np.isfinite(np.float32(v)):
        raise ValueError("%s must be a finite number, got %r" % (name, v))
    v32 = float(np.float32(v))
    if (positive and not v32 > 0.0) or v32 < 0.0:
        raise ValueError("%s must be %s as float32, got %r" % (name, "> 0" if positive else ">= 0", v))
    return v32


def _ln_dt(dt, T):
    if dt is None:
        if T == 1:
            raise ValueError("dt is None and there is one time point: the default 1 / (T - 1) needs T >= 2")
        dt = 1.0 / (T - 1)
    return _ln_number(dt, "dt", True)


def _ln_params(params, count, device, name="params"):
    """params [N, C, 6] and count (None or [N] integers in [0, C]) -> (float32 tensor, int32 tensor [N], was_numpy)"""
    if params is None:
        raise ValueError("%s is None" % name)
    p, was_np = dev_block3(params, (None, 6), device, name)
    N, Cn = int(p.shape[0]), int(p.shape[1])
    if not 1 <= Cn <= LN_MAX_C:
        raise ValueError("%s must hold 1 to %d components (C), got %d" % (name, LN_MAX_C, Cn))
    if count is None:
        cnt = torch.full((N,), Cn, dtype=torch.int32, device=device)
    else:
        c = count if torch.is_tensor(count) else torch.as_tensor(np.asarray(count))
        if c.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError("count must hold integers, got %s" % c.dtype)
        if tuple(c.shape) != (N,):
            raise ValueError("count must be [%d] (one per row of %s), got %s" % (N, name, tuple(c.shape)))
        if N and (int(c.min()) < 0 or int(c.max()) > Cn):
            raise ValueError("count must lie in [0, C = %d], got %d .. %d" % (Cn, int(c.min()), int(c.max())))
        cnt = c.to(device=device, dtype=torch.int32).contiguous()
    return p, cnt, was_np


def _ln_start(start, N, device, default=None):
    """start None (``default`` [N, 2] or the origin), [2] or [N, 2] -> float32 tensor [N, 2]"""
    if start is None:
        return torch.zeros((N, 2), dtype=torch.float32, device=device) if default is None else default.contiguous()
    s = start if torch.is_tensor(start) else torch.as_tensor(np.asarray(start, dtype=np.float32))
    if tuple(s.shape) not in ((2,), (N, 2)):
        raise ValueError("start must be [2] or [%d, 2], got %s" % (N, tuple(s.shape)))
    s = s.to(device=device, dtype=torch.float32)
    return (s.reshape(1, 2).expand(N, 2) if s.dim() == 1 else s).contiguous()


def _ln_strokes(strokes, device):
    s, was_np = dev_block3(strokes, (None, 2), device, "strokes")
    if not 1 <= s.shape[1] <= LN_MAX_T:
        raise ValueError("strokes must hold 1 to %d points (T), got %d" % (LN_MAX_T, s.shape[1]))
    return s, was_np


def lognormal_eval_args(params, n_points, count, start, dt, device):
    """The arguments of ``lognormal_eval`` -> (params [N, C, 6], count [N] int32, start [N, 2], T, dt, was_numpy)"""
    p, cnt, was_np = _ln_params(params, count, device)
    T = as_int(n_points, "n_points", 1, LN_MAX_T)
    return p, cnt, _ln_start(start, int(p.shape[0]), device), T, _ln_dt(dt, T), was_np


def lognormal_sample_options(n_samples, seed, amplitude, angle, straightness):
    """-> (S, seed, amplitude, angle, straightness), the three scales as the float32 values the kernel uses"""
    return (as_int(n_samples, "n_samples", 1, 1 << 20), as_int(seed, "seed", 0, (1 << 64) - 1),
            _ln_number(amplitude, "amplitude", False), _ln_number(angle, "angle", False),
            _ln_number(straightness, "straightness", False))


def lognormal_fit_args(strokes, init, count, start, dt, max_components, n_iters, weights, free, bounds, tol, device):
    """The arguments of ``lognormal_fit`` -> (strokes [N, T, 2], init [N, C, 6], count [N] int32, start [N, 2], dt, (n_iters, wp,
    wv, tol), free (None or a uint8 tensor [6] or [N, C, 6]), lo, hi (None or float32 [6]), was_numpy).  ``init=None`` runs
    ``lognormal_initial_guess`` on the host: the strokes are read back for it."""
    from .lognormal import lognormal_initial_guess
    if strokes is None:
        raise ValueError("strokes is None")
    s, was_np = _ln_strokes(strokes, device)
    N, T = int(s.shape[0]), int(s.shape[1])
    dt32 = _ln_dt(dt, T)
    st = _ln_start(start, N, device, default=s[:, 0, :])
    n_iters = as_int(n_iters, "n_iters", 0, LN_MAX_ITERS)
    if not isinstance(weights, (tuple, list)) or len(weights) != 2 or not all(_is_number(w) and np.isfinite(w) and w >= 0 for w in weights):
        raise ValueError("weights must be (position, velocity), two finite numbers >= 0, got %r" % (weights,))
    if not _is_number(tol) or not np.isfinite(tol) or tol < 0:
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    if init is None:
        if count is not None:
            raise ValueError("count goes with init: the initial guess finds its own")
        as_int(max_components, "max_components", 1, LN_MAX_C)
        guess, cnt = lognormal_initial_guess(s.cpu().numpy(), st.cpu().numpy(), dt32, max_components=max_components)
        p, cnt, _ = _ln_params(guess.astype(np.float32), cnt, device, "init")
    else:
        p, cnt, _ = _ln_params(init, count, device, "init")
        if p.shape[0] != N:
            raise ValueError("init must hold the strokes' %d rows, got %d" % (N, p.shape[0]))
    Cn = int(p.shape[1])
    fr = None
    if free is not None:
        f = free if torch.is_tensor(free) else torch.as_tensor(np.asarray(free))
        if tuple(f.shape) not in ((6,), (N, Cn, 6)):
            raise ValueError("free must be None, [6] or [%d, %d, 6], got %s" % (N, Cn, tuple(f.shape)))
        fr = (f != 0).to(device=device, dtype=torch.uint8).contiguous()
    lo = hi = None
    if bounds is not None:
        if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
            raise ValueError("bounds must be None or (lo, hi), each None or [6]")
        out = []
        for name, b in zip(("lo", "hi"), bounds):
            if b is None:
                out.append(None)
                continue
            b = np.asarray(b.cpu() if torch.is_tensor(b) else b, dtype=np.float64)
            if b.shape != (6,) or np.isnan(b).any():
                raise ValueError("bounds: %s must be [6] without NaN (an infinity leaves a parameter unbounded), got %r" % (name, b))
            out.append(b)
        if out[0] is not None and out[1] is not None and (out[0] > out[1]).any():
            raise ValueError("bounds: lo must be <= hi")
        lo, hi = (None if b is None else to_device32(b, device) for b in out)
    return s, p, cnt, st, dt32, (n_iters, float(weights[0]), float(weights[1]), float(tol)), fr, lo, hi, was_np


def lognormal_augment_args(strokes, params, count, start, dt, n_points, device):
    """Which way ``lognormal_augment`` goes: exactly one of ``strokes`` (fit first) and ``params`` (given components, with
    ``n_points``) -> 'strokes' or 'params'"""
    if (strokes is None) == (params is None):
        raise ValueError("give exactly one of strokes (fitted first) and params (perturbed as they are), got %s"
                         % ("both" if strokes is not None else "neither"))
    if params is not None and n_points is None:
        raise ValueError("params needs n_points: the number of time points to evaluate")
    return "strokes" if strokes is not None else "params"
