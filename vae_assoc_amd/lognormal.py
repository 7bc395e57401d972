"""Host side of the sigma-lognormal stroke model: the first guess a fit starts from and the sample counts
that balance a labelled set.  NumPy only, no GPU; the model itself, its sampler and its fit are device calls
(``AssocVariationalAutoEncoder.lognormal_eval`` / ``lognormal_augment`` / ``lognormal_fit``).

A component is ``(D, t0, mu, sigma, theta_s, theta_e)``: a lognormal speed pulse of area ``D`` that switches on at ``t0``, with
log-time mean ``mu`` and width ``sigma``, whose direction turns from ``theta_s`` to ``theta_e``."""
from collections import Counter

import numpy as np

PARAM_NAMES = ("D", "t0", "mu", "sigma", "theta_s", "theta_e")
MAX_COMPONENTS, MAX_POINTS = 16, 1024


def stroke_velocity(strokes, start, dt):
    """Finite-difference velocity of ``strokes [N, T, 2]``: ``V_0 = (P_0 - start) / dt``, ``V_k = (P_k - P_(k-1)) / dt``"""
    prev = np.concatenate([start[:, None, :], strokes[:, :-1, :]], axis=1)
    return (strokes - prev) / dt


def _check_strokes(strokes, start, dt):
    s = np.asarray(strokes, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 2 or not 1 <= s.shape[1] <= MAX_POINTS:
        raise ValueError("strokes must be [N, T, 2] with T in [1, %d], got %s" % (MAX_POINTS, s.shape))
    N, T = s.shape[0], s.shape[1]
    if dt is None:
        if T == 1:
            raise ValueError("dt is None and the strokes hold one point: 1 / (T - 1) needs T >= 2")
        dt = 1.0 / (T - 1)
    if isinstance(dt, (bool, np.bool_)) or not isinstance(dt, (int, float, np.integer, np.floating)) or not (np.isfinite(dt) and dt > 0):
        raise ValueError("dt must be a finite number > 0, got %r" % (dt,))
    st = s[:, 0, :].copy() if start is None else np.asarray(start, dtype=np.float64)
    if st.shape == (2,):
        st = np.broadcast_to(st, (N, 2)).copy()
    if st.shape != (N, 2):
        raise ValueError("start must be [2] or [%d, 2], got %s" % (N, st.shape))
    return s, st, float(dt)


def lognormal_initial_guess(strokes, start=None, dt=None, max_components=8, sigma=0.3, floor=0.1):
    """A first guess of the components of ``strokes [N, T, 2]`` from the peaks of their speed -> (``params [N, max_components,
    6]`` zero-padded, ``count [N]`` int32).  The project's own, much simpler stand-in for the reference's ``rxzero_sig_extract`` /
    ``vel_profile_registration``.

    The speed ``|V_k|`` is smoothed by ``(1/4, 1/2, 1/4)`` with edge padding; its local maxima of at least ``floor`` times the
    largest are kept, the ``max_components`` highest of them, in time order.  From a peak at ``i`` both flanks are walked down
    while the speed falls and stays above 2 % of the peak's, to ``a`` and ``b``; then, with ``delta = max(b - a, 2) dt``:
    ``mu = ln(delta / (e^(3 sigma) - e^(-3 sigma)))``, ``t0 = i dt - exp(mu - sigma^2)`` (the pulse's mode at the peak),
    ``D = speed_i sigma sqrt(2 pi) exp(mu - sigma^2 / 2)`` (the mode's height is the peak's) and ``theta_s``, ``theta_e`` the
    unwrapped direction angle at ``a`` and ``b``.  ``start`` defaults to each stroke's first point, ``dt`` to ``1 / (T - 1)``."""
    s, st, dt = _check_strokes(strokes, start, dt)
    if isinstance(max_components, (bool, np.bool_)) or not isinstance(max_components, (int, np.integer)) \
            or not 1 <= max_components <= MAX_COMPONENTS:
        raise ValueError("max_components must be an integer in [1, %d], got %r" % (MAX_COMPONENTS, max_components))
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0, got %r" % (sigma,))
    if not (np.isfinite(floor) and 0 <= floor <= 1):
        raise ValueError("floor must be in [0, 1], got %r" % (floor,))
    N, T = s.shape[0], s.shape[1]
    params = np.zeros((N, int(max_components), 6))
    count = np.zeros(N, dtype=np.int32)
    V = stroke_velocity(s, st, dt)
    width = np.exp(3.0 * sigma) - np.exp(-3.0 * sigma)
    for n in range(N):
        if not np.isfinite(V[n]).all():
            continue
        raw = np.hypot(V[n, :, 0], V[n, :, 1])
        pad = np.concatenate([raw[:1], raw, raw[-1:]])
        sp = 0.25 * pad[:-2] + 0.5 * pad[1:-1] + 0.25 * pad[2:]
        top = sp.max()
        if not top > 0:
            continue
        left = np.concatenate([[-np.inf], sp[:-1]])
        right = np.concatenate([sp[1:], [-np.inf]])
        peaks = np.nonzero((sp > left) & (sp >= right) & (sp >= floor * top))[0]
        if len(peaks) > max_components:
            keep = np.argsort(-sp[peaks], kind="stable")[:max_components]
            peaks = np.sort(peaks[keep])
        ang = np.unwrap(np.arctan2(V[n, :, 1], V[n, :, 0]))
        for c, i in enumerate(peaks):
            a = b = int(i)
            while a > 0 and sp[a - 1] < sp[a] and sp[a - 1] > 0.02 * sp[i]:
                a -= 1
            while b < T - 1 and sp[b + 1] < sp[b] and sp[b + 1] > 0.02 * sp[i]:
                b += 1
            delta = max(b - a, 2) * dt
            mu = np.log(delta / width)
            params[n, c] = (sp[i] * sigma * np.sqrt(2.0 * np.pi) * np.exp(mu - 0.5 * sigma * sigma), i * dt - np.exp(mu - sigma * sigma),
                            mu, sigma, ang[a], ang[b])
        count[n] = len(peaks)
    return params, count


def balanced_sample_counts(labels, per_class=100):
    """The reference's ``int(sample_per_char / (len + 1))`` (utils.py:320): how many perturbed samples every recorded stroke of a
    labelled set gets so that each class ends near ``per_class`` rows -> int array ``[N]``, one count per label (0 for a class
    that already holds ``per_class`` strokes or more: the reference keeps those as they are)."""
    if isinstance(per_class, (bool, np.bool_)) or not isinstance(per_class, (int, np.integer)) or per_class < 0:
        raise ValueError("per_class must be an integer >= 0, got %r" % (per_class,))
    labels = list(labels)
    sizes = Counter(labels)
    return np.array([int(per_class / (sizes[l] + 1)) for l in labels], dtype=np.int64)
