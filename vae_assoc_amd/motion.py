"""The motion layer's host side: the basis of the reference's function approximator (pyrbf_funcapprox.py) as matrices.

A joint-modality row holds ``n_dof * (n_basis + 1)`` parameters: per joint ``n_basis`` basis weights and one constant offset
(baxter_writer.py:53-82), standardised with the data set's mean and standard deviation (baxter_vae_assoc_writer.py:109-111).
``MotionBasis`` turns the basis into the dense matrices the device calls take (avae_motion_eval / _fit / _moments in
include/avae.h): the features at the phase points, the truncated-SVD pseudo-inverse of the fit and the two
matrices of a linear equality constraint.  Everything here is NumPy float64 and needs no GPU."""
import numpy as np

from ._capi import MOTION_MAX_ANCHORS as MAX_ANCHORS, MOTION_MAX_DOF as MAX_DOF, MOTION_MAX_KB as MAX_KB, MOTION_MAX_POINTS as MAX_POINTS


def _whole(x, name, lo):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, x))
    return int(x)


class MotionBasis(object):
    """``kind`` 'sigmoid' or 'gaussian' with ``n_basis`` functions and a trailing constant-1 column; ``n_dof`` joints evaluated at
    ``n_points`` phase points; ``normalize`` divides a gaussian row by its sum; ``limits`` [n_dof, 2] (lower, upper) or None;
    ``param_mean`` / ``param_std`` [n_params] or None: what ``dataset.extract_jnt_fa_parms`` returns."""

    def __init__(self, kind="sigmoid", n_basis=20, n_dof=7, n_points=100, normalize=True, limits=None, param_mean=None,
                 param_std=None):
        if kind not in ("sigmoid", "gaussian"):
            raise ValueError("kind must be 'sigmoid' or 'gaussian', got %r" % (kind,))
        self.kind = kind
        self.n_basis = _whole(n_basis, "n_basis", 0)
        self.n_dof = _whole(n_dof, "n_dof", 1)
        self.n_points = _whole(n_points, "n_points", 1)
        self.normalize = bool(normalize)
        if self.n_basis + 1 > MAX_KB:
            raise ValueError("n_basis + 1 = %d must be <= %d" % (self.n_basis + 1, MAX_KB))
        if self.n_dof > MAX_DOF:
            raise ValueError("n_dof = %d must be <= %d" % (self.n_dof, MAX_DOF))
        if self.n_points > MAX_POINTS:
            raise ValueError("n_points = %d must be <= %d" % (self.n_points, MAX_POINTS))
        self.n_kb = self.n_basis + 1
        self.n_params = self.n_dof * self.n_kb
        self.limits = None
        if limits is not None:
            lim = np.array(limits, dtype=np.float64)
            if lim.shape != (self.n_dof, 2):
                raise ValueError("limits must be [%d, 2] (lower, upper), got %s" % (self.n_dof, lim.shape))
            if np.isnan(lim).any():
                raise ValueError("limits must not hold NaN")
            self.limits = lim

        def vec(a, name):
            if a is None:
                return None
            v = np.array(a, dtype=np.float64)
            if v.shape != (self.n_params,):
                raise ValueError("%s must be [%d] (n_dof * (n_basis + 1)), got %s" % (name, self.n_params, v.shape))
            if not np.isfinite(v).all():
                raise ValueError("%s must be finite" % name)
            return v
        self.param_mean = vec(param_mean, "param_mean")
        self.param_std = vec(param_std, "param_std")
        if self.param_std is not None and (self.param_std == 0).any():
            raise ValueError("param_std must not hold a zero")
        self._cache = {}

    # ---- the features (pyrbf_funcapprox.py:26-39 the centres and widths, :72-102 the evaluation)
    def features(self, z):
        """[len(z), n_basis + 1]: the basis functions at the phases ``z`` and the constant column"""
        z = np.atleast_1d(np.asarray(z, dtype=np.float64))
        if z.ndim != 1:
            raise ValueError("z must be one-dimensional, got shape %s" % (z.shape,))
        key = ("features", z.tobytes())
        if key not in self._cache:
            K = self.n_basis
            if K == 0:
                f = np.zeros((len(z), 0))
            elif self.kind == "sigmoid":
                t0 = np.linspace(1.0 / K, 1.0, K)                                  # :35
                f = 1.0 / (1.0 + np.exp(-(2.0 * K) * (z[:, None] - t0[None, :])))  # :34 tau = 2K, :76-78
            else:
                mu = np.linspace(0.1, 0.9, K)                                      # :30
                f = np.exp(-(z[:, None] - mu[None, :]) ** 2 / (1.0 / K))           # :31 sigma = 1/K, :72-74
                if self.normalize:
                    f = f / f.sum(1, keepdims=True)                                # :92-93
            self._cache[key] = np.concatenate([f, np.ones((len(z), 1))], axis=1)   # :94, :97
        return self._cache[key].copy()

    def phases(self, T=None):
        T = self.n_points if T is None else _whole(T, "T", 1)
        if T > MAX_POINTS:
            raise ValueError("T = %d must be <= %d" % (T, MAX_POINTS))
        return np.linspace(0.0, 1.0, T)

    def pinv(self, T=None):
        """[n_basis + 1, T]: the pseudo-inverse of the fit (pyrbf_funcapprox.py:104-121), singular values <= 1e-6 dropped"""
        T = self.n_points if T is None else T
        z = self.phases(T)
        key = ("pinv", len(z))
        if key not in self._cache:
            U, s, Vt = np.linalg.svd(self.features(z), full_matrices=False)        # features [T, Kb] = U s Vt
            n = int((s > 1e-6).sum())
            self._cache[key] = (Vt[:n].T / s[:n]) @ U[:, :n].T
        return self._cache[key].copy()

    def constraint(self, phases):
        """-> (A [Kb, Kb], B [Kb, n_c]): the projection of pyrbf_funcapprox.py:41-61 onto ``features(phases) theta == target`` is
        ``theta -> A theta + B target``"""
        ph = np.atleast_1d(np.asarray(phases, dtype=np.float64))
        if ph.ndim != 1 or not 1 <= len(ph) <= MAX_ANCHORS:
            raise ValueError("phases must hold 1 to %d phase points, got shape %s" % (MAX_ANCHORS, ph.shape))
        if not np.isfinite(ph).all():
            raise ValueError("phases must be finite")
        key = ("constraint", ph.tobytes())
        if key not in self._cache:
            F = self.features(ph).T                                                # [Kb, n_c], :55
            B = F @ np.linalg.pinv(F.T @ F)                                        # :56
            self._cache[key] = (np.eye(self.n_kb) - B @ F.T, B)                    # :59-60
        A, B = self._cache[key]
        return A.copy(), B.copy()

    def projection(self, phases, target):
        """``constraint(phases)`` in the standardised space, per joint: -> (A [n_dof, Kb, Kb], b [rows, n_params]) in float64
        with  s' = A[d] s + b[:, d]  the standardised parameters of joint d whose raw values theta = s * param_std + param_mean
        are the projection of the raw s onto ``features(phases) theta == target[:, d]`` -- what ``search`` takes as ``project``
        (pyrbf_funcapprox.py:163-171 samples under the constraint this way).  ``target`` is [rows, n_dof, n_c]."""
        A, B = self.constraint(phases)
        t = np.asarray(target, dtype=np.float64)
        if t.ndim != 3 or t.shape[1:] != (self.n_dof, B.shape[1]):
            raise ValueError("target must be [rows, %d, %d], got %s" % (self.n_dof, B.shape[1], t.shape))
        std = np.ones(self.n_params) if self.param_std is None else self.param_std
        mean = np.zeros(self.n_params) if self.param_mean is None else self.param_mean
        std, mean = std.reshape(self.n_dof, self.n_kb), mean.reshape(self.n_dof, self.n_kb)
        As = A[None, :, :] * std[:, None, :] / std[:, :, None]
        b = (np.einsum("jk,dk->dj", A, mean)[None] + np.einsum("jc,rdc->rdj", B, t) - mean[None]) / std[None]
        return As, b.reshape(t.shape[0], self.n_params)

    # ---- what the device calls take
    def scale_shift(self):
        """(param_std or None, param_mean or None) as float32: theta = params * scale + shift"""
        sc = None if self.param_std is None else self.param_std.astype(np.float32)
        sh = None if self.param_mean is None else self.param_mean.astype(np.float32)
        return sc, sh

    def eval_matrices(self, anchor_phases=None, T=None):
        """-> (phi [T, Kb], anchor_gain [T, n_c] or None) in float64: with a constraint phi is ``features @ A`` and the gain
        ``features @ B``, so that the device evaluates the projected parameters without knowing of the constraint"""
        F = self.features(self.phases(T))
        if anchor_phases is None:
            return F, None
        A, B = self.constraint(anchor_phases)
        return F @ A, F @ B
