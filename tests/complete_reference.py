"""NumPy restatement of ``complete`` (include/avae.h: avae_complete), fp64 by default.

Per row n independently:  J_n(z) = sum_m w_m recon_obs_m(x[n,m], dec_m(z), o[n,m]) + prior_weight * 0.5 |z|^2, minimised by
``n_iters`` steps of per-row, per-element textbook Adam (bias-corrected, zero moments at the start) on z.

The forward pass is the oracle's ``decode`` (imported, not copied).  The oracle has no standalone decoder input gradient -- its
``backward`` is the whole training step -- so the chain is written here from decode's cache: output gradient on the observed
elements, ``dlogits @ Wout^T``, ``act'(pre)`` per layer, down to dz.  ``quant='bf16'`` puts the kernels' rounding points in
(decode's own, plus every stored activation gradient; transfer-function derivatives from the stored output), ``masks`` hands
over relu decisions as ``oracle.backward`` takes them.  ``dtype=np.float32`` runs the same arithmetic in float32 (the rounding
amplification of the Adam trajectory is measured with it); the bias corrections 1 - b^t are then formed in double and rounded
once, as the kernel forms them."""
import numpy as np

from oracle import vae_assoc_oracle as O

# the model's config: TF-1 AdamOptimizer defaults as the float32 values the library holds
BETA1, BETA2, ADAM_EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))


def recon_obs(x, xhat, o, binary):
    """avae_score's per-row reconstruction terms summed over the observed elements only -> [rows].  Unobserved elements are
    selected away (np.where), never multiplied by 0."""
    o = np.asarray(o) != 0
    xm = np.where(o, x, 0)
    if binary:
        t = -(xm * np.log(1e-3 + xhat) + (1 - xm) * np.log(1e-3 + 1 - xhat))
    else:
        t = (xm - xhat) ** 2 / 2
    return np.sum(np.where(o, t, 0), axis=1)


def objective_and_grad(archs, params, X, observed, z, binary, weights, act, prior_weight, quant=None, masks=None):
    """-> (J [rows], dJ/dz [rows, n_z], decoder outputs [per modality]).  ``X[m]`` None = modality m unobserved,
    ``observed[m]`` None = fully observed; ``masks[m]["dec"][i]`` = relu decisions of another run of the same forward pass."""
    q = O._q(quant)
    dt = z.dtype
    J = prior_weight * 0.5 * np.sum(z * z, axis=1)
    g = prior_weight * z
    outs = []
    for m, (na, p, b, w) in enumerate(zip(archs, params, binary, weights)):
        xhat, cache = O.decode(na, p, z, act, b, quant)
        outs.append(xhat)
        if X[m] is None:
            continue
        o = np.ones(X[m].shape, bool) if observed is None or observed[m] is None else np.asarray(observed[m]) != 0
        xm = np.where(o, X[m], 0).astype(dt)
        J = J + w * recon_obs(xm, xhat, o, b)
        if b:       # d/dlogit of -(x log(1e-3+p) + (1-x) log(1e-3+1-p)), p = sigmoid(logit): the 1e-3 stays inside the log
            dl = xhat * (1 - xhat) * (-xm / (1e-3 + xhat) + (1 - xm) / (1e-3 + 1 - xhat))
        else:
            dl = xhat - xm
        dg = q(w * np.where(o, dl, 0)).astype(dt)
        L = len(O.hidden_sizes(na))
        acts, pre = cache["acts"], cache["pre"]
        dg = dg @ q(p["dec_Wout"]).T.astype(dt)
        for i in range(L - 1, -1, -1):
            if masks is not None:
                d_i = np.asarray(masks[m]["dec"][i], dtype=dt)
            elif quant is None:
                d_i = O.ACT[act][1](pre[i], acts[i + 1])
            else:
                d_i = O.DACT_FROM_OUTPUT[act](acts[i + 1])
            da = q(dg * d_i).astype(dt)
            dg = da @ q(p["dec_W%d" % (i + 1)]).T.astype(dt)
        g = g + dg
    return J, g, outs


def adam_update(z, m, v, g, t, lr, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """one textbook Adam step with bias correction, in z's dtype -> (z, m, v)"""
    dt = z.dtype.type
    m = dt(b1) * m + (dt(1) - dt(b1)) * g
    v = dt(b2) * v + (dt(1) - dt(b2)) * (g * g)
    c1, c2 = dt(1.0 - b1 ** t), dt(1.0 - b2 ** t)
    z = z - dt(lr) * (m / c1) / (np.sqrt(v / c2) + dt(eps))
    return z, m, v


def complete(archs, params_flat, X, observed, z0, binary, weights, act, n_iters, lr, prior_weight=1.0, quant=None,
             dtype=np.float64, masks0=None):
    """-> dict(z, x, objective [n_iters+1, rows], grad0).  ``masks0``: relu decisions for the FIRST gradient only."""
    params = O.unflatten_params(archs, np.asarray(params_flat, dtype=dtype), dtype)
    X = [None if x is None else np.asarray(x, dtype=dtype) for x in X]
    z = np.asarray(z0, dtype=dtype).copy()
    pw = dtype(prior_weight)
    w = [dtype(wm) for wm in weights]
    m, v = np.zeros_like(z), np.zeros_like(z)
    obj, grad0 = [], None
    for t in range(n_iters + 1):
        J, g, outs = objective_and_grad(archs, params, X, observed, z, binary, w, act, pw, quant, masks0 if t == 0 else None)
        obj.append(J)
        if t == 0:
            grad0 = g
        if t < n_iters:
            z, m, v = adam_update(z, m, v, g, t + 1, lr)
    return {"z": z, "x": outs, "objective": np.stack(obj), "grad0": grad0}
