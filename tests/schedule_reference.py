"""fp64 statement of the on-device training schedules (include/avae.h, avae_set_schedule).

Per training step, with t the step number the update gets and u = t - 1:

    cost_t   = sum_m w_m [ kl_t * latent_m + recon_m ] + lambda_t * sum_pairs assoc
    lambda_t = fl32(assoc_lambda * a_t),  lr_eff_t = fl32(learning_rate * l_t)

``schedule_value`` restates the three kinds of schedule; ``scheduled_cost`` is the cost in torch fp64 (autograd supplies the
gradient) after tests/test_oracle.py::torch_cost, with ``kl`` on the KL term only and ``batch_global`` honoured -- the oracle's
``backward`` folds KL and reconstruction under one weight and cannot separate them; ``scheduled_step`` applies the oracle's
``adam_step`` with lr_eff_t."""
import itertools

import numpy as np
import torch

from oracle import vae_assoc_oracle as O

F32 = np.float32


def schedule_value(spec, t):
    """Multiplier of schedule ``spec`` (None, a number, dict(knots=, period=) or dict(decay_rate=, decay_steps=, staircase=)) at
    step number t >= 1, as np.float32.  Python floats are IEEE doubles and nothing is contracted, so the piecewise value is the
    library's to the bit; EXP goes through the platform's pow."""
    u = int(t) - 1
    if spec is None:
        return F32(1.0)
    if not isinstance(spec, dict):
        return F32(spec)
    if "knots" in spec:
        knots = [(int(s), float(F32(v))) for s, v in spec["knots"]]
        period = spec.get("period") or 0
        if period > 0:
            u %= period
        if u <= knots[0][0]:
            return F32(knots[0][1])
        if u >= knots[-1][0]:
            return F32(knots[-1][1])
        for (s0, v0), (s1, v1) in zip(knots[:-1], knots[1:]):
            if s0 <= u < s1:
                return F32(v0 + (v1 - v0) * (float(u - s0) / float(s1 - s0)))
        raise AssertionError("unreachable")
    rate, steps = float(F32(spec["decay_rate"])), int(spec["decay_steps"])
    e = float(u // steps) if spec.get("staircase") else float(u) / float(steps)
    return F32(rate ** e)


def hyper(kl, assoc, lr, lam, learning_rate, t):
    """(kl_t, lambda_t, lr_eff_t) of step t as fp32: the products with the configured values are fp32 products."""
    return (schedule_value(kl, t), F32(lam) * schedule_value(assoc, t), F32(learning_rate) * schedule_value(lr, t))


def ulp_distance(a, b):
    """distance of two finite positive fp32 values in units in the last place"""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def scheduled_cost(archs, flat, X, eps, binary, weights, lam, act, kl=1.0, batch_global=None, masks=None):
    """cost_t of the module docstring in torch fp64 (reference vae_assoc.py:163-222,243-304,306-371).  ``lam`` is lambda_t.
    ``masks`` (conftest.hip_relu_masks): the relu decisions to take instead of the sign of the pre-activation."""
    f = {"relu": torch.relu, "softplus": torch.nn.functional.softplus, "tanh": torch.tanh,
         "sigmoid": torch.sigmoid, "identity": lambda a: a}[act]

    def apply(a, mask):
        return f(a) if mask is None else a * torch.as_tensor(mask, dtype=a.dtype)
    off = 0
    mus, lvs = [], []
    cost = 0.0
    n_z = archs[0]["n_z"]
    Bg = X[0].shape[0] if batch_global is None else batch_global
    for m, (na, x, b, w) in enumerate(zip(archs, X, binary, weights)):
        p = {}
        for name, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            p[name] = flat[off:off + n].reshape(shp)
            off += n
        L = len(O.hidden_sizes(na))
        h = x
        for i in range(L):
            h = apply(h @ p["enc_W%d" % (i + 1)] + p["enc_b%d" % (i + 1)], None if masks is None else masks[m]["enc"][i])
        mu = h @ p["enc_Wmu"] + p["enc_bmu"]
        lv = h @ p["enc_Wsig"] + p["enc_bsig"]
        z = mu + torch.sqrt(torch.exp(lv)) * eps
        g = z
        for i in range(L):
            g = apply(g @ p["dec_W%d" % (i + 1)] + p["dec_b%d" % (i + 1)], None if masks is None else masks[m]["dec"][i])
        a = g @ p["dec_Wout"] + p["dec_bout"]
        k = torch.sum(-0.5 * torch.sum(1 + lv - mu ** 2 - torch.exp(lv), 1))
        if b:
            xr = torch.sigmoid(a)
            r = torch.sum(-torch.sum(x * torch.log(1e-3 + xr) + (1 - x) * torch.log(1e-3 + 1 - xr), 1)) / Bg
        else:
            r = torch.sum((x - a) ** 2) / 2
        cost = cost + w * (kl * k / Bg + r)
        mus.append(mu)
        lvs.append(lv)
    for i, j in itertools.combinations(range(len(archs)), 2):
        a1 = torch.sum(0.5 * (lvs[j].sum(1) - lvs[i].sum(1) - n_z + torch.exp(lvs[i] - lvs[j]).sum(1)
                              + ((mus[j] - mus[i]) ** 2 * torch.exp(-lvs[j])).sum(1)))
        a2 = torch.sum(0.5 * (lvs[i].sum(1) - lvs[j].sum(1) - n_z + torch.exp(lvs[j] - lvs[i]).sum(1)
                              + ((mus[i] - mus[j]) ** 2 * torch.exp(-lvs[i])).sum(1)))
        cost = cost + lam * (a1 + a2)
    return cost


def scheduled_cost_and_grads(archs, flat, X, eps, binary, weights, lam, act, kl=1.0, batch_global=None, masks=None):
    """-> (cost_t, its gradient as a flat fp64 array)"""
    t = torch.tensor(np.asarray(flat, np.float64), dtype=torch.float64, requires_grad=True)
    c = scheduled_cost(archs, t, [torch.tensor(np.asarray(x, np.float64)) for x in X], torch.tensor(np.asarray(eps, np.float64)),
                       binary, weights, float(lam), act, float(kl), batch_global, masks)
    c.backward()
    return float(c.item()), t.grad.numpy().copy()


def scheduled_step(ref, X, eps, kl_t, lambda_t, lr_eff_t, batch_global=None, masks=None):
    """One scheduled step of oracle ``ref`` (an ``OracleAssocVAE``): cost_t and its gradient at ref's weights, then the oracle's
    ``adam_step`` with lr_eff_t -> (cost_t, gradient)."""
    cost, g = scheduled_cost_and_grads(ref.network_architectures, ref.get_params(), X, eps, ref.binary, ref.weights, lambda_t,
                                       ref.act, kl_t, batch_global, masks)
    ref.t += 1
    th, ref.m, ref.v = O.adam_step(ref.get_params(), ref.m, ref.v, g, ref.t, float(lr_eff_t))
    ref.set_params(th)
    return cost, g
