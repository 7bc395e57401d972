"""fp64 reference of the masked step (include/avae.h), composed from the oracle by presence pattern.

A row's masked cost terms are exactly those of the sub-model made of the modalities the row has: its own reconstruction and KL
terms, and the association terms of the pairs inside it.  So, for every non-empty pattern P (the set of modalities present in a
row), the oracle runs forward + backward on the sub-model of P's modalities (their archs, params, inputs, weights, binary flags),
on the pattern's rows with their eps rows, with ``batch_global`` = the whole batch; costs and per-modality gradients add up over
the patterns, and a modality gets no gradient from a row that does not have it.  Exact in fp64 for any M, conv modalities
included.  ``quant`` / relu ``masks`` are handed through as the parity tests use them."""
from itertools import combinations

import numpy as np

from oracle import vae_assoc_oracle as O


def patterns(present):
    """{pattern (tuple of modality indices): row indices} over the rows with at least one modality present"""
    present = np.asarray(present) != 0
    out = {}
    for n, row in enumerate(present):
        key = tuple(int(m) for m in np.flatnonzero(row))
        if key:
            out.setdefault(key, []).append(n)
    return {k: np.asarray(v) for k, v in out.items()}


def masked_cost_and_grads(archs, params_flat, X, eps, present, binary, weights, assoc_lambda, act,
                          batch_global=None, quant=None, masks=None):
    """-> (cost, flat gradient) of the masked cost, fp64.  ``present`` [B, M]; ``X[m]`` may be None when column m is all absent;
    ``masks`` = hip_relu_masks of the whole batch (rows are picked per pattern)."""
    M = len(archs)
    present = np.asarray(present) != 0
    B = present.shape[0]
    Bg = B if batch_global is None else batch_global
    params = O.unflatten_params(archs, np.asarray(params_flat, dtype=np.float64), np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    grads = [{name: np.zeros(shp) for name, shp in O.layer_shapes(na)} for na in archs]
    cost = 0.0
    for pat, rows in patterns(present).items():
        sa = [archs[m] for m in pat]
        sp = [params[m] for m in pat]
        sx = [np.asarray(X[m], dtype=np.float64)[rows] for m in pat]
        sb = [binary[m] for m in pat]
        sw = [weights[m] for m in pat]
        se = eps[rows]
        sm = None
        if masks is not None:
            sm = [{key: [np.asarray(a)[rows] for a in masks[m][key]] for key in ("enc", "dec")} for m in pat]
        fw = O.forward(sa, sp, sx, se, sb, act, quant)
        cost += O.shard_cost(sa, fw, sx, sb, sw, assoc_lambda, Bg)
        g, _ = O.backward(sa, sp, fw, sx, se, sb, sw, assoc_lambda, act, Bg, quant, sm)
        for k, m in enumerate(pat):
            for name in grads[m]:
                grads[m][name] = grads[m][name] + g[k][name]
    return float(cost), O.flatten_params(archs, grads)


def per_row_terms(archs, params_flat, X, eps, binary, act, quant=None):
    """avae_score's per-row columns in fp64: recon [B, M], latent [B, M], assoc [B, P] (pairs i<j in lexicographic order)."""
    params = O.unflatten_params(archs, np.asarray(params_flat, dtype=np.float64), np.float64)
    X = [np.asarray(x, dtype=np.float64) for x in X]
    fw = O.forward(archs, params, X, np.asarray(eps, dtype=np.float64), binary, act, quant)
    recon, latent = [], []
    for f, x, b in zip(fw, X, binary):
        xr, mu, lv = f["xhat"], f["mu"], f["lv"]
        if b:
            recon.append(-np.sum(x * np.log(1e-3 + xr) + (1 - x) * np.log(1e-3 + 1 - xr), axis=1))
        else:
            recon.append(np.sum((x - xr) ** 2, axis=1) / 2.0)
        latent.append(-0.5 * np.sum(1 + lv - mu ** 2 - np.exp(lv), axis=1))
    assoc = []
    for i, j in combinations(range(len(archs)), 2):
        mi, mj, li, lj = fw[i]["mu"], fw[j]["mu"], fw[i]["lv"], fw[j]["lv"]
        assoc.append(np.sum(0.5 * (np.exp(li - lj) + np.exp(lj - li) - 2.0 + (mi - mj) ** 2 * (np.exp(-li) + np.exp(-lj))), axis=1))
    B = X[0].shape[0]
    return (np.stack(recon, 1), np.stack(latent, 1),
            np.stack(assoc, 1) if assoc else np.zeros((B, 0)))


def masked_cost_from_rows(recon, latent, assoc, present, binary, weights, assoc_lambda, batch_global):
    """The masked cost of include/avae.h from per-row columns (avae_score's, or per_row_terms'):
    sum_m w_m [ (1/B_g) sum_n p latent + (binary_m ? 1/B_g : 1) sum_n p recon ] + lambda sum_{i<j} sum_n p_i p_j assoc"""
    p = (np.asarray(present) != 0).astype(np.float64)
    recon, latent, assoc = (np.asarray(a, dtype=np.float64) for a in (recon, latent, assoc))
    M = p.shape[1]
    c = 0.0
    for m in range(M):
        r = np.sum(p[:, m] * recon[:, m])
        c += weights[m] * (np.sum(p[:, m] * latent[:, m]) / batch_global + (r / batch_global if binary[m] else r))
    for k, (i, j) in enumerate(combinations(range(M), 2)):
        c += assoc_lambda * np.sum(p[:, i] * p[:, j] * assoc[:, k])
    return float(c)
