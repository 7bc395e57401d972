"""NumPy references of the per-row scoring calls (the definitions of include/avae.h on the CPU oracle): score_samples' terms and
the importance-weighted log-likelihoods.  Plain module (NumPy and the oracle only), shared by the GPU tests that compare the
kernels against it and by the CPU tests that check the references themselves."""
from itertools import combinations

import numpy as np

from oracle import vae_assoc_oracle as O


def recon_rows(x, xhat, binary):
    if binary:
        return -np.sum(x * np.log(1e-3 + xhat) + (1 - x) * np.log(1e-3 + 1 - xhat), axis=1)
    return 0.5 * np.sum((x - xhat) ** 2, axis=1)


def ref_scores(ref, X, eps, cross=False):
    """Per-row terms from O.forward / O.encode / O.decode (the definitions of include/avae.h)."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    X = [np.asarray(x, np.float64) for x in X]
    fw = O.forward(archs, ref.params, X, np.asarray(eps, np.float64), binary, act, q)
    recon = np.stack([recon_rows(x, f["xhat"], b) for x, f, b in zip(X, fw, binary)], 1)
    latent = np.stack([-0.5 * np.sum(1 + f["lv"] - f["mu"] ** 2 - np.exp(f["lv"]), 1) for f in fw], 1)
    assoc = [np.sum(0.5 * (np.exp(fw[i]["lv"] - fw[j]["lv"]) + np.exp(fw[j]["lv"] - fw[i]["lv"]) - 2.0
                           + (fw[i]["mu"] - fw[j]["mu"]) ** 2 * (np.exp(-fw[i]["lv"]) + np.exp(-fw[j]["lv"]))), 1)
             for i, j in combinations(range(len(archs)), 2)]
    assoc = np.stack(assoc, 1) if assoc else np.zeros((X[0].shape[0], 0))
    w = np.asarray(ref.weights, np.float64)
    out = {"recon": recon, "latent": latent, "assoc": assoc,
           "cost": ((recon + latent) * w).sum(1) + ref.assoc_lambda * assoc.sum(1)}
    if cross:
        M = len(archs)
        mus = [f["mu"] for f in fw]
        cr = np.zeros((X[0].shape[0], M, M))
        for s in range(M):
            for d in range(M):
                xh = O.decode(archs[d], ref.params[d], mus[s], act, binary[d], q)[0]
                cr[:, s, d] = recon_rows(X[d], xh, binary[d])
        out["cross"] = cr
    return out


def logsumexp(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def ref_loglik(ref, X, eps):
    """The definitions of include/avae.h, from O.encode / O.decode and a float64 log-sum-exp.  eps: [N, K, n_z].
    Per proposal s: z_k = mu_s + exp(lv_s/2) eps_k, l_d(z) = -recon_d(x_d, dec_d(z)), r_k = sum(-z^2/2 + eps^2/2 + lv_s/2);
    marginal[s] = LSE_k(l_s + r) - log K, joint[s] = LSE_k(sum_d l_d + r) - log K, conditional[s, d] = LSE_k l_d - log K."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    X = [np.asarray(x, np.float64) for x in X]
    eps = np.asarray(eps, np.float64)
    N, K, nz = eps.shape
    M = len(archs)
    marginal, joint, cond = np.zeros((N, M)), np.zeros((N, M)), np.zeros((N, M, M))
    for s in range(M):
        mu, lv = O.encode(archs[s], ref.params[s], X[s], act, q)[:2]
        z = mu[:, None, :] + np.exp(0.5 * lv)[:, None, :] * eps                       # [N, K, n_z]
        r = np.sum(-0.5 * z ** 2 + 0.5 * eps ** 2 + 0.5 * lv[:, None, :], axis=2)     # [N, K]
        ell = np.stack([-recon_rows(np.repeat(X[d], K, axis=0),
                                    O.decode(archs[d], ref.params[d], z.reshape(N * K, nz), act, binary[d], q)[0],
                                    binary[d]).reshape(N, K) for d in range(M)], axis=2)    # [N, K, M]
        marginal[:, s] = logsumexp(ell[:, :, s] + r, 1) - np.log(K)
        joint[:, s] = logsumexp(ell.sum(2) + r, 1) - np.log(K)
        cond[:, s, :] = logsumexp(ell, 1) - np.log(K)
    return {"marginal": marginal, "joint": joint, "conditional": cond}
