"""fp64 reference of avae_score_masked / avae_loglik_masked (include/avae.h).

The per-row columns come from ``masked_reference.per_row_terms`` and the log-likelihood arithmetic is ``ref_loglik``'s of
tests/scoring_reference.py (both imported, neither edited); absent entries are replaced by zeros before anything reads them and
every gate is an ``np.where`` select, so NaN / Inf / None in an absent entry cannot reach a result.  ``ref`` is an
``OracleAssocVAE`` (its ``quant`` is handed through, so the same code gives the bf16 reference).

``pattern_*`` give the other side of the pattern identity that checks this reference: the masked result of a row with
pattern P is the UNMASKED reference of the sub-model made of P's modalities, on that row with the same eps.  The sub-model is
evaluated on the whole row block (absent entries as zeros) and the pattern's rows are picked from the result: a row's fp64 bits
in a BLAS product can depend on how many rows the product has (one row takes the matrix-vector path), and the identity is
about the arithmetic of a row, so both sides see the same row block and the comparison can be exact."""
from itertools import combinations

import numpy as np

from masked_reference import patterns, per_row_terms
from oracle import vae_assoc_oracle as O
from scoring_reference import logsumexp, recon_rows, ref_loglik, ref_scores


def all_patterns_mask(N, M, shift=0):
    """Deterministic presence [N, M]: row n has pattern perm[(n + shift) mod 2^M] (bit m = modality m), perm a fixed permutation
    of 0..2^M-1 -- so every one of the 2^M patterns, the empty one included, occurs in ANY 2^M consecutive rows."""
    n_pat = 1 << M
    perm = np.array([(5 * k + 3) % n_pat for k in range(n_pat)])            # 5 is odd: a permutation of 0..2^M-1
    assert sorted(perm.tolist()) == list(range(n_pat))
    code = perm[(np.arange(N) + shift) % n_pat]
    return ((code[:, None] >> np.arange(M)[None, :]) & 1).astype(bool)


def has_every_pattern(present):
    p = np.asarray(present) != 0
    M = p.shape[1]
    return len({tuple(r) for r in p.tolist()}) == 1 << M


def _fold(ref, X, present):
    """-> (presence with None modalities folded in, X with absent entries selected to 0 in fp64)"""
    p = (np.asarray(present) != 0).copy()
    Xf = []
    for m, na in enumerate(ref.network_architectures):
        if X[m] is None:
            p[:, m] = False
            Xf.append(np.zeros((p.shape[0], int(na["n_input"]))))
        else:
            Xf.append(np.where(p[:, m:m + 1], np.asarray(X[m], np.float64), 0.0))
    return p, Xf


def ref_scores_masked(ref, X, present, eps, cross=False):
    """Columns of avae_score_masked: recon / latent 0 where absent, assoc 0 where either is absent, cost over what the row has,
    cross NaN where source or target is absent."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    M = len(archs)
    p, Xf = _fold(ref, X, present)
    eps = np.asarray(eps, np.float64)
    recon, latent, assoc = per_row_terms(archs, ref.get_params(), Xf, eps, binary, act, q)
    recon, latent = np.where(p, recon, 0.0), np.where(p, latent, 0.0)
    for k, (i, j) in enumerate(combinations(range(M), 2)):
        assoc[:, k] = np.where(p[:, i] & p[:, j], assoc[:, k], 0.0)
    w = np.asarray(ref.weights, np.float64)
    out = {"recon": recon, "latent": latent, "assoc": assoc,
           "cost": ((recon + latent) * w).sum(1) + ref.assoc_lambda * assoc.sum(1)}
    if cross:
        cr = np.full((p.shape[0], M, M), np.nan)
        for s in range(M):
            mu = O.encode(archs[s], ref.params[s], Xf[s], act, q)[0]
            for d in range(M):
                xh = O.decode(archs[d], ref.params[d], mu, act, binary[d], q)[0]
                cr[:, s, d] = np.where(p[:, s] & p[:, d], recon_rows(Xf[d], xh, binary[d]), np.nan)
        out["cross"] = cr
    return out


def ref_loglik_masked(ref, X, present, eps):
    """Outputs of avae_loglik_masked with ref_loglik's arithmetic; the joint sums the present l_d only."""
    archs, binary, act, q = ref.network_architectures, ref.binary, ref.act, ref.quant
    M = len(archs)
    p, Xf = _fold(ref, X, present)
    eps = np.asarray(eps, np.float64)
    N, K, nz = eps.shape
    marginal, joint, cond = np.full((N, M), np.nan), np.full((N, M), np.nan), np.full((N, M, M), np.nan)
    for s in range(M):
        mu, lv = O.encode(archs[s], ref.params[s], Xf[s], act, q)[:2]
        z = mu[:, None, :] + np.exp(0.5 * lv)[:, None, :] * eps
        r = np.sum(-0.5 * z ** 2 + 0.5 * eps ** 2 + 0.5 * lv[:, None, :], axis=2)
        ell = np.stack([-recon_rows(np.repeat(Xf[d], K, axis=0),
                                    O.decode(archs[d], ref.params[d], z.reshape(N * K, nz), act, binary[d], q)[0],
                                    binary[d]).reshape(N, K) for d in range(M)], axis=2)
        tot = np.zeros((N, K))
        for d in range(M):                                                  # present l_d, in modality order
            tot = np.where(p[:, d:d + 1], tot + ell[:, :, d], tot)
        ps = p[:, s]
        marginal[:, s] = np.where(ps, logsumexp(ell[:, :, s] + r, 1) - np.log(K), np.nan)
        joint[:, s] = np.where(ps, logsumexp(tot + r, 1) - np.log(K), np.nan)
        # conditional: one reduction per pattern over the [N, K, |P|] block of its own columns -- NumPy's sum over the sample axis
        # rounds differently for different widths of the trailing axis, and ref_loglik reduces a sub-model's block this way
        for pat, rows in patterns(p).items():
            if s in pat:
                lse = logsumexp(np.stack([ell[:, :, d] for d in pat], axis=2), 1) - np.log(K)
                for b, d in enumerate(pat):
                    cond[rows, s, d] = lse[rows, b]
    return {"marginal": marginal, "joint": joint, "conditional": cond}


def sub_model(ref, pat):
    """The oracle of the sub-model made of the modalities in ``pat``, on ref's parameters."""
    sa = [ref.network_architectures[m] for m in pat]
    flat = O.flatten_params(sa, [ref.params[m] for m in pat])
    return O.OracleAssocVAE(sa, [ref.binary[m] for m in pat], ref.act, [ref.weights[m] for m in pat], ref.assoc_lambda,
                            ref.learning_rate, ref.batch_size, params_flat=flat, quant=ref.quant)


def pattern_scores(ref, X, present, eps, cross=False):
    """Pattern by pattern: scoring_reference.ref_scores of the sub-model, its values on the pattern's rows scattered into full-width
    columns (NaN marks what the pattern does not define, every column of a row with nothing present included)."""
    p, Xf = _fold(ref, X, present)
    N, M = p.shape
    pairs = list(combinations(range(M), 2))
    out = {"cost": np.full(N, np.nan), "recon": np.full((N, M), np.nan), "latent": np.full((N, M), np.nan),
           "assoc": np.full((N, len(pairs)), np.nan)}
    if cross:
        out["cross"] = np.full((N, M, M), np.nan)
    for pat, rows in patterns(p).items():
        sub = sub_model(ref, pat)
        got = ref_scores(sub, [Xf[m] for m in pat], np.asarray(eps, np.float64), cross=cross)
        got = {key: v[rows] for key, v in got.items()}
        out["cost"][rows] = got["cost"]
        for a, m in enumerate(pat):
            out["recon"][rows, m] = got["recon"][:, a]
            out["latent"][rows, m] = got["latent"][:, a]
            if cross:
                for b, d in enumerate(pat):
                    out["cross"][rows, m, d] = got["cross"][:, a, b]
        for k, (a, b) in enumerate(combinations(range(len(pat)), 2)):
            out["assoc"][rows, pairs.index((pat[a], pat[b]))] = got["assoc"][:, k]
    return out


def pattern_loglik(ref, X, present, eps):
    """Pattern by pattern: scoring_reference.ref_loglik of the sub-model, its values on the pattern's rows scattered (NaN elsewhere)."""
    p, Xf = _fold(ref, X, present)
    N, M = p.shape
    out = {"marginal": np.full((N, M), np.nan), "joint": np.full((N, M), np.nan), "conditional": np.full((N, M, M), np.nan)}
    for pat, rows in patterns(p).items():
        sub = sub_model(ref, pat)
        got = ref_loglik(sub, [Xf[m] for m in pat], np.asarray(eps, np.float64))
        got = {key: v[rows] for key, v in got.items()}
        for a, m in enumerate(pat):
            out["marginal"][rows, m] = got["marginal"][:, a]
            out["joint"][rows, m] = got["joint"][:, a]
            for b, d in enumerate(pat):
                out["conditional"][rows, m, d] = got["conditional"][:, a, b]
    return out


def assert_masked_columns(got, want, tol, what=""):
    """The comparer of the masked outputs: NaN positions must be identical in output and reference; the finite entries then obey
    the rule of test_gpu_score / test_gpu_loglik's assert_columns (max error of a column <= tol * the column's max |ref|), the
    maximum taken over the finite reference entries."""
    for key, r in want.items():
        g = np.asarray(got[key], np.float64)
        r = np.asarray(r, np.float64)
        assert g.shape == r.shape, "%s%s shape %s vs %s" % (what, key, g.shape, r.shape)
        g2, r2 = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
        assert np.array_equal(np.isnan(g2), np.isnan(r2)), "%s%s: NaN positions differ" % (what, key)
        assert not np.any(np.isinf(g2)), "%s%s has infinities" % (what, key)
        for c in range(r2.shape[1]):
            ok = np.isfinite(r2[:, c])
            if not ok.any():
                continue
            scale = max(np.abs(r2[ok, c]).max(), 1e-30)
            err = np.abs(g2[ok, c] - r2[ok, c]).max()
            print("%s%s column %d: max err %.3e, max |ref| %.3e, tol %.1e" % (what, key, c, err, scale, tol))
            assert err <= tol * scale, "%s%s column %d: max err %.3e vs max |ref| %.3e" % (what, key, c, err, scale)
