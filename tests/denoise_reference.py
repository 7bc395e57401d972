"""Reference of denoising training (include/avae.h): the corruption stream restated in NumPy, and the
cost and gradient of a step whose encoders read ``X_in`` while its losses are charged against ``X``.

The stream: Philox4x32-10, key = the handle's seed, counter (global row, column quad, step lo, step hi ^ (salt + modality)); an
element is dropped where the top 24 bits of its word are below floor(drop_prob * 2^24), the normals are the Box-Muller pairs
of the block, formed as the internal eps is.  The step: ``oracle.backward`` takes the encoder's input from the forward cache
and uses ``X`` in the loss gradient only, so ``backward(forward(X_in), X)`` is the exact gradient of
``loss_terms(forward(X_in), X)`` (tests/test_denoise_cpu.py checks it against central differences) and the reference is a
two-line composition of the unchanged oracle; with ``present`` it composes by presence pattern as tests/masked_reference.py."""
import numpy as np

from masked_reference import patterns
from oracle import vae_assoc_oracle as O

SALT_DROP = 0x64726F70
SALT_NOISE = 0x6E6F6973
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counter words (broadcastable integer arrays) and key words -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def stream_words(seed, step, rows, cols, m, salt, row_offset=0):
    """The Philox blocks of modality ``m`` at step ``step``: uint32 [rows, n_quads, 4], block (r, q) for global row
    row_offset + r and columns 4q .. 4q+3."""
    nq = (cols + 3) // 4
    R = (row_offset + np.arange(rows, dtype=np.uint64))[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    step = int(step)
    w = philox4x32_10(R, q, step & 0xFFFFFFFF, ((step >> 32) ^ (salt + m)) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack(w, axis=-1)


def drop_threshold(p):
    """T = floor(drop_prob * 2^24), drop_prob as the float32 the library is handed, the product in double"""
    return int(np.floor(float(np.float32(p)) * 16777216.0))


def drop_mask(seed, step, rows, cols, m, p, row_offset=0):
    """bool [rows, cols]: the dropped elements"""
    w = stream_words(seed, step, rows, cols, m, SALT_DROP, row_offset)
    return ((w >> np.uint32(8)) < np.uint32(drop_threshold(p))).reshape(rows, -1)[:, :cols]


def normals(seed, step, rows, cols, m, row_offset=0):
    """float64 [rows, cols]: the N(0,1) of the noise stream.  The uniforms are formed in float32 as on the device
    (((w >> 8) + 0.5) * 2^-24), log / sqrt / sin / cos in double."""
    w = stream_words(seed, step, rows, cols, m, SALT_NOISE, row_offset)
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    u = u.astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a, b = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    n = np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], axis=-1)
    return n.reshape(rows, -1)[:, :cols]


def corrupt(x, seed, step, m, drop=0.0, noise=0.0, drop_value=0.0, row_offset=0):
    """x~ of include/avae.h in float64: ``dropped ? drop_value : (noise > 0 ? x + noise * n : x)``; a stream is evaluated only
    where its parameter is non-zero.  -> (x~, dropped mask or None)"""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = x.shape
    out = x.copy()
    if noise > 0:
        out = x + float(np.float32(noise)) * normals(seed, step, rows, cols, m, row_offset)
    d = None
    if drop_threshold(drop) > 0:
        d = drop_mask(seed, step, rows, cols, m, drop, row_offset)
        out = np.where(d, float(np.float32(drop_value)), out)
    return out, d


def denoise_cost_and_grads(archs, params_flat, X, X_in, eps, binary, weights, assoc_lambda, act, present=None, batch_global=None,
                           quant=None, masks=None):
    """-> (cost, flat gradient), fp64, of ``loss_terms(forward(X_in), X)``: the encoders read ``X_in``, every loss term is
    charged against ``X``.  ``present`` [B, M]: the masked cost, composed by presence pattern (``X[m]`` / ``X_in[m]`` may be
    None where column m is all absent); ``masks`` = hip_relu_masks of the whole batch; ``batch_global``: the divisor of the
    mean terms (a shard of a larger batch)."""
    params = O.unflatten_params(archs, np.asarray(params_flat, dtype=np.float64), np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    B = eps.shape[0]
    Bg = B if batch_global is None else batch_global
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    X, X_in = [f64(x) for x in X], [f64(x) for x in X_in]
    if present is None:
        fw = O.forward(archs, params, X_in, eps, binary, act, quant)
        if batch_global is None:      # (the oracle's own two branches, so that X_in = X is OracleAssocVAE.cost_and_grads bit for bit)
            cost = O.loss_terms(archs, fw, X, binary, weights, assoc_lambda)["cost"]
        else:
            cost = O.shard_cost(archs, fw, X, binary, weights, assoc_lambda, batch_global)
        g, _ = O.backward(archs, params, fw, X, eps, binary, weights, assoc_lambda, act, batch_global, quant, masks)
        return float(cost), O.flatten_params(archs, g)
    grads = [{name: np.zeros(shp) for name, shp in O.layer_shapes(na)} for na in archs]
    cost = 0.0
    for pat, rows in patterns(present).items():
        pick = lambda L: [L[m] for m in pat]
        sa, sp, sb, sw = pick(archs), pick(params), pick(binary), pick(weights)
        sx, si, se = [X[m][rows] for m in pat], [X_in[m][rows] for m in pat], eps[rows]
        sm = None
        if masks is not None:
            sm = [{key: [np.asarray(a)[rows] for a in masks[m][key]] for key in ("enc", "dec")} for m in pat]
        fw = O.forward(sa, sp, si, se, sb, act, quant)
        cost += O.shard_cost(sa, fw, sx, sb, sw, assoc_lambda, Bg)
        g, _ = O.backward(sa, sp, fw, sx, se, sb, sw, assoc_lambda, act, Bg, quant, sm)
        for k, m in enumerate(pat):
            for name in grads[m]:
                grads[m][name] = grads[m][name] + g[k][name]
    return float(cost), O.flatten_params(archs, grads)
