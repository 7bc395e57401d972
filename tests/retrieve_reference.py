"""The definition of ``latent_topk`` (avae_latent_topk in include/avae.h), for the tests.

Distance of a query posterior (mu_q, lv_q) and a gallery posterior (mu_g, lv_g), with v = exp(lv), iv = exp(-lv), d = mu_q - mu_g,
t = v_q - v_g:

    l2      sum_j d*d
    symkl   0.5 * sum_j [ (t*iv_q)*(t*iv_g) + (d*d)*(iv_q + iv_g) ]

``dist64`` is that in float64; ``dist32`` restates it in NumPy float32 in the stated operation order (every product and sum
rounded to float32, dimensions added in index order, no fused multiply-add); ``two_kl64`` is the reference's formula written out
(vae_assoc.py:355-365): KL(q_q || q_g) + KL(q_g || q_q).  ``order`` is the total order of a result row: (isnan(dist), dist, index)
ascending."""
import numpy as np

METRICS = ("symkl", "l2")


def _pairs(q, g, dt):
    """[N, 1, nz] and [1, G, nz] views of the rows in dtype ``dt`` (logvar None stays None)"""
    qm, ql = q
    gm, gl = g
    c = lambda a, ax: None if a is None else np.expand_dims(np.asarray(a).astype(dt), ax)
    return c(qm, 1), c(ql, 1), c(gm, 0), c(gl, 0)


def dist64(q, g, metric):
    """[N, G] float64 distances of (mu, logvar) pairs q = ([N, nz], [N, nz]) and g = ([G, nz], [G, nz])"""
    qm, ql, gm, gl = _pairs(q, g, np.float64)
    with np.errstate(all="ignore"):
        d = qm - gm
        if metric == "l2":
            return (d * d).sum(-1)
        vq, vg, iq, ig = np.exp(ql), np.exp(gl), np.exp(-ql), np.exp(-gl)
        t = vq - vg
        return 0.5 * ((t * iq) * (t * ig) + (d * d) * (iq + ig)).sum(-1)


def dist32(q, g, metric):
    """The same in float32, operation by operation, the latent dimensions added one after the other"""
    qm, ql, gm, gl = _pairs(q, g, np.float32)
    N, G, nz = qm.shape[0], gm.shape[1], qm.shape[2]
    acc = np.zeros((N, G), np.float32)
    with np.errstate(all="ignore"):
        if metric != "l2":
            vq, vg, iq, ig = np.exp(ql), np.exp(gl), np.exp(-ql), np.exp(-gl)
            assert vq.dtype == np.float32
        for j in range(nz):
            d = qm[..., j] - gm[..., j]
            if metric == "l2":
                acc = acc + d * d
            else:
                t = vq[..., j] - vg[..., j]
                acc = acc + ((t * iq[..., j]) * (t * ig[..., j]) + (d * d) * (iq[..., j] + ig[..., j]))
        out = acc if metric == "l2" else np.float32(0.5) * acc
    assert out.dtype == np.float32
    return out


def two_kl64(q, g):
    """KL(q_q || q_g) + KL(q_g || q_q) of diagonal Gaussians, the reference's two terms written out, float64 [N, G]"""
    qm, ql, gm, gl = _pairs(q, g, np.float64)

    def kl(m1, l1, m2, l2):
        return 0.5 * (np.exp(l1 - l2) + (m1 - m2) ** 2 * np.exp(-l2) - 1.0 - (l1 - l2)).sum(-1)
    return kl(qm, ql, gm, gl) + kl(gm, gl, qm, ql)


def order(dist_row):
    """Gallery indices of one query's distances in the documented total order: NaN last, ties to the lower index"""
    d = np.asarray(dist_row)
    return np.lexsort((np.arange(d.shape[0]), d, np.isnan(d)))


def topk(D, k):
    """(index [N, k] int32, distance [N, k]) of a distance matrix D [N, G] under ``order``; k beyond G pads with -1 / +inf"""
    N, G = D.shape
    index = np.full((N, k), -1, np.int32)
    dist = np.full((N, k), np.inf, D.dtype)
    for n in range(N):
        o = order(D[n])[:k]
        index[n, :o.size] = o
        dist[n, :o.size] = D[n, o]
    return index, dist


def recall(D, ks):
    """Recall@k of paired rows from a square distance matrix D[n, g] (query n's partner is gallery row n): [len(ks)] float64"""
    N = D.shape[0]
    index, _ = topk(D, max(ks))
    hit = index == np.arange(N)[:, None]
    return np.array([hit[:, :k].any(1).mean() for k in ks], np.float64)


def latents(rng, rows, nz):
    """The tests' random posteriors: mu ~ N(0, 1), lv ~ U(-6, 1), float32"""
    return rng.standard_normal((rows, nz)).astype(np.float32), rng.uniform(-6.0, 1.0, (rows, nz)).astype(np.float32)


def plan_cover(rows, gallery_rows, query_tile, gallery_tile, n_splits):
    """What avae_latent_topk_plan's numbers mean (include/avae.h): the query tiles of one chunk and the splits' gallery row ranges
    -> (list of (q_lo, q_hi), list of (g_lo, g_hi))"""
    q = [(a, min(rows, a + query_tile)) for a in range(0, rows, query_tile)]
    tiles = -(-gallery_rows // gallery_tile)
    if n_splits == 0:
        return q, []
    per = -(-tiles // n_splits)
    g = [(s * per * gallery_tile, min(gallery_rows, (s + 1) * per * gallery_tile)) for s in range(n_splits)]
    return q, g
