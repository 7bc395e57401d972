"""The inputs of the latent-space sweeps, in one place: tests/test_gpu_latent_sweep.py runs the kernels on them,
tests/test_latent_sweep_cpu.py checks without a device that every reference is finite and every tolerance is non-zero.

A. latent_topk, latent_stats, aggregate_log_density and fit_latent_prior / latent_prior_score at the latent widths where their
   thread maps change: every width class of k_gmm_estep's phase 2 and of lanes_of (8, 16, 32, 64) at its exact width, one past it
   and at its most idle width; n_z < 4 (a Gram block with guarded edges only, tiles staged with row = e / n_z at n_z = 1, 2, 3,
   unroll-by-4 loops shorter than one round); n_z < 8 (waves of k_agg_logpdf that own no marginal column) and n_z = 63 (the
   merge's 64 columns exactly).
B. latent_topk with more than 64 splits, so that the merge keeps more than one list head per lane.

Everything is seeded and computed once per process.  The tolerance rule is the one of the four kernels' own test files: the
kernel's worst error against the float64 definition may be at most 4x the float32 restatement's own worst error on the same
inputs, pooled per n_z over a test's case list."""
import numpy as np

import aggregate_reference as A
import latent_prior_reference as P
import latent_stats_reference as S
import retrieve_reference as R
from test_gpu_aggregate import SMALL as AGG_SMALL, _arith_case as agg_small_case      # (z, g, refs by (N, G), own (joint, marginal))
from test_gpu_latent_stats import _masked_case as stats_masked_case
from test_gpu_retrieve import _arith_case as topk_case, _rel_err as rel_err

NZ_NEW = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63)


# ------------------------------------------------------------------------------------------------ A1. latent_topk
TOPK_NG = [(N, G) for N in (1, 19) for G in (1, 5, 64)]
TOPK_SELECT_NZ = (1, 9, 16, 33)            # the exact selection check: G = 1000 (4 splits of 4 tiles), N = 70, k in TOPK_KS
TOPK_SELECT_G = 1000
TOPK_KS = (1, 5, 64)


# topk_case(n_z, metric) -> (q, g, ref, own): 19 queries and 64 gallery rows from default_rng(100 + n_z), the float64 definition on
# them and the float32 restatement's worst rel_err over the 19 x 64 pairs (tests/test_gpu_retrieve.py's own case, generic in n_z)


# ------------------------------------------------------------------------------------------------ A2. latent_stats
STATS_ROWS = (1, 2, 65, 4099)
STATS_MASKED_NZ = (3, 9, 33)


def stats_bound(nz, rows=STATS_ROWS):
    """latent_stats_reference.bound pooled over ``rows`` instead of its ROWS -> (4 x worst, worst) per statistic"""
    worst = {k: 0.0 for k in S.NAMES[1:]}
    for name in S.FAMILIES:
        for n in rows:
            for k, e in S.case(name, n, nz)[2].items():
                worst[k] = max(worst[k], e)
    return {k: 4.0 * e for k, e in worst.items()}, worst


# ------------------------------------------------------------------------------------------------ A3. aggregate_log_density
AGG_BIG_NZ = (1, 9, 33, 63)
AGG_BIG = (130, 2100)                       # three slices, the last tile of 52 rows
AGG_EXCLUDE_NZ = (9, 63)
AGG_EXCLUDE = (70, 133)                     # two query tiles, three gallery tiles (the last of 5 rows)


def _agg_own(z, g, ref, nz, exclude=None):
    r32 = A.logpdf32(z, g, exclude)
    return float(A.joint_err(r32[0], ref[0], nz).max()), float(A.marginal_err(r32[1], ref[1]).max())


_AGG = {}


def agg_big_case(nz):
    """AGG_BIG from default_rng(1000 * n_z + G) -> (z, g, ref, own)"""
    if ("big", nz) not in _AGG:
        N, G = AGG_BIG
        rng = np.random.default_rng(1000 * nz + G)
        g = A.latents(rng, G, nz)
        z = A.queries(rng, g, N)
        ref = A.logpdf64(z, g)
        _AGG["big", nz] = (z, g, ref, _agg_own(z, g, ref, nz))
    return _AGG["big", nz]


def agg_exclude_case(nz):
    """AGG_EXCLUDE from default_rng(40 + n_z): every query leaves one gallery row out, the first six on block and tile borders,
    the next four name no row of the gallery -> (z, g, exclude, ref, own)"""
    if ("exclude", nz) not in _AGG:
        N, G = AGG_EXCLUDE
        rng = np.random.default_rng(40 + nz)
        g = A.latents(rng, G, nz)
        z = A.queries(rng, g, N)
        ex = rng.integers(0, G, N)
        ex[:6] = (0, 7, 8, 63, 64, G - 1)
        ex[6:10] = (-1, G, -2 ** 31, 2 ** 31 - 1)
        ref = A.logpdf64(z, g, ex)
        _AGG["exclude", nz] = (z, g, ex, ref, _agg_own(z, g, ref, nz, ex))
    return _AGG["exclude", nz]


# ------------------------------------------------------------------------------------------------ A4. the mixture prior
# every width class of phase 2 (components pg, pg + KG, ..., KG = 256 / JW) meets a K just past one stride of that map and a K
# just past one round of phase 1 (16 components: four waves of four)
PRIOR_PAIRS = ((1, 1), (1, 64), (2, 3), (5, 32), (8, 33), (9, 16), (12, 64), (16, 17), (17, 8), (32, 9), (33, 5), (63, 63))
PRIOR_NZ = tuple(sorted({nz for nz, _ in PRIOR_PAIRS}))
PRIOR_N = (1, 19, 64, 65, 300)
PRIOR_KEYS = ("weights", "means", "logvars")

_PRIOR = {}


def prior_case(nz):
    """For every K paired with this n_z, N of PRIOR_N, with and without logvar: clusters(sep = 3) from
    default_rng(1000 n_z + 10 K + N), its start, one float64 iteration and the float64 E-step of the start; over all of them the
    float32 restatement's worst errors.  -> (cases, own_step (weights, means, logvars, bound), own_score (resp, ll)); a case is
    (K, N, mu, logvar, init, ref, bound, ll64, r64).  n_z = 1 pools K = 1 with K = 64: a single component's weight is exactly 1 in
    both precisions."""
    if nz not in _PRIOR:
        cases, own, own_sc = [], (0.0,) * 4, (0.0, 0.0)
        for K in [k for z, k in PRIOR_PAIRS if z == nz]:
            for N in PRIOR_N:
                rng = np.random.default_rng(1000 * nz + 10 * K + N)
                mu, lv, _ = P.clusters(rng, N, nz, min(K, 4), 3.0)
                for logvar in (lv, None):
                    init = P.start(rng, mu, logvar, K)
                    ref, bound, n = P.step64(mu, logvar, init)
                    assert n == N
                    r32, b32, _ = P.step32(mu, logvar, init)
                    own = tuple(max(o, e) for o, e in zip(own, P.prior_errs(r32, ref, [b32], [bound], nz)))
                    ll64, r64 = P.estep64(mu, logvar, init)
                    ll32, rs32 = P.estep32(mu, logvar, init)
                    own_sc = (max(own_sc[0], float(P.abs_err(rs32, r64).max())), max(own_sc[1], float(P.ll_err(ll32, ll64, nz).max())))
                    cases.append((K, N, mu, logvar, init, ref, bound, ll64, r64))
        _PRIOR[nz] = (cases, own, own_sc)
    return _PRIOR[nz]


# ------------------------------------------------------------------------------------------------ B. more than 64 splits
# (queries, gallery rows, n_z, splits): the merge's lane l keeps the heads of the splits l, l + 64, l + 128, l + 192
#   (1, 16385, 20): 65 splits; split 64 is one tile of one row, the first head with r = 1
#   (70, 65536, 20): 256 splits of 4 tiles, all four heads of every lane; a second query tile of 6 rows
#   (1, 65537, 7): 205 splits of 5 tiles
LATTICE = ((1, 16385, 20, 65), (70, 65536, 20, 256), (1, 65537, 7, 205))
LATTICE_PLANTED = (256 * 64, 256 * 128 + 1, 256 * 192 + 2, 65536 - 1)      # in the 65536 case: bitwise copies of query 0
FLOAT_SPLITS = (65536, 20, ((1, 256), (5000, 13)))                          # gallery rows, n_z, (queries, splits) of the two calls


def lattice_case(rows, G, nz):
    """Integer lattice latents: mu drawn from the integers of [-8, 8] as float32, lv = 0.  Every operation of the kernel's chain
    is then exact in float32 -- differences |d| <= 16, squares <= 256, sums <= 64 * 256 -- and under symkl t = 0, iv = 1 give
    0.5 * (2 * the same sum).  With G = 65536 the rows LATTICE_PLANTED are copies of query 0.  -> (q, g) pairs of (mu, lv)"""
    rng = np.random.default_rng([rows, G, nz])
    qm = rng.integers(-8, 9, (rows, nz)).astype(np.float32)
    gm = rng.integers(-8, 9, (G, nz)).astype(np.float32)
    if G == 65536:
        gm[list(LATTICE_PLANTED)] = qm[0]
    return (qm, np.zeros_like(qm)), (gm, np.zeros_like(gm))


def lattice_table(q, g, k, chunk=8):
    """(index [N, k] int32, distance [N, k] float32) in integer arithmetic: squared distances, ties to the lower index"""
    qi, gi = q[0].astype(np.int64), g[0].astype(np.int64)
    index = np.empty((qi.shape[0], k), np.int32)
    dist = np.empty((qi.shape[0], k), np.float32)
    for lo in range(0, qi.shape[0], chunk):
        d = qi[lo:lo + chunk, None, :] - gi[None]
        D = (d * d).sum(-1)
        o = np.argsort(D, axis=1, kind="stable")[:, :k]
        index[lo:lo + chunk] = o
        dist[lo:lo + chunk] = np.take_along_axis(D, o, 1)
    return index, dist
