"""The cases of the second pass over the sigma-lognormal kernels (HISTORY.md section R20): the fit inside
every tile class (TT = 64 / 32 / 8 time points for CC = 4 / 8 / 16 components) and component count, the exits of its loop, the
step's clips, the weights, and the sampler's edges.  tests/test_gpu_lognormal.py runs them on the device and
tests/test_lognormal_cpu.py asserts the conditions they lean on: every accept decision of the float64 definition has a margin
|L(new) - L| > 1e-3 L, every convergence decision a margin |(L - L(new)) - tol L| > 1e-3 tol L, and the float32 restatement takes
the same decisions.  The seeds were chosen by search on the CPU; each is named next to its case.

A case is ``LR.step_case`` plus T, dt and ``opt``, the options of ``LR.fit`` (free, lo, hi, weights, tol)."""
import numpy as np

import lognormal_reference as LR

F32 = np.float32
TRIES = (1, 4)


def case_dt(T):
    return float(F32(0.01 if T == 1 else 1.0 / (T - 1)))


def make(N, C, seed, counts=None, T=LR.T_CASE, dt=None, rows=None, **opt):
    """``rows``: keep these rows of the case only"""
    dt = (LR.DT_CASE if T == LR.T_CASE else case_dt(T)) if dt is None else dt
    case = LR.step_case(N, C, seed, counts, T, dt)
    if rows is not None:
        case = {k: v[list(rows)] for k, v in case.items()}
    case.update(T=T, dt=dt, opt=dict(opt))
    return case


def run(case, n_iters, restated, **over):
    opt = dict(tol=0.0)
    opt.update(case["opt"])
    opt.update(over)
    return LR.fit(case["target"], case["init"], case["count"], case["start"], case["dt"], n_iters=n_iters, restated=restated, **opt)


def refs(case, tries=TRIES, **over):
    """{n_iters: (definition, restatement)}"""
    return {it: (run(case, it, False, **over), run(case, it, True, **over)) for it in tries}


_CACHE = {}


def cached(name, builder, tries=TRIES):
    """(case, refs) of a named case, built once a session and never changed"""
    if name not in _CACHE:
        case = builder()
        _CACHE[name] = (case, refs(case, tries))
    return _CACHE[name]


def decisions_agree(r64, r32):
    """the restatement accepts and rejects the tries the definition does"""
    same = lambda a, b: [ln is not None and ln < l for l, ln in a] == [ln is not None and ln < l for l, ln in b]
    return all(same(a, b) for a, b in zip(r64["tries"], r32["tries"])) and np.array_equal(r64["status"], r32["status"])


def margin(r):
    return min(LR.margins(t) for t in r["tries"])


def conv_margin(tries, tol):
    """the smallest |(L - Ln) - tol L| / (tol L) over the accepted tries of a run (inf without one)"""
    m = [abs((l - ln) - tol * l) / (tol * l) for l, ln in tries if ln is not None and ln < l]
    return min(m) if m else np.inf


# ------------------------------------------------------------------------------------------------ 1. tile and component classes
# rows of separated_params under seed 2000 (the first seed tried): every cell has a margin above 1e-3
TILE_SEED = 2000
TILE_SHAPES = ([(3, T) for T in (1, 2, 63, 64, 65, 128, 1024)] + [(6, T) for T in (1, 2, 31, 32, 33, 64, 1024)]
               + [(C, T) for C in (9, 12, 15) for T in (1, 2, 7, 8, 9, 16)] + [(12, 1024)])
FREE_PER_ROW_SEED = 78


def tile_case(C, T):
    return cached("tile-%d-%d" % (C, T), lambda: make(2, C, TILE_SEED, T=T))


def _per_row_12():
    case = make(3, 12, RAGGED_SEEDS["per-row-12"], (12, 9, 5))
    case["opt"]["free"] = (np.random.default_rng(FREE_PER_ROW_SEED).random((3, 12, 6)) < 0.7).astype(np.uint8)
    return case


RAGGED_SEEDS = {"ragged-4": 2000, "ragged-12": 2000, "per-row-12": 2000}
RAGGED_CASES = {
    "ragged-4": lambda: make(4, 4, RAGGED_SEEDS["ragged-4"], (4, 2, 1, 0)),
    "ragged-12": lambda: make(4, 12, RAGGED_SEEDS["ragged-12"], (12, 9, 5, 0)),
    "per-row-12": _per_row_12,
}


def ragged_case(name):
    return cached(name, RAGGED_CASES[name])


# ------------------------------------------------------------------------------------------------ 2. the exits
# a finite D near the top of float32: the amplitude overflows, the first loss is not finite and every try is rejected by the solve
OVERFLOW_ROW, OVERFLOW_D = 1, 3e38


def overflow_case():
    case = make(3, 3, 21)
    case["init"][OVERFLOW_ROW, 0, 0] = F32(OVERFLOW_D)
    case["opt"]["tol"] = 1e-9
    return case


# the other rejection: one component, only sigma free, and a D at which the amplitude stays finite while the Jacobian's sigma
# entry, |amp| (z^2 - 1) / sg, does not: M is the 1 x 1 infinity, its pivot passes, and g / sqrt(M) is not finite
X_REJECT_FREE = np.array([0, 0, 0, 1, 0, 0], dtype=np.uint8)
X_REJECT_D = 1e37                                      # (1e37 .. 3e37 take "x"; from 5e37 the pivot is NaN)


def x_reject_case():
    case = make(2, 1, 21)
    case["init"][1, 0, 0] = F32(X_REJECT_D)
    case["opt"].update(tol=1e-9, free=X_REJECT_FREE)
    return case


# tol: rows of step_case(5, 3, 21) on which definition and restatement end in the same try
# (9, 8, 1 and 3 tries at tol 0.5; row 3 takes 7 against 13), and the one row among seeds 21 .. 25 at tol <= 1e-2 (6 tries): on long
# runs the two part ways at the floor of float32
TOL_TRIES = 40
# "between": rows of seed 31 (seeds 21 .. 40 searched) whose last try gains 41 to 46 % of L, which is below tol L and above
# tol L(new): a loop that tested against tol L(new) would go on there (5, 4 and 1 tries)
TOL_CASES = {"tol-0.5": (21, (0, 1, 2, 4), 0.5), "tol-0.01": (22, (4,), 0.01), "tol-0.5-between": (31, (0, 2, 4), 0.5)}
TOL_BETWEEN = ("tol-0.5-between",)


def tol_case(name):
    seed, rows, tol = TOL_CASES[name]
    return cached(name, lambda: make(5, 3, seed, rows=rows, tol=tol), tries=(TOL_TRIES,))


# ------------------------------------------------------------------------------------------------ 3. clips and weights
# (seed, row, component, clip value): an initial sigma of 0.002 on one component of row 2; within four tries the accepted steps
# throw a sigma of that row onto the clip, in the definition and in the restatement alike (seeds 3000 .. 3009 searched)
CLIP_CASES = {"clip-hi-3000": (3000, 2, 0, 3.0), "clip-hi-3008": (3008, 2, 0, 3.0), "clip-lo-3008": (3008, 2, 1, 1e-3)}


def clip_case(name):
    seed, row, comp, _ = CLIP_CASES[name]

    def build():
        case = make(3, 3, seed)
        case["init"][row, comp, 3] = F32(0.002)
        return case
    return cached(name, build)


BOUND_CASES = {"lo-alone": dict(lo=LR.BOUNDS_THAT_BIND[0]), "hi-alone": dict(hi=LR.BOUNDS_THAT_BIND[1])}


def bound_case(name):
    return cached(name, lambda: make(3, 3, 1000, **BOUND_CASES[name]))


WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (3.0, 0.5))
WEIGHT_SHAPES = ((3, 3), (2, 8))                       # seed 1000: margins of at least 0.0026 in all six


def weight_case(N, C, w):
    return cached("w-%d-%d-%g-%g" % (N, C, w[0], w[1]), lambda: make(N, C, 1000, weights=w))


# ------------------------------------------------------------------------------------------------ 5. the sampler's edges
SAMPLE_EDGE_SHAPES = ((3, 2, 16, 1024), (1, 1, 1, 1), (2, 1, 4, 128))
HIGH_SEED = 0xF234567887654321


def sample_edge(shape):
    """-> (params [N, C, 6], count [N], start [N, 2], dt): at N = 3 the counts are (C, 0, 9) and a D is negative"""
    N, S, C, T = shape
    rng = np.random.default_rng(sum(shape))
    params = np.stack([LR.separated_params(C, rng) for _ in range(N)]).astype(F32)
    count = np.full(N, C, dtype=np.int32)
    if N == 3:
        count[:] = (C, 0, 9)
        params[0, 2, 0] = -params[0, 2, 0]
        params[2, 1, 0] = -params[2, 1, 0]
    start = (np.tile(np.asarray(LR.START_CASE, dtype=F32), (N, 1)) + F32(0.25) * np.arange(N, dtype=F32)[:, None]).astype(F32)
    return params, count, start, case_dt(T)
