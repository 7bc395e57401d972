"""The inputs of the iLQR tests (tests/test_track_cpu.py, tests/test_gpu_track.py, tests/test_gpu_track_edges.py; DESIGN.md section
29) and their shared references: every reference is computed once per process and handed out unchanged.

``smooth_case((rows, T, D))``: the targets are the pen tips of a smooth in-limit joint trajectory (``ik_cases.smooth_trajectory``: the
fixture arm for D = 7, else a random chain), the first guess that trajectory plus a slow wave of 0.02 rad, rounded to float32.
``figure_case(a, guess)``: the issue's recorded prototype on the fixture arm -- ``path = fk(seed_pos) + (a cos 2 pi s - a,
a sin 4 pi s, 0)``, s = linspace(0, 1, T), from a position-only damped-least-squares guess ('ik') or from the seed repeated ('seed').
Below them one case per branch of the loop and per exit of the backward pass.  ``named`` hands out a case together with the options
it is run with."""
import numpy as np

import ik_cases as IC
import ik_reference as K
import render_reference as R
import track_reference as TR

F32 = np.float32
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(name, chain, path, init, **more):
    frames, axes = chain.packed()
    return dict(name=name, chain=chain, frames=frames, axes=axes, path=np.ascontiguousarray(path, dtype=F32),
                init=np.ascontiguousarray(init, dtype=F32), **more)


def smooth_case(shape):
    def make():
        chain, q = IC.smooth_trajectory(shape)
        rows, T, D = q.shape
        rng = np.random.default_rng([29, rows, T, D])
        tau = np.linspace(0.0, 1.0, T)[None, :, None]
        wave = 0.02 * np.sin(2.0 * np.pi * (tau + rng.uniform(0.0, 1.0, (rows, 1, D))))
        return _case("smooth-%d-%d-%d" % tuple(shape), chain, chain.forward(q), q + wave)
    return _cached(("smooth", tuple(shape)), make)


def figure_path(chain, seed, a, T):
    s = np.linspace(0.0, 1.0, T)
    return chain.forward(seed) + np.stack([a * np.cos(2 * np.pi * s) - a, a * np.sin(4 * np.pi * s), 0.0 * s], axis=1)


def figure_case(amplitudes, guess, T=100):
    """one row per amplitude"""
    def make():
        chain = IC.fixture_chain()
        seed = np.asarray(R.fixture()["seed_pos"], dtype=np.float64)
        path = np.stack([figure_path(chain, seed, a, T) for a in amplitudes]).astype(F32)
        n = len(amplitudes)
        if guess == "ik":
            frames, axes = chain.packed()
            init = K.ik(path, frames, axes, np.tile(seed.astype(F32), (n, 1)), limits=chain.limits)["trajectory"]
        else:
            init = np.tile(seed, (n, T, 1))
        return _case("figure-%s-%s" % (guess, "-".join("%g" % a for a in amplitudes)), chain, path, init)
    return _cached(("figure", tuple(amplitudes), guess, T), make)


def effort_case():
    """``smooth_case((3, 8, 7))`` under a full effort matrix"""
    c = smooth_case((3, 8, 7))
    rng = np.random.default_rng(2907)
    return dict(c, name="effort", effort=(np.eye(7) + 0.3 * rng.standard_normal((7, 7))).astype(F32))


def binding_case():
    """``smooth_case((3, 8, 7))`` in a box that cuts 0.05 rad into joint 1's range of motion from above: the penalty is active on
    the first guess and stays active.  Run at dt = 0.1: at 0.01 the effort term holds an angle with R / dt^4 = 1e6 per rad^2 and a
    penalty of 1e3 moves nothing."""
    c = smooth_case((3, 8, 7))
    lim = c["chain"].limits.copy()
    lim[1, 1] = c["init"][:, :, 1].max() - 0.05
    return dict(c, name="binding", limits=lim.astype(F32))


def dyadic_case(moving):
    """Effort only (track weights 0) at dt = 1/2, R = 2^59, lam0 = 1e-6, with first guesses that are multiples of 1/4: every first
    control is a float and 2 R + lam is 2^60 in double, so the first try's gain is -u exactly -- in the definition, the restatement
    and the kernel alike -- and the try lands on u = 0, J = 0.  Nothing lowers 0: every later try is rejected and the row leaves by
    lam > lam_max with status 0.  ``moving`` False: the first guess stands still, J = 0 from the start, no try is ever accepted:
    status 2."""
    def make():
        from vae_assoc_amd.kinematics import KinematicChain
        chain = KinematicChain(R.random_joints(3, 30))
        rng = np.random.default_rng([29, 59, int(moving)])
        init = 0.25 * rng.integers(-2, 3, (3, 5, 3)) if moving else np.tile(0.25 * rng.integers(-2, 3, (3, 1, 3)), (1, 5, 1))
        if moving:
            init[:, 2] = init[:, 1] + 0.25                      # (no row stands still)
        return _case("dyadic-%d" % moving, chain, chain.forward(init), init)
    return _cached(("dyadic", bool(moving)), make)


DYADIC = dict(dt=0.5, track_weights=(0.0, 0.0, 0.0), effort_weight=float(2.0 ** 59), lam0=1e-6, tol=0.0, n_iters=20)


def subnormal_case():
    """Tries the backward pass rejects by a gain that is finite as double and infinite as float: 3 rows, T = 6, D = 3, a first
    guess that stands still, the path 0.05 rad away from it, run at dt = 2^-130 (a float32 subnormal) without effort.  Then
    Q_uu = lam + dt^4 S and K ~ 1 / dt = 1.4e39 as long as lam stays below dt^4 S ~ 1e-157; above that the gains shrink to
    dt^3 S / lam and the try is made, and rejected by the cost: nothing moves at that dt (dt^2 k rounds away in q + dt v)."""
    def make():
        from vae_assoc_amd.kinematics import KinematicChain
        chain = KinematicChain(R.random_joints(3, 30))
        init = np.tile(np.random.default_rng(7).uniform(-0.5, 0.5, (3, 1, 3)), (1, 6, 1)).astype(F32)
        return _case("subnormal", chain, chain.forward(init.astype(np.float64) + 0.05), init)
    return _cached("subnormal", make)


SUBNORMAL = dict(dt=float(2.0 ** -130), effort_weight=0.0, tol=0.0, lam_min=1e-300)
# (the options on top of SUBNORMAL, every row's decisions, status)
SUBNORMAL_RUNS = ((dict(lam0=1e-300, n_iters=5), "ppppp", 1),
                  (dict(lam0=1e-300, factor=1e10, lam_max=1e-275, n_iters=12), "ppp", 2),
                  (dict(lam0=1e-170, factor=1e10, n_iters=12), "pppppprrrrrr", 1))


# The pivot exit.  Track weights of 1e20: ww = w w overflows in float, so l_qq of the first guess is inf (NaN where a Jacobian entry
# is 0) in the kernel and in the restatement, V_xx is not finite from T - 1 on and a pivot of Q_uu is NaN as soon as S enters it (the
# gains of T - 2, where S is still 0, are finite: 0).  The definition's l_qq is 2e40 J J, finite: it rejects the same tries by the
# float rule on K ~ 1 / dt, as long as lam stays below dt^4 S (five tries from 1e-300 do).  So the decisions agree, for two reasons.
OVERFLOW = dict(SUBNORMAL, track_weights=(1e20, 1e20, 1e20), lam0=1e-300, n_iters=5)


def huge_case(value=1e36):
    """``smooth_case((3, 5, 3))`` with one first-guess angle of row 1 at ``value``: its first controls are 1e40, finite as double
    and infinite as float, and so are the first try's gains: 'p', then a try that is made from the LDS the rejected one left"""
    c = smooth_case((3, 5, 3))
    init = c["init"].copy()
    init[1, 2, 0] = value
    return dict(c, name="huge-%g" % value, init=init)


HUGE = dict(n_iters=3, tol=0.0)


def boxed(c, name, cuts):
    """the case ``c`` in its chain's limits cut into the first guess's own range: ``cuts`` = ((joint, 'lo' | 'hi', depth), ...)"""
    lim = c["chain"].limits.copy()
    for j, side, depth in cuts:
        if side == "hi":
            lim[j, 1] = c["init"][:, :, j].max() - depth
        else:
            lim[j, 0] = c["init"][:, :, j].min() + depth
    assert (lim[:, 0] < lim[:, 1]).all(), name
    return dict(c, name=name, limits=lim.astype(F32), cuts=cuts)


def outside(c, q):
    """per cut of a ``boxed`` case: does an angle of ``q`` [rows, T, D] lie beyond that side of the box"""
    lim = c["limits"]
    return [bool((q[:, :, j] > lim[j, 1]).any() if side == "hi" else (q[:, :, j] < lim[j, 0]).any()) for j, side, _ in c["cuts"]]


def two_sided_case():
    """``smooth_case((3, 8, 7))``: joint 1 cut from above, joint 3 from below (0.05 rad), joint 5 from both sides (0.02 rad)"""
    return boxed(smooth_case((3, 8, 7)), "two-sided", ((1, "hi", 0.05), (3, "lo", 0.05), (5, "hi", 0.02), (5, "lo", 0.02)))


def box_case(D):
    """the same kind of box in the classes D <= 4 and D = 16: joint 0 from above, the last from below, joint 1 from both sides"""
    shape = {3: (3, 8, 3), 16: (2, 5, 16)}[D]
    return boxed(smooth_case(shape), "box-%d" % D, ((0, "hi", 0.05), (D - 1, "lo", 0.05), (1, "hi", 0.02), (1, "lo", 0.02)))


EFFORT_SHAPES = ((3, 6, 3), (3, 6, 4), (2, 5, 16))


def effort_matrix_case(shape, singular):
    """``smooth_case(shape)`` under E = I + 0.3 N(0, 1); ``singular``: its last row and column zeroed, so that Se = R E^T E has a
    null direction (the last joint's control) and Q_uu is positive there by lam and dt^4 S alone"""
    D = shape[2]
    E = np.eye(D) + 0.3 * np.random.default_rng([2922, D]).standard_normal((D, D))
    if singular:
        E[-1, :] = 0.0
        E[:, -1] = 0.0
    return dict(smooth_case(shape), name="effort-%d%s" % (D, "-singular" if singular else ""), effort=E.astype(F32))


def effort_limits_case():
    """an effort matrix, binding limits on both sides and R > 0 together, on (3, 8, 7)"""
    return dict(two_sided_case(), name="effort-limits", effort=effort_case()["effort"])


# the shapes of the issue: (name, shape); from (3, 4, 4) on: the tops of the D classes (the uniform c < D branch of the walk is never
# taken) and the D no case had; T at the second stride's edges, over a whole third stride and at kTrackMaxT
SHAPES = ((1, 1, 1), (3, 2, 3), (3, 3, 3), (2, 257, 16), (65, 8, 7), (300, 3, 3), (2, 63, 2), (2, 64, 2), (2, 65, 2),
          (3, 4, 5), (3, 4, 9), (3, 4, 12), (3, 4, 15),
          (3, 4, 4), (3, 4, 8), (3, 4, 16), (3, 4, 6), (3, 4, 10), (3, 4, 13), (3, 4, 14), (2, 2, 16), (2, 127, 5), (2, 128, 3),
          (2, 129, 3), (2, 192, 8), (2, 193, 4), (2, 1024, 2), (1, 513, 16))
LONGEST = (1, 1024, 16)                                          # at 1 try only: the margin of its fourth try's 'r' is not measured
FIGURES = (0.02, 0.025, 0.03, 0.035, 0.04)                       # the five rows of (5, 100, 7)
REJECTING = (0.12,)
# the rows of the tol test: their sixth try gains 1.6e-6, 3.4e-6 and 7.0e-6 of the cost (the fifth 5e-4), well above what float32
# moves a cost by (3e-7) and below tol = 1e-5.  (At a = 0.02 the sixth try gains 3e-7: the restatement rejects it.)
TOL_FIGURES = (0.03, 0.035, 0.04)


def named(name):
    """-> (case, the options it runs with but n_iters and tol)"""
    if name.startswith("smooth"):
        return smooth_case(tuple(int(v) for v in name.split("-")[1:])), {}
    return {"figure": lambda: (figure_case(FIGURES, "ik"), {}),
            "rejecting": lambda: (figure_case(REJECTING, "seed"), dict(lam0=1e-6)),
            "effort": lambda: (effort_case(), {}),
            "no-effort": lambda: (smooth_case((3, 8, 7)), dict(effort_weight=0.0, lam0=1e-6)),
            "binding": lambda: (binding_case(), dict(limit_weight=1e3, dt=0.1)),
            "two-sided": lambda: (two_sided_case(), dict(limit_weight=1e3, dt=0.1)),
            "box-3": lambda: (box_case(3), dict(limit_weight=1e3, dt=0.1)),
            "box-16": lambda: (box_case(16), dict(limit_weight=1e3, dt=0.1)),
            "effort-limits": lambda: (effort_limits_case(), dict(limit_weight=1e3, dt=0.1)),
            **{effort_matrix_case(s, sing)["name"]: (lambda s=s, sing=sing: (effort_matrix_case(s, sing), {}))
               for s in EFFORT_SHAPES for sing in (False, True)}}[name]()


STEP_CASES = tuple("smooth-%d-%d-%d" % s for s in SHAPES) + ("figure", "effort", "no-effort", "binding")
BOXED_CASES = ("two-sided", "box-3", "box-16", "effort-limits")
# the limit term's other branch and other classes, E in every class, full and singular (tests/test_gpu_track_edges.py)
TERM_CASES = BOXED_CASES + tuple("effort-%d%s" % (s[2], t) for s in EFFORT_SHAPES for t in ("", "-singular"))

# options only the C ABI reaches: (label, case, options, every row's decisions, status)
ABI_RUNS = (("factor 2", lambda: figure_case((0.03, 0.035), "ik"), dict(factor=2.0, n_iters=8, tol=0.0), "aaaaaaaa", 1),
            ("lam_max 1e-3", lambda: figure_case(REJECTING, "seed"), dict(lam0=1e-6, lam_max=1e-3, tol=0.0), "aaarrrr", 0),
            ("tol 1", lambda: figure_case(FIGURES, "ik"), dict(tol=1.0), "a", 0),
            ("tol 0.5", lambda: figure_case(FIGURES, "ik"), dict(tol=0.5), "a", 0),
            # the figures from the seed repeated: the first try gains 25.9 % of J, between tol / (1 + tol) = 23.1 % and tol -- below
            # tol J and above tol J', so the old cost is what the test is made against (the later tries gain 31.7, 28.4, 1.4 %)
            ("tol 0.3", lambda: figure_case(FIGURES, "seed"), dict(tol=0.3), "a", 0))


def solve(c, prec, **options):
    """track_reference.track on a case, cached per (case, precision, options)"""
    key = ("solve", c["name"], np.dtype(prec).name, tuple(sorted((k, str(v)) for k, v in options.items())))
    return _cached(key, lambda: TR.track(c["path"], c["init"], c["frames"], c["axes"], effort=c.get("effort"),
                                         limits=c.get("limits"), prec=prec, **options))


def refs(c, **options):
    """-> (definition, restatement), having checked that they take the same decisions"""
    r64, r32 = solve(c, np.float64, **options), solve(c, F32, **options)
    assert r64["decisions"] == r32["decisions"], (c["name"], options, r64["decisions"], r32["decisions"])
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(r64[k], r32[k]), (c["name"], k)
    return r64, r32


def rel_err(got, ref):
    return R.rel_err(got, ref)


def errors(got, ref):
    """the measure of the issue per quantity: worst |err| / (|ref| + 1); the controls against max |u| + 1"""
    u = np.asarray(ref["controls"], dtype=np.float64)
    scale = (np.abs(u).max() if u.size else 0.0) + 1.0
    ue = float(np.abs(np.asarray(got["controls"], dtype=np.float64) - u).max() / scale) if u.size else 0.0
    return dict(trajectory=rel_err(got["trajectory"], ref["trajectory"]), controls=ue, cost=rel_err(got["cost"], ref["cost"]))
