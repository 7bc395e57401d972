"""The inputs of the iLQR tests (tests/test_track_cpu.py, tests/test_gpu_track.py) and their shared
references: every reference is computed once per process and handed out unchanged.

``smooth_case((rows, T, D))``: the targets are the pen tips of a smooth in-limit joint trajectory (``ik_cases.smooth_trajectory``: the
fixture arm for D = 7, else a random chain), the first guess that trajectory plus a slow wave of 0.02 rad, rounded to float32.
``figure_case(a, guess)``: the issue's recorded prototype on the fixture arm -- ``path = fk(seed_pos) + (a cos 2 pi s - a,
a sin 4 pi s, 0)``, s = linspace(0, 1, T), from a position-only damped-least-squares guess ('ik') or from the seed repeated ('seed').
Below them one case per branch of the loop.  ``named`` hands out a case together with the options it is run with."""
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

# the shapes of the issue: (name, shape)
SHAPES = ((1, 1, 1), (3, 2, 3), (3, 3, 3), (2, 257, 16), (65, 8, 7), (300, 3, 3), (2, 63, 2), (2, 64, 2), (2, 65, 2),
          (3, 4, 5), (3, 4, 9), (3, 4, 12), (3, 4, 15))
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
            "binding": lambda: (binding_case(), dict(limit_weight=1e3, dt=0.1))}[name]()


STEP_CASES = tuple("smooth-%d-%d-%d" % s for s in SHAPES) + ("figure", "effort", "no-effort", "binding")


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
