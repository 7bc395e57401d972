"""The black-box search without a GPU: properties of the float64 definition (tests/search_reference.py), the
restatement of the kernels against it, the folded constraint of ``MotionBasis.projection``, convergence of the loop on the
reference's own toy problem with the Philox stream, and every ValueError of ``search`` / ``refine_motion`` (marshalling on
``device="cpu"``)."""
import numpy as np
import pytest
import torch

import search_reference as S
from vae_assoc_amd import vae_assoc as V
from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
from vae_assoc_amd.motion import MotionBasis


def _case(P=3, R=12, n=5, seed=0, family="spread"):
    return S.update_case(P, R, n, family, np.random.default_rng(seed))


NO_BOUNDS = dict(rel_lower=-1.0, abs_lower=-1.0, abs_upper=-1.0)


# ------------------------------------------------------------------------------------------------ the stream
def test_normals_have_the_moments_of_a_normal_and_depend_on_every_counter_word():
    z = S.normals(7, 0, 4, 1024, 6)
    assert z.shape == (4, 1024, 6)
    se = 1.0 / np.sqrt(1024)
    assert np.abs(z.mean(1)).max() < 5 * se and np.abs(z.var(1) - 1.0).max() < 5 * np.sqrt(2.0) * se
    for other in (S.normals(8, 0, 4, 1024, 6), S.normals(7, 1, 4, 1024, 6), S.normals(7, 0, 4, 1024, 6, problem_offset=1)):
        assert (other != z).all()
    assert np.array_equal(S.normals(7, 0, 2, 1024, 6, problem_offset=2), z[2:])             # chunking by problem_offset
    assert np.array_equal(S.normals(7, 0, 4, 1024, 5), z[:, :, :5])                          # a dimension's draw does not depend on n
    assert np.abs(S.normals_f32(7, 0, 4, 64, 6) - z[:, :64]).max() < 1e-5


def test_sample_restated_follows_the_definition():
    rng = np.random.default_rng(1)
    for P, R, n in S.SAMPLE_SHAPES:
        mean, var = rng.standard_normal((P, n)).astype(np.float32), (0.1 + rng.random((P, n))).astype(np.float32)
        proj = None
        if n in S.SAMPLE_GROUPS:
            G, g = S.SAMPLE_GROUPS[n]
            proj = (rng.standard_normal((G, g, g)).astype(np.float32) / np.sqrt(g), rng.standard_normal((P, n)).astype(np.float32))
        for pr in (None, proj):
            r64, r32 = S.sample(mean, var, 5, 3, R, 0, pr), S.sample_restated(mean, var, 5, 3, R, 0, pr)
            assert r32.dtype == np.float32 and r32.shape == (P, R, n)
            assert (np.abs(r32 - r64) / (np.abs(r64) + 1.0)).max() < 2e-6


# ------------------------------------------------------------------------------------------------ the update
def test_equal_costs_and_vanishing_eliteness_give_the_plain_mean():
    x, c, st = _case()
    plain = x.astype(np.float64).mean(1)
    new, h = S.update(x, np.full_like(c, 1.25), st, S.options(**NO_BOUNDS))
    assert np.abs(new["mean"] - plain).max() < 1e-14 and np.allclose(h["avg_cost"], 1.25) and (new["n_applied"] == 1).all()
    new, _ = S.update(x, c, st, S.options(eliteness=1e-12, **NO_BOUNDS))
    assert np.abs(new["mean"] - plain).max() < 1e-11
    for weighting in (S.CEM, S.CMAES):                              # the equal-cost test precedes every weighting
        new, _ = S.update(x, np.full_like(c, 1.25), st, S.options(weighting=weighting, eliteness=3, **NO_BOUNDS))
        assert np.abs(new["mean"] - plain).max() < 1e-14


def test_cem_covariance_is_the_weighted_sample_variance_and_pibb_is_about_the_old_mean():
    x, c, st = _case(seed=1)
    x64 = x.astype(np.float64)
    for weighting, e in ((S.PIBB, 10.0), (S.CEM, 4), (S.CMAES, 4)):
        new, _ = S.update(x, c, st, S.options(weighting=weighting, cov_update=S.CEM, eliteness=e, **NO_BOUNDS))
        for p in range(x.shape[0]):
            cp = c[p].astype(np.float64)
            if weighting == S.PIBB:
                w = np.exp(-e * (cp - cp.min()) / (cp.max() - cp.min() + 1e-6))
            else:
                order = np.argsort(cp, kind="stable")[:e]
                w = np.zeros_like(cp)
                w[order] = 1.0 / e if weighting == S.CEM else np.log(e + 0.5) - np.log(np.arange(e) + 1.0)
            w = w / w.sum()
            m = w @ x64[p]
            assert np.abs(new["mean"][p] - m).max() < 1e-13
            assert np.abs(new["var"][p] - w @ (x64[p] - m) ** 2).max() < 1e-13
    new, _ = S.update(x, c, st, S.options(lr=0.5, **NO_BOUNDS))
    cp = c[0].astype(np.float64)
    w = np.exp(-10.0 * (cp - cp.min()) / (cp.max() - cp.min() + 1e-6))
    w = w / w.sum()
    want = 0.5 * st["var"][0] + 0.5 * (w @ (x64[0] - st["mean"][0]) ** 2)
    assert np.abs(new["var"][0] - want).max() < 1e-13


def test_bounds_hold_in_their_order():
    x, c, st = _case(seed=2, n=9)
    free, _ = S.update(x, c, st, S.options(**NO_BOUNDS))
    rel, _ = S.update(x, c, st, S.options(rel_lower=0.5))
    for p in range(3):
        floor = 0.5 * free["var"][p].max()
        assert rel["var"][p].min() >= floor and (free["var"][p] < floor).any()
        assert np.array_equal(rel["var"][p], np.maximum(free["var"][p], floor))
    both, _ = S.update(x, c, st, S.options(rel_lower=0.5, abs_lower=0.01, abs_upper=0.2))
    for p in range(3):
        capped = np.minimum(free["var"][p], 0.2)
        assert np.array_equal(both["var"][p], np.maximum(capped, max(0.01, 0.5 * capped.max())))
    only_abs, _ = S.update(x, c, st, S.options(rel_lower=-1.0, abs_lower=0.3))
    assert np.array_equal(only_abs["var"], np.maximum(free["var"], 0.3))
    assert np.array_equal(rel["mean"], free["mean"])


def test_a_nonfinite_cost_changes_nothing_but_its_own_weight():
    x, c, st = _case(seed=3)
    for bad in (np.nan, np.inf, -np.inf):
        c2, x2 = c.copy(), x.copy()
        c2[1, 4] = bad
        x2[1, 4] = np.nan                                            # (what such a rollout holds does not matter either)
        new, h = S.update(x2, c2, st, S.options())
        keep = np.arange(c.shape[1]) != 4
        alone, ha = S.update(x[:, keep], c[:, keep], st, S.options())
        for k in ("mean", "var", "best_cost", "best_x"):                 # problem 1 is the problem without that rollout
            assert np.abs(new[k][1] - alone[k][1]).max() < 1e-13, k      # (NumPy's sums of 11 and of 12 terms pair differently)
        assert abs(h["avg_cost"][1] - ha["avg_cost"][1]) < 1e-13 and np.isfinite(new["mean"]).all()


def test_all_nan_and_frozen_problems_are_left_alone():
    x, c, st = _case(seed=4, family="all_nan")
    st["frozen"][2] = 1
    new, h = S.update(x, c, st, S.options())
    for p in (1, 2):                                                 # problem 1: all NaN; problem 2: frozen
        assert np.array_equal(new["mean"][p], st["mean"][p]) and np.array_equal(new["var"][p], st["var"][p])
        assert new["n_applied"][p] == 0 and np.isnan([h[k][p] for k in h]).all()
    assert new["n_applied"][0] == 1 and np.isfinite([h[k][0] for k in h]).all()
    assert new["best_cost"][1] == st["best_cost"][1] and np.array_equal(new["best_x"][1], st["best_x"][1])
    assert new["best_cost"][2] == min(st["best_cost"][2], c[2].min())          # a frozen problem still keeps the best it saw


def test_freezing_n_applied_and_the_best_rollout():
    cost = lambda x: np.linalg.norm(x, axis=2)
    x0 = np.array([[5.0, 5.0], [1e-9, 0.0]])
    st, h = S.search(cost, x0, 1e-20, n_rollouts=6, n_iters=4, opt=S.options(rel_lower=-1.0, tol=1e-6), seed=1)
    assert st["frozen"].tolist() == [1, 1] and st["n_applied"].tolist() == [1, 1]
    assert np.isfinite(h["moved"][0]).all() and np.isnan(h["moved"][1:]).all() and (h["moved"][0] < 1e-6).all()
    never, h = S.search(cost, x0, 1e-20, n_rollouts=6, n_iters=4, opt=S.options(rel_lower=-1.0, tol=0.0), seed=1)
    assert never["frozen"].tolist() == [0, 0] and never["n_applied"].tolist() == [4, 4] and np.isfinite(h["moved"]).all()
    # the best rollout: the lowest cost seen, the earlier on a tie
    x, c, st = _case(seed=5)
    c[0, 3] = c[0, 7] = 0.5
    st["best_cost"][:] = np.inf
    new, _ = S.update(x, c, st, S.options())
    assert new["best_cost"][0] == 0.5 and np.array_equal(new["best_x"][0], x[0, 3].astype(np.float64))
    again, _ = S.update(x[:, ::-1], c[:, ::-1], new, S.options())
    assert np.array_equal(again["best_x"][0], new["best_x"][0])      # an equal cost later does not replace it


def test_k_then_m_iterations_are_k_plus_m():
    cost = lambda x: np.linalg.norm(x - 0.3, axis=2)
    x0 = np.random.default_rng(6).standard_normal((3, 4))
    whole, hw = S.search(cost, x0, 0.5, n_rollouts=8, n_iters=7, seed=9)
    part, h1 = S.search(cost, x0, 0.5, n_rollouts=8, n_iters=3, seed=9)
    part, h2 = S.search(cost, None, None, n_rollouts=8, n_iters=4, seed=9, state=part)
    for k in ("mean", "var", "best_cost", "best_x", "n_applied", "frozen"):
        assert np.array_equal(whole[k], part[k]), k
    assert whole["iteration"] == part["iteration"] == 7
    assert np.array_equal(hw["avg_cost"], np.concatenate([h1["avg_cost"], h2["avg_cost"]]))


def test_restated_update_follows_the_definition_on_every_family():
    rng = np.random.default_rng(7)
    worst = 0.0
    for P, R, n in ((3, 10, 20), (2, 300, 33), (1, 1024, 8)):
        for family in S.FAMILIES:
            for weighting, e in ((S.PIBB, 10.0), (S.CEM, 3), (S.CMAES, 3)):
                x, c, st = S.update_case(P, R, n, family, rng)
                opt = S.options(weighting=weighting, eliteness=e, cov_update=S.CEM if weighting == S.CEM else S.PIBB, lr=0.5,
                                abs_upper=0.9)
                d, hd = S.update(x, c, st, opt)
                r, hr = S.update_restated(x, c, st, opt)
                assert r["mean"].dtype == np.float32 and np.array_equal(d["n_applied"], r["n_applied"])
                assert np.array_equal(d["best_cost"], r["best_cost"].astype(np.float64)) and np.array_equal(d["best_x"], r["best_x"])
                worst = max(worst, (np.abs(r["mean"] - d["mean"]) / (np.abs(d["mean"]) + 1.0)).max(),
                            (np.abs(r["var"] - d["var"]).max(1) / d["var"].max(1)).max())
                assert np.array_equal(np.isnan(hd["avg_cost"]), np.isnan(hr["avg_cost"]))
    assert worst < 1.2e-7                                            # one float32 rounding of an O(1) value


# ------------------------------------------------------------------------------------------------ the class shapes
def _rel(got, ref):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1.0)).max())


@pytest.mark.parametrize("shape", S.SAMPLE_CLASS_SHAPES)
def test_sample_restated_follows_the_definition_at_the_class_shapes(shape):
    """test_gpu_search.py's inputs: a non-zero restatement error without and with the map, a zero variance gives the mean"""
    P, R, n = shape
    rng = np.random.default_rng(0)
    mean, var = rng.standard_normal((P, n)).astype(np.float32), (0.05 + rng.random((P, n))).astype(np.float32)
    proj = None
    if n in S.SAMPLE_CLASS_GROUPS:
        G, g = S.SAMPLE_CLASS_GROUPS[n]
        assert G * g == n and g <= 64
        proj = ((rng.standard_normal((G, g, g)) / np.sqrt(g)).astype(np.float32), rng.standard_normal((P, n)).astype(np.float32))
    for pr in (None,) + ((proj,) if proj is not None else ()):
        r64, r32 = S.sample(mean, var, 5, 3, R, 0, pr), S.sample_restated(mean, var, 5, 3, R, 0, pr)
        assert r32.dtype == np.float32 and r32.shape == (P, R, n) and 0.0 < _rel(r32, r64) < 2e-6
        assert np.array_equal(S.sample_restated(mean[-1:], var[-1:], 5, 3, R, P - 1, None if pr is None else (pr[0], pr[1][-1:])), r32[-1:])
        z64, z32 = S.sample(mean, 0 * var, 5, 3, R, 0, pr), S.sample_restated(mean, 0 * var, 5, 3, R, 0, pr)
        if pr is None:
            assert np.array_equal(z32, np.broadcast_to(mean[:, None, :], (P, R, n))) and np.array_equal(z64, z32.astype(np.float64))
        else:
            assert 0.0 < _rel(z32, z64) < 2e-6 and np.array_equal(z32, np.broadcast_to(z32[:, :1], z32.shape))
    tile = 1024 // (4 * ((n + 3) // 4))                          # rows of a tile: the classes the shapes stand for
    assert tile == {3: 256, 2: 256, 1024: 1, 1021: 1, 513: 1, 340: 3, 128: 8, 5: 128, 64: 16}[n]


@pytest.mark.parametrize("shape", S.UPDATE_CLASS_SHAPES)
def test_restated_update_follows_the_definition_at_the_class_shapes(shape):
    """The whole grid and ``class_options`` as test_gpu_search.py runs them: n_applied and frozen agree, every quantity under the
    4x rule has a non-zero restatement error (min_cost is exact by construction), the special options do what they are for"""
    P, R, n = shape
    rng = np.random.default_rng(2)
    worst = dict(mean=0.0, var=0.0, avg_cost=0.0, min_cost=0.0, moved=0.0)
    cases = [(f, o, None) for f, o in S.option_grid()] + S.class_options()
    assert len(cases) == 42 + 8
    for i, (family, opt, rel) in enumerate(cases):
        x, c, st = S.update_case(P, R, n, family, rng)
        if rel is not None:
            opt = S.with_abs_lower(x, c, st, opt, rel)
        d, hd = S.update(x, c, st, opt)
        r, hr = S.update_restated(x, c, st, opt)
        assert np.array_equal(d["n_applied"], r["n_applied"]) and np.array_equal(d["frozen"], r["frozen"]), (family, opt)
        assert np.array_equal(d["best_cost"], r["best_cost"].astype(np.float64)) and np.array_equal(d["best_x"], r["best_x"])
        ok = d["n_applied"] > 0
        for k in ("avg_cost", "min_cost", "moved"):
            assert np.array_equal(np.isnan(hd[k]), ~ok) and np.array_equal(np.isnan(hr[k]), ~ok)
            if ok.any():
                worst[k] = max(worst[k], _rel(hr[k][ok], hd[k][ok]))
        worst["mean"] = max(worst["mean"], _rel(r["mean"], d["mean"]))
        top = d["var"].max(1)
        worst["var"] = max(worst["var"], float((np.abs(r["var"] - d["var"]).max(1) / np.where(top > 0, top, 1.0)).max()))
        if i < 42:
            continue
        free, _ = S.update(x, c, st, dict(opt, rel_lower=-1.0, abs_lower=-1.0))
        vmax = free["var"].max(1)
        j = i - 42
        if j == 0:                                               # eliteness 2000: some weights underflow to exactly 0, not all
            cp = c[0].astype(np.float64)
            w = np.exp(-2000.0 * (cp - cp.min()) / (cp.max() - cp.min() + 1e-6))
            assert 0 < (w == 0.0).sum() < R
        elif j == 1:                                             # eliteness 0: the plain mean
            assert np.abs(d["mean"] - x.astype(np.float64).mean(1)).max() < 1e-12
        elif j == 2:                                             # one rollout kept: its x, no spread, the floor everywhere
            assert np.array_equal(d["mean"], x[np.arange(P), c.argmin(1)].astype(np.float64)) and (d["var"] == 0.3).all()
        elif j == 3:                                             # mu >= R: every counting rollout weighs, the cap alone
            assert d["var"].max() <= 0.2 and (free["var"] == d["var"]).all() and np.isnan(c).sum() == P
        elif j == 4:                                             # lr = 0: the old variances, floored
            assert np.array_equal(d["var"], np.maximum(st["var"], 0.5 * st["var"].max(1, keepdims=True)))
        elif j == 5:
            assert not d["var"].any()
        else:                                                    # problem 0: rel_lower * vmax on either side of abs_lower
            rel_floor = opt["rel_lower"] * vmax[0]
            assert (opt["abs_lower"] > rel_floor) == (j == 6) and abs(opt["abs_lower"] / rel_floor - 1.0) < 2e-3
            assert np.array_equal(d["var"][0], np.maximum(free["var"][0], max(opt["abs_lower"], rel_floor)))
    assert all(v > 0.0 for k, v in worst.items() if k != "min_cost") and worst["min_cost"] == 0.0, worst
    assert max(worst.values()) < 2e-7
    a, b = (S.update_case(P, R, n, "spread", np.random.default_rng(2)) for _ in range(2))     # seeded
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["best_cost"], b[2]["best_cost"])


# ------------------------------------------------------------------------------------------------ affine sets
def _basis(rng=None):
    rng = np.random.default_rng(0) if rng is None else rng
    return MotionBasis(n_basis=20, n_dof=7, n_points=100, param_mean=rng.standard_normal(147), param_std=0.5 + rng.random(147))


def test_a_mean_of_candidates_on_an_affine_set_stays_on_it():
    basis = _basis()
    rng = np.random.default_rng(1)
    phases = [0.0, 1.0]
    target = rng.standard_normal((2, 7, 2))
    A, b = basis.projection(phases, target)
    mean, var = rng.standard_normal((2, 147)), np.full((2, 147), 0.3)
    x = S.sample(mean, var, 3, 0, 12, 0, (A, b))
    F = basis.features(phases)                                       # [n_c, Kb]

    def residual(s):
        theta = (s * basis.param_std + basis.param_mean).reshape(s.shape[:-1] + (7, 21))
        return np.abs(np.einsum("ck,...dk->...dc", F, theta) - (target[:, None] if s.ndim == 3 else target)).max()
    assert residual(x) < 1e-11
    new, _ = S.update(x, rng.random((2, 12)) + 1.0, S.new_state(mean, var), S.options())
    assert residual(new["mean"]) < 1e-11 and residual(mean) > 0.1


def test_projection_reproduces_the_constraint_in_raw_units():
    basis = _basis(np.random.default_rng(2))
    rng = np.random.default_rng(3)
    phases, target = [0.0], rng.standard_normal((4, 7, 1))
    A, b = basis.projection(phases, target)
    assert A.shape == (7, 21, 21) and b.shape == (4, 147)
    s = rng.standard_normal((4, 147))
    got = (np.einsum("djk,rdk->rdj", A, s.reshape(4, 7, 21)).reshape(4, 147) + b) * basis.param_std + basis.param_mean
    Ar, Br = basis.constraint(phases)
    theta = (s * basis.param_std + basis.param_mean).reshape(4, 7, 21)
    want = np.einsum("jk,rdk->rdj", Ar, theta) + np.einsum("jc,rdc->rdj", Br, target)
    assert np.abs(got.reshape(4, 7, 21) - want).max() < 1e-12
    plain = MotionBasis(n_basis=20, n_dof=7)                         # no standardisation: the raw pair itself
    A0, b0 = plain.projection(phases, target)
    assert np.allclose(A0, Ar[None]) and np.allclose(b0.reshape(4, 7, 21), np.einsum("jc,rdc->rdj", Br, target))
    with pytest.raises(ValueError):
        basis.projection(phases, target[:, :, 0])


# ------------------------------------------------------------------------------------------------ convergence
QUADRATIC = [dict(n=2, x0=5.0, var0=1.0, R=10, iters=40, bound=0.01), dict(n=20, x0=1.0, var0=0.01, R=20, iters=60, bound=0.1)]
SEEDS = (0, 1, 2)


@pytest.mark.parametrize("case", QUADRATIC, ids=["n2", "n20"])
def test_the_loop_converges_on_the_norm_cost_with_the_philox_stream(case):
    """pygcem_test's problem (pygcem.py:154-183): cost |x|, defaults.  With NumPy's generator a float64 run over 200 seeds stayed
    below 1.8e-6 (n = 2) and 0.021 (n = 20) of |x0|; the Philox stream on the seeds used here is printed."""
    x0 = np.full((len(SEEDS), case["n"]), case["x0"])
    cost = lambda x: np.linalg.norm(x, axis=2)
    for i, seed in enumerate(SEEDS):
        st, _ = S.search(cost, x0[i:i + 1], case["var0"], n_rollouts=case["R"], n_iters=case["iters"], opt=S.options(tol=0.0), seed=seed)
        ratio = np.linalg.norm(st["mean"][0]) / np.linalg.norm(x0[i])
        print("n = %d seed %d: |mean| / |x0| = %.3e (bound %g)" % (case["n"], seed, ratio, case["bound"]))
        assert ratio < case["bound"]


# ------------------------------------------------------------------------------------------------ argument errors
def _args(**kw):
    base = dict(x0=np.zeros((3, 4), np.float32), var0=0.1, n_rollouts=10, n_iters=2, eliteness=10, weighting="PI-BB", cov_update="PI-BB",
                learning_rate=1.0, covar_bounds=(0.1,), tol=1e-6, project=None, seed=0, state=None, device="cpu")
    base.update(kw)
    return V.search_args(**base)


def test_search_args_marshal_on_the_cpu():
    st, opt, R, n_iters, proj, seed, was_np = _args(var0=np.arange(4.0), project=(np.zeros((2, 2, 2)), np.zeros((3, 4))))
    assert was_np and R == 10 and n_iters == 2 and proj[2:] == (2, 2) and st["iteration"] == 0
    assert st["var"].shape == (3, 4) and st["var"][1].tolist() == [0.0, 1.0, 2.0, 3.0] and torch.isinf(st["best_cost"]).all()
    assert (opt.rel_lower, opt.abs_lower, opt.abs_upper, opt.eliteness, opt.weighting) == (0.1, -1.0, -1.0, 10.0, 0)
    opt = _args(covar_bounds=None, weighting="CMA-ES", cov_update="CEM", eliteness=4)[1]
    assert (opt.rel_lower, opt.weighting, opt.cov_update) == (-1.0, 2, 1)
    again = _args(x0=None, var0=None, state=st)[0]                   # a copy: the caller's state is not the one updated
    assert again["mean"].data_ptr() != st["mean"].data_ptr() and torch.equal(again["var"], st["var"])


@pytest.mark.parametrize("kw", [
    dict(x0=np.zeros(4)), dict(x0=np.zeros((3, 0))), dict(x0=np.zeros((2, 1025))), dict(x0=None), dict(var0=None),
    dict(var0=np.zeros(3)), dict(var0=-1.0), dict(var0=float("nan")), dict(n_rollouts=0), dict(n_rollouts=1025), dict(n_rollouts=2.5),
    dict(n_iters=-1), dict(eliteness=-1.0), dict(eliteness=float("nan")), dict(weighting="CEM", eliteness=2.5),
    dict(weighting="CMA-ES", eliteness=0), dict(weighting="cem"), dict(cov_update="decay"), dict(cov_update="CMA-ES"),
    dict(learning_rate=1.5), dict(learning_rate=-0.1), dict(covar_bounds=(0.1, 0.2, 0.3, 0.4)), dict(covar_bounds=(1.5,)),
    dict(covar_bounds=(float("nan"),)), dict(tol=-1.0), dict(seed=-1), dict(seed=1.5), dict(seed=1 << 64),
    dict(project=np.zeros((2, 2, 2))), dict(project=(np.zeros((2, 3, 3)), np.zeros((3, 4)))),
    dict(project=(np.zeros((2, 2, 2)), np.zeros((2, 4)))), dict(project=(np.zeros((1, 4, 3)), np.zeros((3, 4)))),
    dict(state=dict(mean=torch.zeros(3, 4))), dict(state="state"),
])
def test_search_argument_errors_are_value_errors(kw):
    with pytest.raises(ValueError):
        _args(**kw)


def test_a_state_of_the_wrong_shape_is_refused():
    st = _args()[0]
    for key, bad in (("var", torch.zeros(3, 5)), ("n_applied", torch.zeros(3)), ("best_cost", torch.zeros(4)), ("iteration", -1),
                     ("iteration", (1 << 31) - 1), ("frozen", torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(ValueError):
            _args(state=dict(st, **{key: bad}))


def test_refine_motion_argument_errors_are_value_errors():
    basis = MotionBasis(n_basis=20, n_dof=2)
    chain = KinematicChain([dict(type="revolute", axis=[0, 0, 1]), dict(type="revolute", xyz=[0.5, 0, 0], axis=[0, 0, 1]),
                            dict(type="fixed", xyz=[0.4, 0, 0])])
    widths = (784, 42)
    assert V.refine_motion_args(basis, chain, "latent", None, 1, {}, widths) == (10, {})
    assert V.refine_motion_args(basis, chain, "params", None, 1, dict(seed=3), widths) == (20, dict(seed=3))
    assert V.refine_motion_args(basis, chain, "params", 7, 1, {}, widths)[0] == 7
    for args in ((None, chain, "latent", None, 1, {}), (basis, None, "latent", None, 1, {}), (basis, chain, "cartesian", None, 1, {}),
                 (basis, chain, "latent", None, 2, {}), (basis, chain, "latent", None, True, {}), (basis, chain, "latent", None, 0, {}),
                 (basis, chain, "latent", None, 1, dict(n_rollout=3)), (basis, chain, "latent", None, 1, dict(project=None)),
                 (MotionBasis(n_basis=20, n_dof=3), chain, "latent", None, 1, {})):
        with pytest.raises(ValueError):
            V.refine_motion_args(*(args + (widths,)))
    with pytest.raises(ValueError):
        V.writing_cost_args((0.3, 10.0), 0, StrokeCanvas(), widths)
