"""Sigma-lognormal strokes without a GPU: the float64 definition of tests/lognormal_reference.py (Jacobian,
fit, sampler), its float32 restatement, the host side (``lognormal_initial_guess``, ``balanced_sample_counts``) and the validators
of the Python surface, which run on ``device="cpu"``."""
import numpy as np
import pytest
import torch

import lognormal_cases as LC
import lognormal_reference as LR
from vae_assoc_amd import _args as M
from vae_assoc_amd.lognormal import balanced_sample_counts, lognormal_initial_guess

START = np.asarray(LR.START_CASE)


@pytest.mark.parametrize("C", (1, 3, 6, 12))
def test_jacobian_agrees_with_central_differences(C):
    """T = 100.  The step is 1e-7: the truncation error of a central difference falls with h^2 (1e-8 of the largest entry at
    h = 1e-6 and C = 12, where a narrow component switches on between two time points, 1e-10 here), and the rounding error,
    1e-16 / h = 1e-9 of the values differenced, stays below the bound of 1e-8 of the largest entry (3e-10 to 2e-9 seen)."""
    p = LR.separated_params(C, np.random.default_rng(C))
    _, _, JP, JV = LR.jacobian(p, START, LR.T_CASE, LR.DT_CASE)
    h = 1e-7
    for J, which in ((JP, 0), (JV, 1)):
        num = np.zeros_like(J)
        for i in range(6 * C):
            a, b = p.reshape(-1).copy(), p.reshape(-1).copy()
            a[i] += h
            b[i] -= h
            num[:, :, i] = (LR.stroke(a.reshape(-1, 6), START, LR.T_CASE, LR.DT_CASE)[which]
                            - LR.stroke(b.reshape(-1, 6), START, LR.T_CASE, LR.DT_CASE)[which]) / (2 * h)
        err = np.abs(num - J).max() / np.abs(J).max()
        print("C = %d %s Jacobian: %.2e of the largest entry" % (C, ("position", "velocity")[which], err))
        assert err < 1e-8


def test_restatement_agrees_with_the_definition():
    """eval, sample and four fit tries.  The bounds are float32's: an error of 6e-8 in ln t, divided by sigma >= 0.15 and multiplied
    by |z| <= 5 in the exponent, is about 1e-5 of a velocity term, and a hundred of them are added: 1e-4 on values of order 1 to 10
    (|ref| + 1 below); the loss after four tries inherits the parameters' drift and gets 1e-3."""
    rng = np.random.default_rng(0)
    P = np.stack([LR.separated_params(8, rng) for _ in range(5)])
    st = np.tile(START, (5, 1))
    cnt = np.array([8, 5, 1, 0, 8])
    for T in (63, 100, 257):
        a, b = LR.evaluate(P, cnt, st, T, 0.01), LR.evaluate_restated(P, cnt, st, T, 0.01)
        worst = max(LR.rel_err(b[0], a[0]), LR.rel_err(b[1], a[1]))
        print("eval T = %d: worst |err| / (|ref| + 1) = %.2e" % (T, worst))
        assert worst < 1e-4
        assert np.array_equal(a[0][3], np.broadcast_to(st[3], (T, 2)))
    for shift in (False, True):
        a = LR.sample(P, cnt, st, 100, 0.01, 3, 11, shift_mean=shift)
        b = LR.sample_restated(P, cnt, st, 100, 0.01, 3, 11, shift_mean=shift)
        worst = max(LR.rel_err(b[0], a[0]), LR.rel_err(b[1], a[1]))
        print("sample shift_mean = %s: worst %.2e" % (shift, worst))
        assert worst < 1e-4
    case = LR.step_case(3, 3, LR.step_seed("3x3"))
    a, b = LR.run_step_case(case, "full", 4, False), LR.run_step_case(case, "full", 4, True)
    worst = LR.rel_err(b["loss"], a["loss"])
    print("fit, four tries: loss worst %.2e" % worst)
    assert worst < 1e-3 and np.array_equal(a["accepted"], b["accepted"]) and np.array_equal(a["iterations"], b["iterations"])


@pytest.mark.parametrize("C", (1, 2, 3, 4, 6))
def test_initial_guess_and_forty_iterations_reproduce_the_stroke(C):
    for seed in LR.CONTRACT_SEEDS[C]:
        s, p = LR.contract_stroke(C, seed)
        g, cnt = lognormal_initial_guess(s[None], START[None], LR.DT_CASE)
        assert g.shape == (1, 8, 6) and cnt.dtype == np.int32 and cnt[0] == C
        assert np.all(g[0, C:] == 0.0)
        ext = LR.extent(s)
        off0 = np.abs(LR.stroke(g[0, :C], START, LR.T_CASE, LR.DT_CASE)[0] - s).max() / ext
        r = LR.fit_row(s, g[0, :C], START, LR.DT_CASE, n_iters=40)
        off = np.abs(LR.stroke(r["params"], START, LR.T_CASE, LR.DT_CASE)[0] - s).max() / ext
        print("C = %d seed %d: the guess is off by %.2f of the extent, the fit by %.1e (status %d after %d tries)"
              % (C, seed, off0, off, r["status"], r["iterations"]))
        assert off < 1e-9 and r["status"] in (0, 1)


def test_initial_guess_defaults_and_errors():
    s, _ = LR.contract_stroke(3, 0)
    two = np.stack([s, s[::-1]])
    g, cnt = lognormal_initial_guess(two, max_components=2)
    assert g.shape == (2, 2, 6) and (cnt <= 2).all() and np.isfinite(g).all()
    g1, _ = lognormal_initial_guess(two, start=two[:, 0], dt=1.0 / 99, max_components=2)
    assert np.array_equal(g, g1)
    assert lognormal_initial_guess(np.zeros((1, 5, 2)))[1][0] == 0                  # a stroke that stands still
    for bad in (dict(strokes=np.zeros((2, 5, 3))), dict(strokes=np.zeros((2, 1, 2))), dict(strokes=np.zeros((2, 1025, 2))),
                dict(strokes=two, dt=0.0), dict(strokes=two, max_components=17), dict(strokes=two, start=np.zeros((3, 2))),
                dict(strokes=two, sigma=0.0), dict(strokes=two, floor=2.0)):
        with pytest.raises(ValueError):
            lognormal_initial_guess(**bad)
    assert lognormal_initial_guess(np.zeros((2, 1, 2)), dt=0.1)[0].shape == (2, 8, 6)


def test_sampler_draws_have_a_third_of_their_scale():
    """20,000 draws per ratio: the standard error of a standard deviation is 1 / sqrt(2 n) = 0.5 %, the bound is 3 %."""
    P = np.stack([LR.separated_params(4, np.random.default_rng(3)) for _ in range(10)])
    S_, amp, ang, stra = 500, 0.2, np.pi / 9, 0.1
    for nrm in (LR.normals(5, 10, S_, 4), LR.normals_f32(5, 10, S_, 4)):
        pert = LR.perturb(P, None, nrm, amp, ang, stra, np.float64)
        D, ths, the = P[:, None, :, 0], P[:, None, :, 4], P[:, None, :, 5]
        r0 = (pert[..., 0] - D) / (amp * D)
        r1 = (pert[..., 4] - ths) / ang
        r2 = ((pert[..., 5] - the) - (pert[..., 4] - ths)) / (stra * (the - ths))
        for r in (r0, r1, r2):
            assert r.size == 20000 and abs(r.std() * 3.0 - 1.0) < 0.03 and abs(r.mean()) < 0.01
        assert np.array_equal(pert[..., 1:4], np.broadcast_to(P[:, None, :, 1:4], pert[..., 1:4].shape))
    assert not np.array_equal(LR.words(5, 2, 2, 2), LR.words(6, 2, 2, 2))
    assert np.array_equal(LR.words(5, 5, 2, 3)[2:], LR.words(5, 3, 2, 3, row_offset=2))


def test_shift_mean_gives_zero_mean_samples():
    P = np.stack([LR.separated_params(3, np.random.default_rng(4)) for _ in range(2)])
    st = np.tile(START, (2, 1))
    shifted, _ = LR.sample(P, None, st, 100, 0.01, 4, 1, shift_mean=True)
    plain, _ = LR.sample(P, None, st, 100, 0.01, 4, 1, shift_mean=False)
    assert np.abs(shifted.mean(axis=2)).max() < 1e-14
    assert np.abs(plain - plain.mean(axis=2, keepdims=True) - shifted).max() < 1e-14
    r32, _ = LR.sample_restated(P, None, st, 100, 0.01, 4, 1, shift_mean=True)
    assert np.abs(r32.astype(np.float64).mean(axis=2)).max() < 1e-6


def test_balanced_sample_counts():
    labels = ["a", "b", "a", "c", "a", "b"]
    assert balanced_sample_counts(labels, 100).tolist() == [25, 33, 25, 50, 25, 33]
    assert balanced_sample_counts(labels, 3).tolist() == [0, 1, 0, 1, 0, 1]
    assert balanced_sample_counts([], 10).tolist() == []
    with pytest.raises(ValueError):
        balanced_sample_counts(labels, -1)


def test_step_cases_have_a_decision_margin():
    """every accept decision of the definition over the compared tries is clear by more than 1e-3 L"""
    for name, N, C, counts, variant in LR.STEP_CASES:
        case = LR.step_case(N, C, LR.step_seed(name), counts)
        r = LR.run_step_case(case, variant, 4, False)
        assert min(LR.margins(t) for t in r["tries"]) > 1e-3, name
        assert (r["iterations"][case["count"] > 0] == 4).all() and (r["iterations"][case["count"] == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ the second pass's conditions
def _clear_and_agreed(case, refs):
    for it, (r64, r32) in refs.items():
        assert LC.margin(r64) > 1e-3 and LC.decisions_agree(r64, r32), it
        assert np.array_equal(r64["iterations"], r32["iterations"]) and np.array_equal(r64["accepted"], r32["accepted"])
        assert (r64["iterations"] == np.where(case["count"] > 0, it, 0)).all()


@pytest.mark.parametrize("C", (3, 6, 9, 12, 15))
def test_tile_cases_have_a_decision_margin_and_an_agreeing_restatement(C):
    """every (C, T) of LC.TILE_SHAPES, after 1 and 4 tries; at T = 1 the loss is exactly 0 and nothing is accepted"""
    shapes = [s for s in LC.TILE_SHAPES if s[0] == C]
    assert len(shapes) in (6, 7) and len(LC.TILE_SHAPES) == 33
    for _, T in shapes:
        case, refs = LC.tile_case(C, T)
        assert case["target"].shape == (2, T, 2) and case["dt"] == float(np.float32(0.01 if T == 1 else 1.0 / (T - 1)))
        _clear_and_agreed(case, refs)
        if T == 1:
            for it in LC.TRIES:
                for r in refs[it]:
                    assert not r["loss"].any() and not r["loss0"].any() and not r["accepted"].any() and (r["status"] == 1).all()
                    assert np.array_equal(r["params"], case["init"].astype(np.float64))


def test_step_case_keeps_its_bits_at_the_default_t_and_dt():
    a, b = LR.step_case(3, 3, 1000), LR.step_case(3, 3, 1000, None, LR.T_CASE, LR.DT_CASE)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["target"].shape == (3, LR.T_CASE, 2)
    assert LR.step_case(2, 3, 1000, T=17, dt=0.05)["target"].shape == (2, 17, 2)


@pytest.mark.parametrize("name", sorted(LC.RAGGED_CASES))
def test_ragged_cases_have_a_decision_margin(name):
    case, refs = LC.ragged_case(name)
    _clear_and_agreed(case, refs)
    assert (case["count"] < case["init"].shape[1]).any() and case["init"].shape[1] in (4, 12)
    if name == "per-row-12":
        assert case["opt"]["free"].shape == (3, 12, 6) and 0 < case["opt"]["free"].mean() < 1


def test_overflow_rows_take_one_rejection_each():
    """D = 3e38: every try of the restatement ends at a pivot that is not > 0; one component, only sigma free, D = 1e37: every
    pivot passes and the solution is not finite.  Status 2 after 8 tries, none accepted, no finite loss; the float64 definition
    does not overflow on either row (which is why those rows are compared with the restatement)."""
    for case, which in ((LC.overflow_case(), "pivot"), (LC.x_reject_case(), "x")):
        n = LC.OVERFLOW_ROW
        kw = dict(n_iters=40, tol=case["opt"]["tol"], free=case["opt"].get("free"))
        with np.errstate(all="ignore"):
            r32 = LR.fit_row(case["target"][n], case["init"][n], case["start"][n], case["dt"], restated=True, **kw)
        r64 = LR.fit_row(case["target"][n], case["init"][n], case["start"][n], case["dt"], **kw)
        assert np.isfinite(case["init"]).all()
        assert r32["solves"] == [which] * 8 and all(ln is None for _, ln in r32["tries"])
        assert (r32["status"], r32["iterations"], r32["accepted"]) == (2, 8, 0)
        assert not np.isfinite(r32["loss0"]) and not np.isfinite(r32["loss"])
        assert np.array_equal(r32["params"], case["init"][n])
        assert np.isfinite(r64["loss0"]) and set(r64["solves"]) == {"ok"}


def test_solve_says_which_rejection_it_took():
    why = []
    assert LR._solve(np.array([[4.0, 2.0], [2.0, 1.0]]), np.ones(2), why) is None and why == ["pivot"]
    assert LR._solve(np.array([[np.inf]]), np.array([np.inf]), why) is None and why == ["pivot", "x"]
    assert np.allclose(LR._solve(np.array([[4.0, 2.0], [2.0, 3.0]]), np.array([2.0, 1.0]), why), [0.5, 0.0]) and why[-1] == "ok"
    assert LR._solve(np.array([[np.nan]]), np.ones(1)) is None


@pytest.mark.parametrize("name", sorted(LC.TOL_CASES))
def test_tol_cases_end_in_the_same_try_with_a_convergence_margin(name):
    case, refs = LC.tol_case(name)
    r64, r32 = refs[LC.TOL_TRIES]
    tol = case["opt"]["tol"]
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(r64[k], r32[k]), k
    assert (r64["status"] == 0).all() and (r64["iterations"] < LC.TOL_TRIES).all()
    for n, tries in enumerate(r64["tries"]):
        print("%s row %d: %d tries, convergence margin %.3f, accept margin %.5f" % (name, n, len(tries), LC.conv_margin(tries, tol),
                                                                                   LR.margins(tries)))
        assert LC.conv_margin(tries, tol) > 1e-3
        l, ln = tries[-1]
        assert ln < l and l - ln < tol * l                                      # the last try is the one that converged
        if name in LC.TOL_BETWEEN:                                              # tol L(new) <= L - L(new) < tol L, both clearly
            assert l - ln > 1.01 * tol * ln and l - ln < 0.99 * tol * l
            assert all((x - y) > 1.01 * tol * y for x, y in tries if y is not None and y < x)
    assert tol <= 1e-2 or name.startswith("tol-0.5")


def test_clip_bound_and_weight_cases():
    for name, (_, row, _, clip) in LC.CLIP_CASES.items():
        case, refs = LC.clip_case(name)
        _clear_and_agreed(case, refs)
        on64, on32 = refs[4][0]["params"][row, :, 3] == clip, refs[4][1]["params"][row, :, 3] == np.float32(clip)
        assert on64.any() and np.array_equal(on64, on32), name
    for name in LC.BOUND_CASES:
        case, refs = LC.bound_case(name)
        _clear_and_agreed(case, refs)
        side = "lo" if "lo" in case["opt"] else "hi"
        assert (side == "lo") == ("hi" not in case["opt"])
        assert (refs[4][0]["params"] == np.asarray(case["opt"][side])[None, None, :]).any(), name      # the bound binds
    for N, C in LC.WEIGHT_SHAPES:
        for w in LC.WEIGHTS:
            case, refs = LC.weight_case(N, C, w)
            _clear_and_agreed(case, refs)
        for restated in (False, True):
            r = LC.run(LC.make(N, C, 1000, weights=(0.0, 0.0)), 40, restated, tol=1e-9)
            assert (r["status"] == 2).all() and (r["iterations"] == 8).all() and not r["accepted"].any() and not r["loss"].any()


def test_sampler_edges_in_the_reference():
    """what tests/test_gpu_lognormal.py section 11 leans on: the stream at row_offset = 2^32 - N, a count = 0 row under shift_mean
    (start minus the butterfly mean of start: tiny, not 0), and T = 1"""
    N = 3
    off = 2 ** 32 - N
    w = LR.words(99, N, 2, 4, row_offset=off)
    assert np.array_equal(w[1:], LR.words(99, N - 1, 2, 4, row_offset=off + 1)) and not np.array_equal(w, LR.words(99, N, 2, 4))
    for shape in LC.SAMPLE_EDGE_SHAPES:
        params, count, start, dt = LC.sample_edge(shape)
        Nn, S, C, T = shape
        for shift in (False, True):
            a = LR.sample(params, count, start, T, dt, S, 7, shift_mean=shift)
            b = LR.sample_restated(params, count, start, T, dt, S, 7, shift_mean=shift)
            assert a[0].shape == (Nn, S, T, 2) and np.isfinite(a[0]).all() and np.isfinite(b[0]).all()
            assert LR.rel_err(b[0], a[0]) < 1e-4
            for n in np.flatnonzero(count == 0):
                assert np.abs(b[0][n]).max() < 1e-6 if shift else np.array_equal(b[0][n], np.broadcast_to(start[n], (S, T, 2)))
    assert (LC.sample_edge(LC.SAMPLE_EDGE_SHAPES[0])[0][..., 0] < 0).any()


# ------------------------------------------------------------------------------------------------ the validators
def _p(N=3, C=4):
    return np.zeros((N, C, 6), dtype=np.float32)


def test_eval_args():
    p, cnt, st, T, dt, was_np = M.lognormal_eval_args(_p(), 100, None, None, None, "cpu")
    assert p.shape == (3, 4, 6) and cnt.tolist() == [4, 4, 4] and cnt.dtype == torch.int32 and st.shape == (3, 2)
    assert T == 100 and dt == float(np.float32(1.0 / 99)) and was_np
    p, cnt, st, T, dt, was_np = M.lognormal_eval_args(torch.zeros(3, 4, 6), 1, [0, 4, 2], [1.0, 2.0], 0.5, "cpu")
    assert not was_np and cnt.tolist() == [0, 4, 2] and st.tolist() == [[1.0, 2.0]] * 3 and dt == 0.5
    for bad in (dict(params=np.zeros((3, 4, 5))), dict(params=np.zeros((3, 17, 6))), dict(params=np.zeros((3, 6))),
                dict(n_points=1025), dict(n_points=0), dict(n_points=1), dict(count=[0, 5, 1]), dict(count=[0, -1, 1]),
                dict(count=[1, 1]), dict(count=[0.5, 1, 1]), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")),
                dict(start=np.zeros((2, 2))), dict(params=None)):
        kw = dict(params=_p(), n_points=100, count=None, start=None, dt=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            M.lognormal_eval_args(device="cpu", **kw)


def test_fit_args():
    s, _ = LR.contract_stroke(2, 0)
    strokes = np.stack([s, s]).astype(np.float32)
    base = dict(strokes=strokes, init=None, count=None, start=None, dt=None, max_components=8, n_iters=40, weights=(1.0, 1e-3),
                free=None, bounds=None, tol=1e-9)
    st, p, cnt, start, dt, opts, fr, lo, hi, was_np = M.lognormal_fit_args(device="cpu", **base)
    assert st.shape == (2, 100, 2) and p.shape == (2, 8, 6) and cnt.tolist() == [2, 2] and was_np
    assert torch.equal(start, st[:, 0, :]) and opts == (40, 1.0, 1e-3, 1e-9) and fr is None and lo is None and hi is None
    kw = dict(base, init=_p(2, 3), count=[3, 1], free=[1, 1, 0, 0, 1, 1], bounds=(None, [1, 1, 1, 1, 1, np.inf]), dt=0.01)
    st, p, cnt, start, dt, opts, fr, lo, hi, was_np = M.lognormal_fit_args(device="cpu", **kw)
    assert fr.dtype == torch.uint8 and fr.tolist() == [1, 1, 0, 0, 1, 1] and lo is None and hi.shape == (6,) and cnt.tolist() == [3, 1]
    assert M.lognormal_fit_args(device="cpu", **dict(kw, free=np.ones((2, 3, 6))))[6].shape == (2, 3, 6)
    for bad in (dict(strokes=np.zeros((2, 100, 3))), dict(strokes=np.zeros((2, 1025, 2))), dict(strokes=np.zeros((2, 1, 2))),
                dict(strokes=None), dict(dt=0.0), dict(count=[1, 1]), dict(max_components=17), dict(n_iters=-1),
                dict(weights=(1.0,)), dict(weights=(1.0, -1.0)), dict(tol=-1.0), dict(init=_p(3, 3)), dict(init=_p(2, 17)),
                dict(init=_p(2, 3), count=[4, 0]), dict(init=_p(2, 3), free=np.ones((2, 4, 6))), dict(init=_p(2, 3), free=[1, 1]),
                dict(bounds=([0] * 6,)), dict(bounds=([0] * 5, None)), dict(bounds=([1] * 6, [0] * 6)),
                dict(bounds=([float("nan")] * 6, None))):
        with pytest.raises(ValueError):
            M.lognormal_fit_args(device="cpu", **dict(base, **bad))
    assert M.lognormal_fit_args(device="cpu", **dict(base, strokes=np.zeros((2, 1, 2)), dt=0.1))[0].shape == (2, 1, 2)


def test_augment_args():
    assert M.lognormal_augment_args(np.zeros((1, 5, 2)), None, None, None, None, None, "cpu") == "strokes"
    assert M.lognormal_augment_args(None, _p(), None, None, None, 100, "cpu") == "params"
    for strokes, params, n_points in ((None, None, 100), (np.zeros((1, 5, 2)), _p(), 100), (None, _p(), None)):
        with pytest.raises(ValueError):
            M.lognormal_augment_args(strokes, params, None, None, None, n_points, "cpu")
    assert M.lognormal_sample_options(10, 0, 0.2, np.pi / 9, 0.1)[:2] == (10, 0)
    for bad in ((0, 0, 0.2, 0.3, 0.1), (10, -1, 0.2, 0.3, 0.1), (10, 0, -0.2, 0.3, 0.1), (10, 0, 0.2, float("inf"), 0.1),
                (10, 0, 0.2, 0.3, "x"), (2.5, 0, 0.2, 0.3, 0.1)):
        with pytest.raises(ValueError):
            M.lognormal_sample_options(*bad)
