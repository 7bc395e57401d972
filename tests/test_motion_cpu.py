"""The motion layer's host side (vae_assoc_amd/motion.py) and the argument checks of the motion entry points, without a GPU:
the basis against tests/motion_reference.py and against the figures measured with NumPy for the reference's basis, fit-then-evaluate,
the constraint matrices, the float32 restatement against the definition, and every ValueError (marshalling on ``device="cpu"``)."""
import numpy as np
import pytest
import torch

import motion_reference as R
from vae_assoc_amd import vae_assoc as V
from vae_assoc_amd.motion import MotionBasis


# ------------------------------------------------------------------------------------------------ the basis
@pytest.mark.parametrize("kind,normalize", [("sigmoid", True), ("gaussian", True), ("gaussian", False)])
@pytest.mark.parametrize("K", [0, 1, 9, 20, 63])
def test_features_match_the_restatement(kind, normalize, K):
    b = MotionBasis(kind=kind, n_basis=K, normalize=normalize)
    z = np.concatenate([np.linspace(0.0, 1.0, 37), [-0.3, 1.4]])
    F = b.features(z)
    assert F.shape == (39, K + 1) and np.array_equal(F[:, -1], np.ones(39))
    assert np.abs(F - R.features64(kind, K, z, normalize)).max() < 1e-14
    assert np.array_equal(b.phases(), np.linspace(0.0, 1.0, 100)) and np.array_equal(b.phases(8), np.linspace(0.0, 1.0, 8))


def test_sigmoid_basis_figures():
    """K = 20 at 100 phase points: rank 21, singular values in [0.0702, 29.13], max |pinv| = 4.84; at T = 8 the rank is 8"""
    b = MotionBasis()
    assert (b.n_params, b.n_kb, b.n_dof, b.n_points) == (147, 21, 7, 100)
    F = b.features(np.linspace(0.0, 1.0, 100))
    s = np.linalg.svd(F, compute_uv=False)
    assert np.linalg.matrix_rank(F) == 21
    assert 0.0702 <= s.min() < 0.0703 and 29.12 < s.max() <= 29.13
    P = b.pinv(100)
    assert P.shape == (21, 100) and abs(np.abs(P).max() - 4.84) < 0.005
    assert np.abs(P - R.pinv64(F)).max() < 1e-12 and np.abs(P - np.linalg.pinv(F)).max() < 1e-10
    assert np.linalg.matrix_rank(b.features(b.phases(8))) == 8 and b.pinv(8).shape == (21, 8)


def test_gaussian_basis_is_truncated():
    """K = 20 normalised gaussians: 13 of 21 singular values survive the 1e-6 cut, max |pinv| ~ 5e4"""
    g = MotionBasis(kind="gaussian")
    F = g.features(g.phases())
    s = np.linalg.svd(F, compute_uv=False)
    assert int((s > 1e-6).sum()) == 13
    P = g.pinv()
    assert np.linalg.matrix_rank(P, tol=1e-3) == 13 and 4e4 < np.abs(P).max() < 7e4
    assert np.abs(P - R.pinv64(F)).max() < 1e-6 * np.abs(P).max()


def test_fit_then_evaluate_reproduces_a_trajectory_in_the_span():
    b = MotionBasis(n_points=21)
    rng = np.random.default_rng(0)
    F = b.features(b.phases())
    y = F @ rng.standard_normal((21, 7))
    assert np.abs(F @ (b.pinv(21) @ y) - y).max() < 1e-12
    params = R.fit64(y[None], b.pinv(21))
    q, sat = R.eval64(params, F, 7)
    assert np.abs(q[0] - y).max() < 1e-12 and not sat.any()


@pytest.mark.parametrize("kind", ["sigmoid", "gaussian"])
@pytest.mark.parametrize("phases", [[0.0], [0.0, 1.0], [0.0, 0.25, 0.5, 1.0]])
def test_constraint_matrices(kind, phases):
    b = MotionBasis(kind=kind)
    A, B = b.constraint(phases)
    nc = len(phases)
    assert A.shape == (21, 21) and B.shape == (21, nc)
    rng = np.random.default_rng(1)
    theta, target = rng.standard_normal(21), rng.standard_normal(nc)
    assert np.abs(b.features(phases) @ (A @ theta + B @ target) - target).max() < 1e-10
    assert np.abs(A @ A - A).max() < 1e-10
    A2, B2 = R.constraint64(R.features64(kind, 20, phases))
    assert np.abs(A - A2).max() < 1e-10 and np.abs(B - B2).max() < 1e-10
    phi, gain = b.eval_matrices(phases)
    F = b.features(b.phases())
    assert np.abs(phi - F @ A).max() < 1e-12 and np.abs(gain - F @ B).max() < 1e-12


def test_results_are_cached_and_returned_as_copies():
    b = MotionBasis()
    for f, arg in ((b.features, np.linspace(0, 1, 5)), (b.pinv, 30), (lambda p: b.constraint(p)[0], [0.0])):
        a = f(arg)
        a += 1.0
        assert np.array_equal(f(arg) + 1.0, a)
    assert ("pinv", 30) in b._cache


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_restatement_is_close_to_the_definition(shape, variant):
    c = R.case(shape, 17, variant)
    kw = R.eval_kw(c)
    q64, s64 = R.eval64(c["params"], c["phi"], c["D"], **kw)
    q32, s32 = R.eval32(c["params"], c["phi"], c["D"], **kw)
    assert q32.dtype == np.float32 and R.rel_err(q32, q64) < 1e-4
    raw = R.unclamped(c["params"], c["phi"], c["D"], c["scale"], c["shift"], c["gain"], c["target"])
    lo, hi = R.sandwich(raw, c["limits"], 4 * float(np.abs(q32 - q64).max()), 1)
    assert (lo <= s32).all() and (s32 <= hi).all() and (lo <= s64).all() and (s64 <= hi).all()
    if c["limits"] is not None and shape[2] > 2:
        assert 0 < s64.sum() < s64.size * shape[2]          # some points clamp, some do not
    if c["nc"] and c["Kb"] > c["nc"]:                       # the anchored trajectory starts at its first target (phase 0)
        assert np.abs(raw[:, 0, :] - c["target"][:, :, 0]).max() < 1e-4 * (1 + np.abs(raw).max())
    ref = q64 + 0.01
    r64, m64 = R.errors64(q64, ref)
    r32, m32 = R.errors32(q32, ref.astype(np.float32), c["Kb"])
    assert R.rel_err(r32, r64) < 1e-4 and R.rel_err(m32, m64) < 1e-4
    p64, p32 = R.fit64(q64, c["pinv"], c["scale"], c["shift"]), R.fit32(q64, c["pinv"], c["scale"], c["shift"])
    assert p32.dtype == np.float32 and R.rel_err(p32, p64) < 1e-3


def test_class_shapes_stand_for_their_slab_classes():
    assert [R.slab_of(*s) for s in R.CLASS_SHAPES] == [(512, 256), (144, 36), (204, 51), (63, 128), (64, 16)]
    assert [s[2] % R.slab_of(*s)[0] for s in R.CLASS_SHAPES] == [0, 16, 1, 1, 44]                 # the last slab
    assert [-(-s[2] // R.slab_of(*s)[0]) for s in R.MOMENT_CLASS_SHAPES] == [5, 8]                # slabs of the moment cases
    assert R.CLASS_ROWS == (1, 5, 17) and R.CLASS_VARIANTS[:len(R.VARIANTS)] == R.VARIANTS
    assert [(S + 3) // 4 for S in R.MOMENT_CLASS_S] == [1, 2, 3] and [S % 4 for S in R.MOMENT_CLASS_S] == [3, 1, 1]


@pytest.mark.parametrize("shape", R.CLASS_SHAPES)
def test_restatement_is_close_to_the_definition_at_the_class_shapes(shape):
    """test_gpu_motion.py's class sweep: every quantity under its 4x rule has a non-zero restatement error over the rows and
    variants it runs, some points clamp and some do not, and the anchors of three and four phases hold"""
    D, Kb, T = shape
    worst = dict.fromkeys(("trajectory", "rmse", "max_abs", "fit"), 0.0)
    for rows in R.CLASS_ROWS:
        for variant in R.CLASS_VARIANTS:
            c = R.case(shape, rows, variant)
            again = R.case(shape, rows, variant)
            assert all(np.array_equal(c[k], again[k]) for k in ("params", "phi", "pinv")) and c["rows"] == rows
            assert not np.array_equal(c["params"], R.case(shape, rows, variant, seed=1)["params"])
            kw = R.eval_kw(c)
            q64, s64 = R.eval64(c["params"], c["phi"], D, **kw)
            q32, s32 = R.eval32(c["params"], c["phi"], D, **kw)
            raw = R.unclamped(c["params"], c["phi"], D, c["scale"], c["shift"], c["gain"], c["target"])
            lo, hi = R.sandwich(raw, c["limits"], 4 * float(np.abs(q32 - q64).max()), 1)
            assert (lo <= s32).all() and (s32 <= hi).all() and (lo <= s64).all() and (s64 <= hi).all()
            if c["limits"] is not None:
                assert 0 < s64.sum() < s64.size * T
            if variant in ("anchor3", "anchor4"):
                nc = c["nc"]
                assert nc == int(variant[-1]) and c["gain"].shape == (T, nc) and c["target"].shape == (rows, D, nc)
                F = R.features64("sigmoid", Kb - 1, np.array(R.ANCHOR_PHASES[:nc]))      # the trajectory at the anchored phases
                A, Bm = R.constraint64(F)
                th = c["params"].astype(np.float64).reshape(rows, D, Kb)
                at = np.einsum("ck,rdk->rdc", F @ A, th) + np.einsum("cj,rdj->rdc", F @ Bm, c["target"].astype(np.float64))
                assert np.abs(at - c["target"]).max() < 1e-9 * (1 + np.abs(raw).max())
                assert np.abs(raw[:, [0, T - 1][:1 if nc == 3 else 2], :].transpose(0, 2, 1)
                              - c["target"][:, :, [0, 3][:1 if nc == 3 else 2]]).max() < 1e-4 * (1 + np.abs(raw).max())
            refp = (c["params"] + 0.1).astype(np.float32)
            kw_ref = dict(kw, gain=None, target=None)
            e64 = R.errors64(q64, R.eval64(refp, c["phi"], D, **kw_ref)[0])
            e32 = R.errors32(q32, R.eval32(refp, c["phi"], D, **kw_ref)[0], Kb)
            f64, f32 = R.fit64(q64.astype(np.float32), c["pinv"], c["scale"], c["shift"]), \
                R.fit32(q64.astype(np.float32), c["pinv"], c["scale"], c["shift"])
            for name, a, b in (("trajectory", q32, q64), ("rmse", e32[0], e64[0]), ("max_abs", e32[1], e64[1]), ("fit", f32, f64)):
                worst[name] = max(worst[name], R.rel_err(a, b))
    assert all(0.0 < v < 1e-3 for v in worst.values()), worst
    assert worst["trajectory"] < 1e-5 and worst["rmse"] < 1e-5 and worst["max_abs"] < 1e-4


@pytest.mark.parametrize("S", R.MOMENT_CLASS_S)
@pytest.mark.parametrize("shape", R.MOMENT_CLASS_SHAPES)
def test_moments_restatement_at_the_tile_classes(shape, S):
    worst = [0.0, 0.0]
    for rows in (1, 5):
        for variant in ("plain", "all"):
            c = R.case(shape, rows, variant, S=S)
            assert c["params"].shape == (rows, S, shape[0] * shape[1])
            both = R.moments_both(c["params"], c["phi"], shape[0], **R.eval_kw(c))
            (m64, v64, _), (m32, v32) = both["r64"], both["r32"]
            worst = [max(worst[0], R.rel_err(m32, m64)), max(worst[1], R.var_err(v32, v64))]
            lo, hi = both["counts"](4.0 * both["worst"])
            assert (lo <= hi).all() and 0 < both["worst"] < 1e-4
            assert np.array_equal(R.case(shape, rows, variant, S=S)["params"], c["params"])
    assert 0.0 < worst[0] < 1e-5 and 0.0 < worst[1] < 1e-5, worst


def test_moments_restatement():
    c = R.case((7, 21, 100), 5, "all", S=7)
    kw = R.eval_kw(c)
    m64, v64, f64 = R.moments64(c["params"], c["phi"], 7, **kw)
    m32, v32, f32, worst = R.moments32(c["params"], c["phi"], 7, **kw)
    lo, hi = R.moments64(c["params"], c["phi"], 7, delta=4 * worst, **kw)[3:]
    assert 0 < worst < 1e-4 and (lo <= f64 * 700 + 1e-9).all() and (f64 * 700 <= hi + 1e-9).all() and (lo > 0).any()
    assert R.rel_err(m32, m64) < 1e-4 and R.var_err(v32, v64) < 1e-4 and np.abs(f32 - f64).max() < 0.01
    both = R.moments_both(c["params"], c["phi"], 7, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(both["r64"], (m64, v64, f64))) and both["worst"] == worst
    assert all(np.array_equal(a, b) for a, b in zip(both["r32"], (m32, v32)))
    assert all(np.array_equal(a, b) for a, b in zip(both["counts"](4 * worst), (lo, hi)))
    each = np.stack([R.eval64(c["params"][:, k], c["phi"], 7, **kw)[0] for k in range(7)], 1)
    assert np.abs(each.mean(1) - m64).max() < 1e-12 and np.abs(each.var(1) - v64).max() < 1e-12
    one = R.moments32(c["params"][:, :1], c["phi"], 7, **kw)
    assert np.array_equal(one[0], R.eval32(c["params"][:, 0], c["phi"], 7, **kw)[0]) and not one[1].any()


# ------------------------------------------------------------------------------------------------ errors
def test_basis_argument_errors():
    with pytest.raises(ValueError, match="param_std"):
        MotionBasis(param_std=np.r_[np.ones(146), 0.0])
    with pytest.raises(ValueError, match="param_std"):
        MotionBasis(param_std=np.r_[np.ones(146), np.inf])
    with pytest.raises(ValueError, match="param_mean"):
        MotionBasis(param_mean=np.r_[np.ones(146), np.nan])
    with pytest.raises(ValueError, match="param_mean"):
        MotionBasis(param_mean=np.ones(146))
    with pytest.raises(ValueError, match="n_basis"):
        MotionBasis(n_basis=64)
    with pytest.raises(ValueError, match="n_dof"):
        MotionBasis(n_dof=17)
    with pytest.raises(ValueError, match="n_dof"):
        MotionBasis(n_dof=0)
    with pytest.raises(ValueError, match="n_points"):
        MotionBasis(n_points=1025)
    with pytest.raises(ValueError, match="n_points"):
        MotionBasis(n_points=0)
    with pytest.raises(ValueError, match="kind"):
        MotionBasis(kind="tanh")
    with pytest.raises(ValueError, match="limits"):
        MotionBasis(limits=np.zeros((6, 2)))
    b = MotionBasis(n_basis=63, n_dof=16, n_points=1024)       # the largest sizes are fine
    assert b.n_params == 1024
    with pytest.raises(ValueError, match="phases"):
        b.constraint([0.0, 0.1, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match="phases"):
        b.constraint([])
    with pytest.raises(ValueError, match="T ="):
        b.pinv(1025)


def test_marshalling_errors_on_cpu():
    dev = torch.device("cpu")
    b = MotionBasis(param_mean=np.zeros(147), param_std=np.ones(147), limits=np.c_[-np.ones(7), np.ones(7)])
    p = np.zeros((5, 147), np.float32)
    out = V.motion_eval_args(p, b, dict(phases=[0.0], target=np.zeros((5, 7, 1))), None, p, dev)
    assert out[0].shape == (5, 147) and out[1]["phi"].shape == (100, 21) and out[1]["gain"].shape == (100, 1)
    assert out[1]["nc"] == 1 and out[1]["limits"].shape == (7, 2) and out[1]["scale"].dtype == torch.float32 and out[4]
    assert V.motion_eval_args(torch.zeros(5, 147), b, None, None, None, dev)[4] is False
    for bad in (dict(params=np.zeros((5, 146))), dict(params=np.zeros(147)), dict(basis="sigmoid"),
                dict(anchor=dict(phases=[0.0], target=np.zeros((4, 7, 1)))), dict(anchor=dict(phases=[0.0], target=np.zeros((5, 7, 2)))),
                dict(anchor=dict(phases=[0.0])), dict(anchor=dict(phases=[0.0] * 5, target=np.zeros((5, 7, 5)))),
                dict(reference=np.zeros((5, 100, 7)), reference_params=p), dict(reference=np.zeros((5, 99, 7))),
                dict(reference=np.zeros((4, 100, 7))), dict(reference_params=np.zeros((4, 147)))):
        kw = dict(params=p, basis=b, anchor=None, reference=None, reference_params=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.motion_eval_args(device=dev, **kw)
    t, pinv, sc, sh, was_np = V.motion_fit_args(np.zeros((3, 8, 7)), b, dev)
    assert t.shape == (3, 8, 7) and pinv.shape == (21, 8) and sc.shape == (147,) and was_np
    for bad in (np.zeros((3, 8, 6)), np.zeros((8, 7)), np.zeros((3, 0, 7)), np.zeros((1, 1025, 7))):
        with pytest.raises(ValueError):
            V.motion_fit_args(bad, b, dev)
    s, mats, _ = V.motion_moments_args(np.zeros((3, 4, 147)), b, None, dev)
    assert s.shape == (3, 4, 147) and mats["nc"] == 0 and mats["target"] is None
    for bad in (np.zeros((3, 4, 146)), np.zeros((3, 147)), np.zeros((3, 0, 147))):
        with pytest.raises(ValueError):
            V.motion_moments_args(bad, b, None, dev)
    with pytest.raises(ValueError):
        V.motion_moments_args(np.zeros((3, 4, 147)), b, dict(phases=[0.0], target=np.zeros((2, 7, 1))), dev)
    X = [np.zeros((6, 784), np.float32), np.zeros((6, 147), np.float32)]
    args = dict(X=X, basis=b, modality=1, present=None, n_samples=3, eps=np.zeros((6, 3, 20)), anchor=None, widths=(784, 147), n_z=20,
                device=dev)
    (ts, rows, was_np, _, _, _, S, e), mats = V.predict_motion_args(**args)
    assert rows == 6 and S == 3 and e.shape == (6, 3, 20) and was_np
    for bad in (dict(modality=0), dict(modality=2), dict(modality=True), dict(n_samples=-1), dict(eps=np.zeros((6, 2, 20))),
                dict(n_samples=0), dict(basis=MotionBasis(n_dof=6)), dict(X=[X[0], None, None]),
                dict(anchor=dict(phases=[0.0], target=np.zeros((5, 7, 1))))):
        with pytest.raises(ValueError):
            V.predict_motion_args(**dict(args, **bad))
