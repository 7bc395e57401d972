"""Pen-path kinematics and stroke rendering without a GPU: the chain (vae_assoc_amd/kinematics.py) against the
reference's own numbers and closed forms, the rasteriser's definition (tests/render_reference.py) on cases with exact answers and
against a brute-force raster, the float32 restatement of the kernels against the definition on every case of tests/test_gpu_render.py,
and every ValueError of the new calls (marshalling on ``device="cpu"``)."""
import numpy as np
import pytest
import torch

import render_reference as R
from vae_assoc_amd import vae_assoc as V
from vae_assoc_amd.kinematics import KinematicChain, StrokeCanvas
from vae_assoc_amd.motion import MotionBasis


# ------------------------------------------------------------------------------------------------ the chain
def test_fixture_chain_reproduces_the_writers_block_center():
    """The writer's seed pose puts the pen on its block centre, given to 3 decimals (baxter_writer.py:29-32); measured: 3.7e-4 at
    most.  All-zero angles: (0.82504, -1.02004, 0.32098)."""
    fx = R.fixture()
    chain = KinematicChain(fx["joints"])
    assert chain.n_dof == 7 and len(chain.joints) == 12
    tip = chain.forward(fx["seed_pos"])
    assert np.abs(tip - np.array(fx["block_center"])).max() < 1e-3
    assert np.abs(chain.forward(np.zeros(7)) - np.array([0.82504, -1.02004, 0.32098])).max() < 1e-5
    lim = chain.limits
    assert lim.shape == (7, 2) and (lim[:, 0] < np.array(fx["seed_pos"])).all() and (np.array(fx["seed_pos"]) < lim[:, 1]).all()


@pytest.mark.parametrize("joints", [R.fixture_joints(7), R.fixture_joints(3), R.random_joints(16, 0), R.random_joints(5, 1)])
def test_packed_chain_equals_the_unpacked_product(joints):
    chain = KinematicChain(joints)
    frames, axes = chain.packed(np.float64)
    assert frames.shape == (chain.n_dof + 1, 3, 4) and axes.shape == (chain.n_dof, 3)
    q = np.random.default_rng(2).uniform(-3.0, 3.0, (9, 4, chain.n_dof))
    assert np.abs(R.fk64(q, frames, axes) - chain.forward(q)).max() < 1e-12
    f32, a32 = chain.packed()
    assert f32.dtype == np.float32 and a32.dtype == np.float32
    assert np.array_equal(f32, frames.astype(np.float32)) and np.array_equal(a32, axes.astype(np.float32))
    f32 += 1.0                                              # (a copy: the cache is not touched)
    assert np.array_equal(chain.packed()[0], frames.astype(np.float32))


def test_planar_two_link_chain_matches_its_closed_form():
    l1, l2 = 0.7, 0.45
    chain = KinematicChain([dict(type="revolute", axis=[0, 0, 1]), dict(type="revolute", xyz=[l1, 0, 0], axis=[0, 0, 1]),
                            dict(type="fixed", xyz=[l2, 0, 0])])
    q = np.random.default_rng(3).uniform(-3.0, 3.0, (50, 2))
    want = np.stack([l1 * np.cos(q[:, 0]) + l2 * np.cos(q[:, 0] + q[:, 1]), l1 * np.sin(q[:, 0]) + l2 * np.sin(q[:, 0] + q[:, 1]),
                     np.zeros(50)], 1)
    assert np.abs(chain.forward(q) - want).max() < 1e-14
    f, a = chain.packed(np.float64)
    assert np.abs(R.fk64(q, f, a) - want).max() < 1e-14 and np.abs(R.fk32(q, f, a) - want).max() < 1e-6


URDF = """<?xml version="1.0"?>
<robot name="arm">
  <link name="world"/><link name="a"/><link name="b"/><link name="c"/><link name="side"/>
  <joint name="mount" type="fixed"><origin xyz="0 0 0.5" rpy="0 0 1.0"/><parent link="world"/><child link="a"/></joint>
  <joint name="shoulder" type="revolute"><origin xyz="0.1 0 0" rpy="0.3 0 0"/><axis xyz="0 1 0"/>
    <parent link="a"/><child link="b"/><limit lower="-1.5" upper="2.0" effort="1" velocity="1"/></joint>
  <joint name="branch" type="fixed"><origin xyz="9 9 9"/><parent link="a"/><child link="side"/></joint>
  <joint name="elbow" type="continuous"><origin xyz="0 0 0.4"/><parent link="b"/><child link="c"/></joint>
</robot>"""


def test_from_urdf_walks_from_the_tip(tmp_path):
    want = KinematicChain([dict(type="fixed", xyz=[0, 0, 0.5], rpy=[0, 0, 1.0]),
                           dict(type="revolute", xyz=[0.1, 0, 0], rpy=[0.3, 0, 0], axis=[0, 1, 0]),
                           dict(type="revolute", xyz=[0, 0, 0.4], axis=[1, 0, 0])])
    path = tmp_path / "arm.urdf"
    path.write_text(URDF)
    q = np.random.default_rng(4).uniform(-2, 2, (6, 2))
    for chain in (KinematicChain.from_urdf(str(path), "world", "c"), KinematicChain.from_urdf(URDF, "world", "c")):
        assert [j["name"] for j in chain.joints] == ["mount", "shoulder", "elbow"] and chain.n_dof == 2
        assert (chain.joints[1]["lower"], chain.joints[1]["upper"]) == (-1.5, 2.0) and chain.limits is None
        assert np.array_equal(chain.forward(q), want.forward(q))
    sub = KinematicChain.from_urdf(URDF, "a", "c")
    assert [j["name"] for j in sub.joints] == ["shoulder", "elbow"]
    with pytest.raises(ValueError, match="no joint chain"):
        KinematicChain.from_urdf(URDF, "side", "c")


def test_chain_and_canvas_argument_errors():
    rev = dict(type="revolute", axis=[0, 0, 1])
    for bad in ([], [dict(type="fixed")], [rev] * 17, [dict(type="prismatic")], [dict(type="revolute", axis=[0, 0, 2])],
                [dict(type="revolute", axis=[0, 0])], [dict(rev, xyz=[0, np.nan, 0])], [dict(rev, rpy=[0, 0])], ["revolute"]):
        with pytest.raises(ValueError):
            KinematicChain(bad)
    assert KinematicChain([rev] * 16).n_dof == 16
    with pytest.raises(ValueError, match="q must be"):
        KinematicChain([rev]).forward(np.zeros((3, 2)))
    for kw in (dict(scale=0.0), dict(half_width=0.0), dict(half_width=-1.0), dict(half_width=np.inf), dict(size=0), dict(size=65),
               dict(size=2.5), dict(supersample=3), dict(supersample=16), dict(margin=-0.1), dict(margin=np.nan),
               dict(plane=np.zeros((2, 3))), dict(plane=np.full((3, 3), np.nan)), dict(supersample=True)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            StrokeCanvas(**kw)
    c = StrokeCanvas()
    assert (c.size, c.supersample, c.n_pixels) == (28, 4, 784) and c.half_width == 0.0625
    assert np.allclose(c.plane, [[0, -1 / 0.03, 0], [1 / 0.03, 0, 0], [0, 0, 1]])
    assert StrokeCanvas(size=64, supersample=8, margin=0.0).n_pixels == 4096


# ------------------------------------------------------------------------------------------------ the rasteriser's definition
def _draw(uv, r=R.HALF_WIDTH, margin=R.MARGIN, H=28, ss=4, plane=None, f=R.render64):
    plane = R.default_plane() if plane is None else plane
    rng = np.random.default_rng(0)
    return f(R.lift(np.asarray(uv, dtype=np.float64), plane, rng)[None], plane, r, margin, H, ss)


def test_a_dot_is_a_centred_disc():
    out = _draw([[0.3, -0.2]])
    img = out["image"][0].reshape(28, 28)
    assert abs(out["window"][0, 2] - 3.2 * R.HALF_WIDTH) < 1e-12               # W = (1 + margin) * 2 r
    assert np.abs(img - img[::-1]).max() < 1e-9 and np.abs(img - img[:, ::-1]).max() < 1e-9 and np.abs(img - img.T).max() < 1e-9
    assert img[13:15, 13:15].min() == 1.0 and img[0].max() == 0.0 and img[:, 0].max() == 0.0
    assert abs(img.sum() - np.pi * (28 / 3.2) ** 2) < 1.0                      # the disc's area in pixels


def test_a_horizontal_line_sets_the_window_and_sits_in_the_middle_rows():
    r = R.HALF_WIDTH
    out = _draw(np.stack([np.linspace(-1.0, 1.0, 9), np.zeros(9)], 1))
    L = 2.0 + 2 * r
    assert abs(out["window"][0, 2] - 1.6 * L) < 1e-9 and np.abs(out["window"][0, :2]).max() < 1e-9
    img = out["image"][0].reshape(28, 28)
    rows = np.nonzero(img.sum(1) > 0)[0]
    pitch = 1.6 * L / 28
    assert rows.min() >= 13 - np.ceil(r / pitch) and rows.max() <= 14 + np.ceil(r / pitch) and 13 in rows and 14 in rows
    assert np.abs(img - img[::-1]).max() < 1e-9 and np.abs(img - img[:, ::-1]).max() < 1e-9
    assert abs(img.sum() - (2.0 * 2 * r + np.pi * r * r) / pitch ** 2) < 0.25  # a stadium's area in pixels
    cols = np.nonzero(img.sum(0) > 0)[0]
    assert abs((cols.max() - cols.min() + 1) * pitch - L) <= 2 * pitch
    # a zero-length segment is a point, repeated points change nothing
    twice = _draw(np.repeat(np.stack([np.linspace(-1.0, 1.0, 9), np.zeros(9)], 1), 2, axis=0))
    assert np.abs(twice["image"] - out["image"]).max() < 1e-12


def test_translation_and_scaling_with_the_width_leave_the_image_unchanged():
    rng = np.random.default_rng(6)
    uv = R.letter_uv(40, rng)
    base = _draw(uv)
    moved = _draw(uv + np.array([3.0, -7.0]))
    assert np.abs(moved["image"] - base["image"]).max() < 1e-9 and abs(moved["window"][0, 2] - base["window"][0, 2]) < 1e-9
    scaled = _draw(2.5 * uv, r=2.5 * R.HALF_WIDTH)
    assert np.abs(scaled["image"] - base["image"]).max() < 1e-9 and abs(scaled["window"][0, 2] - 2.5 * base["window"][0, 2]) < 1e-9
    turned = R.rotated_plane()
    assert np.abs(_draw(uv, plane=turned)["image"] - base["image"]).max() < 1e-9


def test_supersampled_coverage_against_a_brute_force_raster():
    """ss = 4 against 32 x 32 hard-coverage samples per pixel on six seeded letter-like paths with T = 100.  The issue's trial
    measured at most 0.032 per pixel and 0.047 in L2 on its own six paths; the bounds here are those plus a quarter (other
    paths): 0.040 and 0.059.  Measured on these paths: per pixel 0.012 to 0.021, L2 0.024 to 0.040, of image norms 3.7 to 6.1;
    ss = 1 differs by 0.21 to 0.35 per pixel and has to be worse than ss = 4 on every path."""
    plane = R.default_plane()
    for seed in range(6):
        rng = np.random.default_rng([11, seed])
        path = R.lift(R.letter_uv(100, rng), plane, rng)
        hard = R.hard_raster64(path, plane, R.HALF_WIDTH, R.MARGIN, 28)
        soft = R.render64(path[None], plane, R.HALF_WIDTH, R.MARGIN, 28, 4)["image"][0]
        one = R.render64(path[None], plane, R.HALF_WIDTH, R.MARGIN, 28, 1)["image"][0]
        d = soft - hard
        print("seed %d: per pixel %.4f, L2 %.4f of %.2f; ss = 1: %.3f" % (seed, np.abs(d).max(), np.linalg.norm(d),
                                                                          np.linalg.norm(hard), np.abs(one - hard).max()))
        assert np.abs(d).max() <= 0.040 and np.linalg.norm(d) <= 0.059
        assert np.abs(one - hard).max() > np.abs(d).max()
        assert 25.0 < hard.sum() < 60.0


def test_nonfinite_rows_are_nan_in_the_definition_and_the_restatement():
    plane = R.default_plane().astype(np.float32)
    path = R.batches((7, 5, 4))[0][2].copy()
    path[1, 3, 2] = np.nan
    path[3, 0, 0] = np.inf
    clean = R.batches((7, 5, 4))[0][2]
    tgt, h = np.zeros((5, 25), np.float32), np.zeros(5, np.float32)
    for f in (R.render64, R.render32):
        out, ref = f(path, plane, R.HALF_WIDTH, R.MARGIN, 5, 4, tgt, h), f(clean, plane, R.HALF_WIDTH, R.MARGIN, 5, 4, tgt, h)
        for k in ("image", "window", "img_l2", "height_l2"):
            assert np.isnan(out[k][[1, 3]]).all() and np.array_equal(out[k][[0, 2, 4]], ref[k][[0, 2, 4]])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape", R.FK_SHAPES)
def test_fk_restatement_is_close_to_the_definition(shape):
    c = R.fk_case(shape)
    r64, r32 = R.fk64(c["traj"], c["frames"], c["axes"]), R.fk32(c["traj"], c["frames"], c["axes"])
    assert r32.dtype == np.float32 and r32.shape == shape[:2] + (3,)
    assert 0.0 < R.rel_err(r32, r64) < 2e-6
    lim = c["chain"].limits
    assert (c["traj"] >= lim[:, 0].astype(np.float32)).all() and (c["traj"] <= lim[:, 1].astype(np.float32)).all()
    assert np.abs(c["chain"].forward(c["traj"].astype(np.float64)) - r64).max() < 2e-6      # (the constants' rounding)


@pytest.mark.parametrize("shape", R.RENDER_SHAPES)
def test_render_restatement_is_close_to_the_definition(shape):
    """fp32 coordinates centred on the path's mean: a sample's distance is good to about 1e-6 of the pitch, and so is its coverage"""
    T, H, ss = shape
    rows = []
    for name, plane, path, height, target, r64, r32 in R.render_refs(shape):
        e = R.render_errors(r32, r64)
        rows.append(path.shape[0])
        assert e["image"] < 2e-5 and e["window"] < 1e-5 and e["img_l2"] < 1e-5 and e["height_l2"] < 1e-5, (name, e)
        assert r32["image"].shape == (path.shape[0], H * H) and (r64["image"] >= 0).all() and (r64["image"] <= 1).all()
        assert (r64["image"].sum(1) > 0).all()
        assert np.abs(r64["height_l2"]).max() < 0.1          # the height is the row's own mean: what is left is the relief
    assert sorted(rows) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("shape,wild", [(s, False) for s in R.FK_CLASS_SHAPES] + [(R.FK_WILD, True)])
def test_fk_restatement_is_close_to_the_definition_at_the_class_shapes(shape, wild):
    c = R.fk_case(shape, wild=wild)
    r64, r32 = R.fk64(c["traj"], c["frames"], c["axes"]), R.fk32(c["traj"], c["frames"], c["axes"])
    assert r32.dtype == np.float32 and r32.shape == shape[:2] + (3,)
    assert 0.0 < R.rel_err(r32, r64) < 2e-6
    again = R.fk_case(shape, wild=wild)
    assert np.array_equal(again["traj"], c["traj"]) and np.array_equal(again["frames"], c["frames"])
    lim = c["chain"].limits.astype(np.float32)
    inside = ((c["traj"] >= lim[:, 0]) & (c["traj"] <= lim[:, 1])).all()
    assert inside != wild and (not wild or np.abs(c["traj"]).max() > 3.0 * np.pi)
    if shape[2] > 7:
        assert shape[2] == c["chain"].n_dof and not np.array_equal(c["traj"], R.fk_case(shape, seed=1)["traj"])


def test_the_new_path_families_are_what_they_say_and_seeded():
    for T in (5, 9, 100, 257):
        d, f = R.path_uv("diagonal", T, None), R.path_uv("frame", T, None)
        assert d.shape == f.shape == (T, 2)
        assert np.array_equal(d[:, 0], d[:, 1]) and d[0].tolist() == [-1.0, -1.0] and d[-1].tolist() == [1.0, 1.0]
        assert np.abs(f).max(1).min() == 1.0 and np.abs(f).max() == 1.0            # every point on the square's outline
        assert np.array_equal(f[0], f[-1]) and f[0].tolist() == [-1.0, -1.0]       # traversed once, closed
        step = np.abs(np.diff(f, axis=0)).sum(1)
        assert np.abs(step.sum() - 8.0) < 1e-12 and step.max() <= 8.0 / (T - 1) + 1e-12
    # the frame's ink hugs the window's edge around an empty middle; the diagonal passes the box test everywhere
    out = _draw(R.path_uv("frame", 100, None), r=0.002, margin=0.0, H=16, ss=1)["image"][0].reshape(16, 16)
    assert (out[[0, -1]] > 0).all() and (out[:, [0, -1]] > 0).all() and not out[1:-1, 1:-1].any()
    out = _draw(R.path_uv("diagonal", 100, None), r=0.002, margin=0.0, H=16, ss=1)["image"][0].reshape(16, 16)
    assert (np.diag(out[::-1]) > 0).all() and (out > 0).sum() <= 3 * 16
    for shape in R.RENDER_CLASS_SHAPES:
        a, b = R.class_batches(shape), R.class_batches(shape)
        assert len(a) == 2 and all(np.array_equal(x[2], y[2]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
        assert not np.array_equal(a[0][2], R.class_batches(shape, seed=1)[0][2])
        assert not np.array_equal(a[0][1], a[1][1])                                # the default plane and the rotated one


@pytest.mark.parametrize("shape,params", [(s, p) for s in R.RENDER_CLASS_SHAPES for p in R.class_params(s)])
def test_render_restatement_is_close_to_the_definition_at_the_class_shapes(shape, params):
    """What test_gpu_render.py's class sweep leans on: a non-zero restatement error for every output, and that each case
    exercises what it is for (a sparsely inked row; a second pass of step 5 where the shape and the margin leave room for one)"""
    T, H, ss = shape
    refs = R.class_refs(shape, params)
    worst = dict.fromkeys(("image", "window", "img_l2", "height_l2"), 0.0)
    for name, plane, path, height, target, r64, r32 in refs:
        e = R.render_errors(r32, r64)
        assert e["image"] < 2e-5 and e["window"] < 1e-5 and e["img_l2"] < 1e-5 and e["height_l2"] < 1e-5, (name, e)
        assert r32["image"].shape == (path.shape[0], H * H) and (r64["image"].sum(1) > 0).all()
        worst = {k: max(worst[k], e[k]) for k in worst}
    assert all(v > 0.0 for v in worst.values()), worst
    share, items = R.class_coverage(shape, refs)
    assert share < 0.5 if H > 1 else share == 1.0
    if H * H * ss > R.THREADS and params[1] < 1.0:
        assert items > R.THREADS
    assert R.class_refs(shape, params) is refs                                     # computed once


# ------------------------------------------------------------------------------------------------ errors
def test_marshalling_errors_on_cpu():
    dev = torch.device("cpu")
    chain, canvas, b = KinematicChain(R.fixture_joints()), StrokeCanvas(), MotionBasis()
    t, frames, axes, was_np = V.motion_fk_args(np.zeros((3, 8, 7)), chain, dev)
    assert t.shape == (3, 8, 7) and frames.shape == (8, 3, 4) and axes.shape == (7, 3) and frames.dtype == torch.float32 and was_np
    assert V.motion_fk_args(torch.zeros(3, 8, 7), chain, dev)[3] is False
    for bad in (np.zeros((3, 8, 6)), np.zeros((8, 7)), np.zeros((3, 0, 7)), np.zeros((1, 1025, 7))):
        with pytest.raises(ValueError):
            V.motion_fk_args(bad, chain, dev)
    with pytest.raises(ValueError, match="KinematicChain"):
        V.motion_fk_args(np.zeros((3, 8, 7)), "baxter", dev)

    p, plane, tg, hg, was_np = V.render_args(np.zeros((4, 9, 3)), canvas, np.zeros((4, 784)), np.zeros(4), dev)
    assert p.shape == (4, 9, 3) and plane.shape == (3, 3) and tg.shape == (4, 784) and hg.shape == (4,) and was_np
    p, plane, tg, hg, _ = V.render_args(np.zeros((4, 9, 3)), canvas, np.ones(784), 0.25, dev)
    assert tg.shape == (4, 784) and tg.is_contiguous() and hg.tolist() == [0.25] * 4
    assert V.render_args(np.zeros((4, 9, 3)), canvas, None, None, dev)[2:4] == (None, None)
    for bad in (dict(path=np.zeros((4, 9, 2))), dict(path=np.zeros((9, 3))), dict(path=np.zeros((4, 0, 3))),
                dict(path=np.zeros((1, 1025, 3))), dict(canvas=28), dict(target=np.zeros((4, 783))), dict(target=np.zeros((3, 784))),
                dict(target=np.zeros(783)), dict(height=np.zeros(3)), dict(height=np.zeros((4, 1)))):
        kw = dict(path=np.zeros((4, 9, 3)), canvas=canvas, target=None, height=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.render_args(device=dev, **kw)

    out = V.draw_args(np.zeros((5, 147)), b, chain, canvas, None, np.zeros((5, 784)), None, dev)
    assert out[0].shape == (5, 147) and out[1]["phi"].shape == (100, 21) and out[5].shape == (5, 784) and out[6] is None and out[7]
    for bad in (dict(params=np.zeros((5, 146))), dict(basis="sigmoid"), dict(chain=None), dict(canvas=None),
                dict(chain=KinematicChain(R.fixture_joints(3))), dict(basis=MotionBasis(n_dof=6)),
                dict(target=np.zeros((4, 784))), dict(height=np.zeros(6)), dict(anchor=dict(phases=[0.0], target=np.zeros((4, 7, 1))))):
        kw = dict(params=np.zeros((5, 147)), basis=b, chain=chain, canvas=canvas, anchor=None, target=None, height=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.draw_args(device=dev, **kw)

    assert V.writing_cost_args((0.3, 10.0, 0.7), 0, canvas, (784, 147)) == [0.3, 10.0, 0.7]
    for bad in (dict(weights=(1.0, 2.0)), dict(weights=(1.0, np.nan, 0.0)), dict(weights=0.3), dict(image_modality=1),
                dict(image_modality=2), dict(image_modality=True), dict(canvas=StrokeCanvas(size=27)), dict(canvas="canvas")):
        kw = dict(weights=(0.3, 10.0, 0.7), image_modality=0, canvas=canvas, widths=(784, 147))
        kw.update(bad)
        with pytest.raises(ValueError):
            V.writing_cost_args(**kw)


def test_model_methods_exist_with_the_documented_signatures():
    import inspect
    M = V.AssocVariationalAutoEncoder
    assert list(inspect.signature(M.motion_fk).parameters) == ["self", "trajectories", "chain"]
    assert list(inspect.signature(M.render_strokes).parameters) == ["self", "path", "canvas", "target", "height"]
    assert list(inspect.signature(M.draw_motion).parameters) == ["self", "params", "basis", "chain", "canvas", "anchor", "target",
                                                                 "height"]
    sig = inspect.signature(M.writing_cost)
    assert list(sig.parameters) == ["self", "params", "basis", "chain", "canvas", "target_image", "target_latent", "height", "weights",
                                    "image_modality"]
    assert sig.parameters["weights"].default == (0.3, 10.0, 0.7) and sig.parameters["image_modality"].default == 0
    assert list(inspect.signature(M.cycle_error).parameters) == ["self", "X", "basis", "chain", "canvas", "source", "modality"]
    import vae_assoc_amd
    assert vae_assoc_amd.KinematicChain is KinematicChain and vae_assoc_amd.StrokeCanvas is StrokeCanvas
