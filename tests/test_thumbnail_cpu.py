"""CPU checks of letter thumbnails (avae_letter_thumbnail, include/avae.h): the two forms of the definition
in tests/thumbnail_reference.py agree, the integer border rule is the reference's float one, the plan call is host-only and
tiles the frame, the symbols are exported and the Python validators word their errors.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import thumbnail_reference as R


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    return _capi


# (Hf, Wf, box or None): six frame shapes -- L from w and from h, L - h / L - w / b odd and even, a box on every edge, one pixel
SMALL = [(9, 7, None), (12, 20, (3, 2, 11, 4)), (20, 12, (1, 3, 4, 11)), (16, 16, (0, 0, 16, 16)), (5, 5, (4, 4, 1, 1)),
         (13, 31, (2, 5, 27, 8))]


@pytest.mark.parametrize("size", [1, 2, 5, 28])
def test_the_two_forms_agree(size):
    rng = np.random.default_rng(size)
    for Hf, Wf, box in SMALL:
        for C_, mode, order in ((1, R.CANVAS, "rgb"), (3, R.CAMERA, "bgr"), (4, dict(threshold=254), "rgb"), (1, {}, "rgb")):
            bg = 255 if mode.get("invert") else 0
            frames = np.stack([R.letter_frame(rng, Hf, Wf, C_, box, bg), R.letter_frame(rng, Hf, Wf, C_, None, bg)])
            a = R.thumbnails(frames, size, channel_order=order, **mode)
            b = R.thumbnails(frames, size, channel_order=order, sums=R.sums_kron, **mode)
            for k in a:
                assert np.array_equal(a[k].view(np.uint32 if k == "image" else np.int32), b[k].view(np.uint32 if k == "image" else np.int32)), (Hf, Wf, C_, k)
            if box is not None and mode != {}:
                assert tuple(a["box"][0]) == box
            assert a["image"].max() <= 1.0 and a["ink"].min() > 0


def test_definition_by_hand():
    """one 2 x 2 box in a 6 x 8 frame: L = 2, b = 1, S = 3, oy = ox = 0; at size 3 the canvas itself over 255, at size 1 its mean"""
    f = np.zeros((1, 6, 8), np.uint8)
    f[0, 2:4, 5:7] = [[255, 51], [0, 102]]
    out = R.thumbnails(f, 3)
    assert tuple(out["box"][0]) == (5, 2, 2, 2) and tuple(out["window"][0]) == (5, 2, 3) and out["ink"][0] == 3
    want = np.array([[255, 51, 0], [0, 102, 0], [0, 0, 0]], np.float64) / 255.0
    assert np.array_equal(out["image"][0].reshape(3, 3), want.astype(np.float32))
    assert out["image"][0].sum() > 0 and R.thumbnails(f, 1)["image"][0, 0] == np.float32(np.float64(408) / np.float64(255 * 9))
    blank = R.thumbnails(np.zeros((1, 6, 8), np.uint8), 4)
    assert tuple(blank["box"][0]) == (0, 0, 8, 6) and blank["ink"][0] == 0 and not blank["image"].view(np.uint32).any()
    assert tuple(blank["window"][0]) == (-2, -3, 12)


def test_integer_border_is_the_float_one():
    """b = (3 L) // 5 is the reference's int(0.6 * L) (utils.py:241) for every L a frame can give, and far beyond"""
    for L in range(1, 65537):
        assert (3 * L) // 5 == int(0.6 * L), L


def test_grey_formula_keeps_black_white_and_order():
    px = np.array([[[[0, 0, 0, 9], [255, 255, 255, 0], [255, 0, 0, 1], [0, 0, 255, 2]]]], np.uint8)
    assert R.grey(px).tolist() == [[[0, 255, (4899 * 255 + 8192) >> 14, (1868 * 255 + 8192) >> 14]]]
    assert R.grey(px, "bgr")[0, 0, 2] == R.grey(px)[0, 0, 3] and np.array_equal(R.grey(px[..., :3]), R.grey(px))


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_ink_box_addressing_restated(Cn):
    """k_ink_box's chunk, funnel and head / tail arithmetic (thumbnail_reference.ink_box_restated) gives the definition's box and
    count, loads nothing outside a row and owns every pixel once: rows of 1 to 39, 53, 64 and 100 pixels, padded by 0, 1, 3 and 13
    bytes, the buffer at residues 0, 1, 5, 15 and 16, random bytes everywhere (padding included), three modes"""
    rng = np.random.default_rng(Cn)
    for Wf in list(range(1, 40)) + [53, 64, 100]:
        for Hf in (1, 3):
            for pad in (0, 1, 3, 13):
                for base in (0, 1, 5, 15, 16):
                    rs = Wf * Cn + pad
                    buf = rng.integers(0, 256, base + Hf * rs + 40, dtype=np.uint8)
                    frame = np.lib.stride_tricks.as_strided(buf[base:], (Hf, Wf * Cn), (rs, 1)).reshape(1, Hf, Wf, Cn)
                    for thr, inv, order in ((None, False, "rgb"), (108, True, "bgr"), (200, False, "rgb")):
                        g = R.ink_values(R.grey(frame, order)[0], thr, inv)
                        assert R.ink_box_restated(buf, base, rs, Hf, Wf, Cn, thr, inv, order) == R.bounding_box(g), (Wf, Hf, pad, base, thr)


def _plan(L, rows, Hf, Wf):
    slabs, n = C.c_int32(-1), C.c_size_t(0)
    assert L.avae_letter_thumbnail_plan(rows, Hf, Wf, C.byref(slabs), C.byref(n)) == 0, L.avae_last_error(None)
    return slabs.value, n.value


def test_plan_is_host_only_and_tiles_the_frame(capi):
    L = capi.lib()
    for Hf in (1, 2, 63, 64, 65, 480, 4095, 4096):
        for Wf in (1, 2, 16, 127, 128, 129, 640, 4096):
            slabs, n = _plan(L, 3, Hf, Wf)
            assert 1 <= slabs <= 64 and n == 3 * slabs * 32, (Hf, Wf, slabs, n)
            slab_rows = -(-Hf // slabs)
            # the plan's bands [s * slab_rows, min(Hf, (s + 1) * slab_rows)) tile Hf exactly, none empty
            assert (slabs - 1) * slab_rows < Hf <= slabs * slab_rows
            # at most 64 bands, each of at least 8192 pixels where the frame has that many
            assert slabs == -(-Hf // max(-(-Hf // 64), -(-8192 // Wf))), (Hf, Wf, slabs)
    assert _plan(L, 0, 5, 5)[1] == 0
    assert _plan(L, 1, 4096, 4096) == (64, 64 * 32) and _plan(L, 1, 480, 640) == (37, 37 * 32)
    n, slabs = C.c_size_t(0), C.c_int32(0)
    assert L.avae_letter_thumbnail_plan(2, 8, 8, None, C.byref(n)) == 0 and n.value == 64       # NULL outputs are allowed,
    assert L.avae_letter_thumbnail_plan(2, 8, 8, C.byref(slabs), None) == 0 and slabs.value == 1
    assert L.avae_letter_thumbnail_plan(2, 8, 8, None, None) == 2                               # not both
    assert "every output is NULL" in L.avae_last_error(None).decode()
    for bad, word in (((-1, 8, 8), "rows"), (((1 << 24) + 1, 8, 8), "rows"), ((1, 0, 8), "Hf"), ((1, 4097, 8), "Hf"),
                      ((1, 8, 0), "Wf"), ((1, 8, 4097), "Wf")):
        assert L.avae_letter_thumbnail_plan(*bad, C.byref(slabs), C.byref(n)) == 2
        msg = L.avae_last_error(None).decode()
        assert msg.startswith("avae_letter_thumbnail_plan: ") and word in msg, msg


def test_symbols_and_constants(capi):
    assert "avae_letter_thumbnail" in capi.SYMBOLS and "avae_letter_thumbnail_plan" in capi.SYMBOLS
    L = capi.lib()
    assert hasattr(L, "avae_letter_thumbnail") and len(L.avae_letter_thumbnail.argtypes) == 18
    assert (capi.THUMB_MAX_FRAME, capi.THUMB_MAX_SIZE, capi.THUMB_INVERT, capi.THUMB_BGR) == (4096, 64, 1, 2)
    from vae_assoc_amd import vae_assoc as V
    lt = V.AssocVariationalAutoEncoder.letter_thumbnails
    assert lt.CAMERA == dict(threshold=108, invert=True) == R.CAMERA and lt.CANVAS == dict(invert=True) == R.CANVAS


def test_validator_messages():
    from vae_assoc_amd import _args as A
    ok = np.zeros((2, 5, 6), np.uint8)

    def call(frames=ok, size=28, threshold=None, invert=False, channel_order="rgb"):
        return A.letter_thumbnail_args(frames, size, threshold, invert, channel_order, "cpu")
    t, row, frame, flags, thr, size, was_np = call()
    assert tuple(t.shape) == (2, 5, 6, 1) and (row, frame, flags, thr, size, was_np) == (6, 30, 0, -1, 28, True)
    assert call(np.zeros((1, 4, 4, 4), np.uint8), 64, 108, True, "bgr")[3:6] == (3, 108, 64)
    for kw, word in ((dict(frames=ok.astype(np.float32)), "uint8"), (dict(frames=torch.zeros(1, 4, 4)), "float32"),
                     (dict(frames=ok[0]), "[N, Hf, Wf]"), (dict(frames=np.zeros((1, 4, 4, 2), np.uint8)), "1, 3 or 4 channels"),
                     (dict(frames=np.zeros((1, 4097, 1), np.uint8)), "4096"), (dict(frames=np.zeros((1, 0, 4), np.uint8)), "1 to 4096"),
                     (dict(size=0), "size"), (dict(size=65), "size"), (dict(size=28.0), "size"), (dict(threshold=256), "threshold"),
                     (dict(threshold=-1), "threshold"), (dict(threshold=True), "threshold"), (dict(invert=1), "invert"),
                     (dict(channel_order="RGBA"), "channel_order")):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert word in str(e.value), (kw.keys(), str(e.value))


def test_strided_frames_pass_through_without_a_copy():
    from vae_assoc_amd import _marshal as M
    big = torch.zeros((3, 20, 32, 4), dtype=torch.uint8)
    crop = big[:, 2:12, 5:25]                                       # rows padded, frames padded: read in place
    t, row, frame, _ = M.dev_frames(crop, "cpu")
    assert t.data_ptr() == crop.data_ptr() and (row, frame) == (32 * 4, 20 * 32 * 4)
    grey = big[..., 0]                                              # pixel stride 4 with C = 1: copied
    t, row, frame, _ = M.dev_frames(grey, "cpu")
    assert t.data_ptr() != grey.data_ptr() and (row, frame) == (32, 20 * 32) and tuple(t.shape) == (3, 20, 32, 1)
    flipped = big.flip(1)[:, :, :, :3]                              # (a copy already) three of four channels: pixel stride 4 != 3
    assert M.dev_frames(flipped, "cpu")[1:3] == (32 * 3, 20 * 32 * 3)
    one = big[1:2, 3:4]                                             # one frame, one row: their strides do not matter
    assert M.dev_frames(one, "cpu")[1:3] == (32 * 4, 32 * 4)
    overlapping = torch.zeros(64, dtype=torch.uint8).as_strided((2, 3, 8, 1), (8, 4, 1, 1))
    assert M.dev_frames(overlapping, "cpu")[1:3] == (8, 24)         # rows overlap: copied


def test_occlude_quadrant():
    from vae_assoc_amd import occlude_quadrant
    x = np.arange(1, 2 * 16 + 1, dtype=np.float32).reshape(2, 16)
    out, obs = occlude_quadrant(x, (1, 0))
    assert isinstance(out, np.ndarray) and obs.dtype == np.uint8 and obs.shape == (2, 16)
    want = np.ones((4, 4), np.uint8)
    want[2:4, 0:2] = 0                                              # the reference's [14 f0 : 14 (f0 + 1), 14 f1 : 14 (f1 + 1)] at H = 4
    assert np.array_equal(obs[0].reshape(4, 4), want) and np.array_equal(out, x * want.reshape(1, 16))
    out, obs = occlude_quadrant(torch.from_numpy(x), np.array([[0, 0], [1, 1]]))
    assert torch.is_tensor(out) and obs[0].reshape(4, 4)[:2, :2].sum() == 0 and obs[1].reshape(4, 4)[2:, 2:].sum() == 0
    assert int(obs.sum()) == 24 and bool((out[obs == 0] == 0).all()) and bool((out[obs == 1] == torch.from_numpy(x)[obs == 1]).all())
    for bad_x, bad_q, word in ((x[:, :15], (0, 0), "H even"), (x[:, :9], (0, 0), "H even"), (x, (0, 2), "quadrant"), (x, (0,), "quadrant"),
                               (x, (0.0, 1.0), "quadrant"), (x, np.zeros((3, 2), np.int64), "quadrant")):
        with pytest.raises(ValueError) as e:
            occlude_quadrant(bad_x, bad_q)
        assert word in str(e.value)
