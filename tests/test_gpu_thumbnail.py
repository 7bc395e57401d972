"""Letter thumbnails (avae_letter_thumbnail, letter_thumbnails / frames_to_motion / occlude_quadrant) on a real MI355X
(include/avae.h) against tests/thumbnail_reference.py.

Every comparison is bitwise against the int64 definition: the arithmetic is exact, no tolerance is involved.  1. frame shapes and
pixel formats; 2. where the box lies and what window it gives; 3. output sizes, strides, modes, blank frames; 4. the plan's slab
counts and the workspace; 5. independence and repetition; 6. the C ABI's errors; 7. the model level.

S = L + (3 L) // 5 takes the values 1, 3, 4, 6, 8, ...: the window classes S < size are tested at S = 1, 3 and 27 (S = 2 belongs to
no L), S = size at L = 18, S a multiple of size at L = 35."""
import ctypes as C

import numpy as np
import pytest
import torch

import thumbnail_reference as R
from conftest import make_arch

pytestmark = pytest.mark.gpu

B = 16
NZ = 20
OUTPUTS = ("image", "box", "window", "ink")
WIDTH = dict(image=None, box=4, window=3, ink=1)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


_MODELS = {}


def _model(V):
    """one small fp32 relu model (the c5_small-sized nets of the other GPU tests), shared by every test here"""
    if "m" not in _MODELS:
        archs = [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]
        _MODELS["m"] = V.AssocVariationalAutoEncoder(archs, binary=[True, False], transfer_fct="relu", weights=[50, 1],
                                                     assoc_lambda=8.0, learning_rate=1e-3, batch_size=B, compute_dtype="fp32",
                                                     device=0, seed=3)
    return _MODELS["m"]


def _stream(model):
    return C.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)


def _err(model):
    return model._L.avae_last_error(model._h).decode()


def _plan(model, rows, Hf, Wf):
    slabs, n = C.c_int32(0), C.c_size_t(0)
    assert model._L.avae_letter_thumbnail_plan(rows, Hf, Wf, C.byref(slabs), C.byref(n)) == 0
    return slabs.value, n.value


GUARD = 64


def _pack(frames, row_pad=0, frame_pad=0, shift=0, fill=0xFF):
    """uint8 frames [N, Hf, Wf, C] -> (flat buffer, offset of the first pixel, row stride, frame stride): rows padded by ``row_pad``
    bytes, frames by ``frame_pad`` more, ``GUARD + shift`` bytes ahead and GUARD behind, every byte that is no pixel ``fill``"""
    N, Hf, Wf, Cn = frames.shape
    rs = Wf * Cn + row_pad
    fs = Hf * rs + frame_pad
    buf = np.full(GUARD + shift + N * fs + GUARD, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[GUARD + shift:], (N, Hf, Wf * Cn), (fs, rs, 1))
    view[...] = frames.reshape(N, Hf, Wf * Cn)
    return buf, GUARD + shift, rs, fs


def _as4(frames):
    f = np.asarray(frames)
    return f[..., None] if f.ndim == 3 else f


def _call(model, frames, size=28, threshold=None, invert=False, order="rgb", want=OUTPUTS, row_pad=0, frame_pad=0, shift=0,
          ws=None, ws_fill=None, ws_extra=0, ws_bytes=None, rc_want=0, **over):
    """avae_letter_thumbnail on packed frames -> dict of the NumPy outputs asked for (``want``), each prefilled with -7.  ``over``
    replaces arguments of the C call by name (rows, Hf, Wf, C, row_stride, frame_stride, flags, frames_ptr, ws_ptr)."""
    f = _as4(frames)
    N, Hf, Wf, Cn = f.shape
    buf, off, rs, fs = _pack(f, row_pad, frame_pad, shift)
    dev = torch.from_numpy(buf).to(model.device)
    a = dict(rows=N, Hf=Hf, Wf=Wf, C=Cn, row_stride=rs, frame_stride=fs, frames_ptr=dev.data_ptr() + off,
             flags=(1 if invert else 0) | (2 if order == "bgr" else 0), threshold=-1 if threshold is None else threshold, size=size)
    a.update(over)
    n_out = max(min(a["rows"], N), 1)
    out = {}
    for k in want:
        if k == "image":
            out[k] = torch.full((n_out, max(a["size"], 1) ** 2), -7.0, device=model.device)
        else:
            out[k] = torch.full((n_out, WIDTH[k]) if k != "ink" else (n_out,), -7, dtype=torch.int32, device=model.device)
    if ws is None:
        need = _plan(model, max(a["rows"], 0), min(max(a["Hf"], 1), 4096), min(max(a["Wf"], 1), 4096))[1] if a["rows"] <= 1 << 24 else 64
        ws = torch.empty(max(need + ws_extra, 16), dtype=torch.uint8, device=model.device)
        if ws_fill is not None:
            ws.fill_(ws_fill)
    nbytes = ws.numel() if ws_bytes is None else ws_bytes
    p = lambda k: None if k not in out else out[k].data_ptr()      # noqa: E731
    rc = model._L.avae_letter_thumbnail(model._h, a["frames_ptr"], a["rows"], a["Hf"], a["Wf"], a["C"], a["row_stride"],
                                        a["frame_stride"], a["flags"], a["threshold"], a["size"], a.get("ws_ptr", ws.data_ptr()),
                                        nbytes, p("image"), p("box"), p("window"), p("ink"), _stream(model))
    torch.cuda.synchronize()
    assert (rc == 0) == (rc_want == 0), (rc, _err(model))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, ref, keys=None):
    for k in keys or got.keys():
        if got[k].shape != ref[k].shape or not np.array_equal(_bits(got[k]), _bits(ref[k])):
            return False
    return True


def _check(model, frames, what, **kw):
    """one call against the definition, bit by bit"""
    ref_kw = {k: kw[k] for k in ("size", "threshold", "invert") if k in kw}
    ref = R.thumbnails(frames, channel_order=kw.get("order", "rgb"), **ref_kw)
    got = _call(model, frames, **kw)
    for k in OUTPUTS:
        bad = np.nonzero(_bits(got[k]).reshape(len(ref[k]), -1) != _bits(ref[k]).reshape(len(ref[k]), -1))
        assert got[k].shape == ref[k].shape and bad[0].size == 0, \
            (what, k, "frame %d, element %d: %r, definition %r" % (bad[0][0], bad[1][0], got[k].reshape(len(ref[k]), -1)[bad[0][0], bad[1][0]],
                                                                   ref[k].reshape(len(ref[k]), -1)[bad[0][0], bad[1][0]]))
    return got, ref


def _letters(seed, N, Hf, Wf, Cn=1, background=255, blank=()):
    rng = np.random.default_rng([seed, N, Hf, Wf, Cn])
    f = np.stack([R.letter_frame(rng, Hf, Wf, Cn, None, background) for _ in range(N)])
    for n in blank:
        f[n] = background
        if Cn == 4:
            f[n, ..., 3] = 77
    return f


def _colours(seed, N, Hf, Wf, Cn):
    """random colours (every channel its own value, random alpha) inside a random box, white elsewhere"""
    rng = np.random.default_rng([seed, N, Hf, Wf, Cn, 5])
    f = np.full((N, Hf, Wf, Cn), 255, np.uint8)
    for n in range(N):
        w, h = int(rng.integers(1, Wf + 1)), int(rng.integers(1, Hf + 1))
        x, y = int(rng.integers(0, Wf - w + 1)), int(rng.integers(0, Hf - h + 1))
        patch = rng.integers(0, 256, (h, w, Cn))
        f[n, y:y + h, x:x + w] = np.where(rng.random((h, w, 1)) < 0.5, patch, 255)
    if Cn == 4:
        f[..., 3] = rng.integers(0, 256, (N, Hf, Wf))
    return f


# ------------------------------------------------------------------------------------------------ 1. shapes and pixel formats
SHAPES = [(1, 1, 1), (3, 3, 5), (5, 28, 28), (2, 37, 53), (65, 16, 16), (2, 120, 160), (1, 7, 300), (1, 300, 7), (1, 480, 640),
          (1, 4096, 4096)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_shapes_against_the_definition(V, shape):
    model = _model(V)
    N, Hf, Wf = shape
    frames = _letters(1, N, Hf, Wf, blank=(N // 2,) if N >= 5 else ())
    if shape == (1, 4096, 4096):
        frames[0, 0, 0] = frames[0, -1, -1] = 0                     # the whole frame is the box: w = 4096, 16 columns per thread
    got, ref = _check(model, frames, shape, **R.CAMERA)
    if N > 1 or Hf * Wf > 1:
        assert ref["ink"].max() > 0
    # the Python call: NumPy in, NumPy out; device tensors in, device tensors out
    if Hf * Wf <= 480 * 640:
        again = model.letter_thumbnails(frames, **model.letter_thumbnails.CAMERA)
        assert isinstance(again["image"], np.ndarray) and _same(again, ref, OUTPUTS)
        dev = model.letter_thumbnails(torch.from_numpy(frames).to(model.device), **R.CAMERA)
        assert all(torch.is_tensor(v) and v.device == model.device for v in dev.values())
        assert _same({k: v.cpu().numpy() for k, v in dev.items()}, ref, OUTPUTS)


@pytest.mark.parametrize("Cn,order", [(1, "rgb"), (3, "rgb"), (3, "bgr"), (4, "rgb"), (4, "bgr")])
def test_pixel_formats(V, Cn, order):
    model = _model(V)
    for (N, Hf, Wf), mode in (((4, 37, 53), R.CANVAS), ((3, 20, 300), R.CAMERA), ((2, 9, 16), dict(threshold=200))):
        frames = _colours(2, N, Hf, Wf, Cn)
        for pad in (0, 1):
            _check(model, frames, (Cn, order, Hf, Wf, pad), order=order, row_pad=pad, shift=pad, **mode)
    if Cn > 1:
        # the two orders differ, and the fourth channel changes nothing
        frames = _colours(3, 2, 12, 12, Cn)
        a, b = (_call(model, frames, order=o, **R.CANVAS)["image"] for o in ("rgb", "bgr"))
        assert not np.array_equal(a, b)
        if Cn == 4:
            other = frames.copy()
            other[..., 3] = 255 - other[..., 3]
            assert _same(_call(model, other, order=order, **R.CANVAS), _call(model, frames, order=order, **R.CANVAS))
        assert _same(model.letter_thumbnails(frames, channel_order=order, **R.CANVAS), R.thumbnails(frames, channel_order=order, **R.CANVAS))


# ------------------------------------------------------------------------------------------------ 2. boxes and windows
def _boxed(boxes, Hf, Wf, Cn, seed=4):
    rng = np.random.default_rng([seed, Hf, Wf, Cn])
    return _as4(np.stack([R.letter_frame(rng, Hf, Wf, Cn, b, 255) for b in boxes]))


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_box_at_every_residue_mod_16(V, Cn):
    """x and x + w at every residue mod 16 (256 frames of 5 x 50 in one call), with dense rows and with rows of Wf C + 1 bytes, so
    that the rows of a frame start at every residue as well"""
    model = _model(V)
    boxes = [(x, 1, 17 + e, 3) for x in range(16) for e in range(16)]
    frames = _boxed(boxes, 5, 50, Cn)
    for pad, shift in ((0, 0), (1, 7)):
        got, ref = _check(model, frames, (Cn, pad), row_pad=pad, shift=shift, **R.CANVAS)
        assert [tuple(b) for b in got["box"]] == boxes


def test_boxes_on_the_frame_edges_and_single_pixels(V):
    model = _model(V)
    Hf, Wf = 21, 45
    boxes = [(0, 5, 9, 7), (36, 5, 9, 7), (11, 0, 9, 7), (11, 14, 9, 7), (0, 0, Wf, Hf), (0, 0, Wf, 1), (0, Hf - 1, Wf, 1),
             (0, 0, 1, Hf), (Wf - 1, 0, 1, Hf)]
    for Cn in (1, 3, 4):
        frames = _boxed(boxes, Hf, Wf, Cn)
        got, _ = _check(model, frames, ("edges", Cn), row_pad=3, **R.CANVAS)
        assert [tuple(b) for b in got["box"]] == boxes
        # one ink pixel in each corner; the last one is the last pixel of the last row: its bytes end the buffer
        single = np.full((4, Hf, Wf, Cn), 255, np.uint8)
        for n, (y, x) in enumerate(((0, 0), (0, Wf - 1), (Hf - 1, 0), (Hf - 1, Wf - 1))):
            single[n, y, x, :min(Cn, 3)] = 0
        got, _ = _check(model, single, ("corners", Cn), **R.CANVAS)
        assert got["ink"].tolist() == [1, 1, 1, 1] and tuple(got["box"][3]) == (Wf - 1, Hf - 1, 1, 1)
        assert (got["window"][:, 2] == 1).all() and np.array_equal(got["image"], np.ones((4, 784), np.float32))
        _check(model, single[3:], ("last byte", Cn), **R.CANVAS)


def test_every_small_box_and_window_class(V):
    """every (w, h) in 1 .. 14 squared (196 frames in one call): L from w and from h, L - h, L - w and b odd and even, S = 1 and 3;
    then S = 27 (L = 17), S = size (L = 18), S = 2 size (L = 35), and w = 255, 256, 257, 4096 (one, one, two and sixteen columns
    per thread)"""
    model = _model(V)
    boxes = [(14 - w, 15 - h, w, h) for w in range(1, 15) for h in range(1, 15)]
    got, _ = _check(model, _boxed(boxes, 16, 15, 1), "small", **R.CANVAS)
    S = got["window"][:, 2]
    assert {1, 3}.issubset(set(S.tolist()))
    for (w, h), s_want in (((17, 5), 27), ((5, 17), 27), ((18, 18), 28), ((18, 2), 28), ((35, 20), 56), ((20, 35), 56)):
        got, _ = _check(model, _boxed([(2, 1, w, h)], 40, 40, 3), (w, h), **R.CANVAS)
        assert got["window"][0, 2] == s_want
    for w in (255, 256, 257, 4096):
        got, _ = _check(model, _boxed([(4096 - w if w < 4096 else 0, 1, w, 3)], 5, 4096, 1), w, **R.CAMERA)
        assert got["box"][0, 2] == w
    got, _ = _check(model, _boxed([(3, 0, 2, 4096)], 4096, 7, 1), "h = 4096", **R.CAMERA)
    assert got["box"][0, 3] == 4096 and got["window"][0, 2] == 4096 + 2457


# ------------------------------------------------------------------------------------------------ 3. sizes, strides, modes, blanks
@pytest.mark.parametrize("size", [1, 2, 27, 28, 29, 64])
def test_output_sizes(V, size):
    model = _model(V)
    _check(model, _letters(5, 4, 37, 53), size, size=size, **R.CANVAS)
    _check(model, _boxed([(1, 1, 1, 1), (0, 0, 2, 2), (3, 2, 17, 9), (0, 0, 40, 35)], 35, 40, 4), size, size=size, **R.CAMERA)
    assert _same(model.letter_thumbnails(_letters(5, 2, 9, 9), size=size), R.thumbnails(_letters(5, 2, 9, 9), size))


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_strides_and_guard_bytes(V, Cn):
    """Rows of Wf C + 1, + 3, + 13 bytes, frames further apart than their rows, the buffer starting at every residue mod 16; every
    byte that is no pixel is 0xFF, which would be ink in this mode (bright ink on black, no threshold, no inversion)"""
    model = _model(V)
    frames = _letters(6, 3, 11, 37, Cn, background=0)
    if Cn == 4:
        frames[..., 3] = 0                                         # (alpha is ignored; a bright alpha must not be ink either)
        frames[1, ..., 3] = 255
    ref = R.thumbnails(frames)
    assert (ref["ink"] > 0).all()
    for row_pad, frame_pad, shift in ((1, 0, 0), (3, 0, 1), (13, 0, 5), (0, 29, 15), (13, 1000, 8), (0, 0, 3)):
        got, _ = _check(model, frames, (Cn, row_pad, frame_pad, shift), row_pad=row_pad, frame_pad=frame_pad, shift=shift)
    # a frame that is all ink up to its last byte, between guards of no ink (inverted: 0xFF is no ink, 0 is)
    full = np.zeros((2, 5, 19, Cn), np.uint8)
    got, _ = _check(model, full, (Cn, "full"), row_pad=3, frame_pad=7, shift=9, **R.CANVAS)
    assert got["ink"].tolist() == [95, 95]
    # the Python call reads a crop of wider device frames in place
    big = torch.from_numpy(_letters(7, 3, 30, 50, Cn, background=0)).to(model.device)
    big = big if Cn > 1 else big[..., None]
    crop = big[:, 4:27, 9:42]
    want = R.thumbnails(crop.cpu().numpy())
    assert _same({k: v.cpu().numpy() for k, v in model.letter_thumbnails(crop).items()}, want, OUTPUTS)


MODES = [(t, i) for t in (None, 0, 108, 254, 255) for i in (False, True)]


@pytest.mark.parametrize("threshold,invert", MODES, ids=["t%s%s" % (t, "i" if i else "") for t, i in MODES])
def test_every_mode(V, threshold, invert):
    model = _model(V)
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (3, 19, 23), dtype=np.uint8)
    frames[1] = rng.integers(100, 117, (19, 23))                   # values around 108, the threshold itself among them
    frames[2] = 108 if threshold is None else threshold             # a frame exactly at the threshold: v > threshold nowhere
    frames[0, :3] = 0
    frames[0, -3:] = 255
    got, ref = _check(model, frames, (threshold, invert), threshold=threshold, invert=invert)
    if threshold is not None:
        assert got["ink"][2] == (19 * 23 if invert else 0)
        assert set(np.unique(got["image"][2]).tolist()) <= {0.0, 1.0} or invert
    colour = _colours(9, 2, 14, 18, 4)
    _check(model, colour, (threshold, invert, "rgba"), threshold=threshold, invert=invert, order="bgr")


def test_blank_frames(V):
    model = _model(V)
    for Cn, mode, bg in ((1, R.CAMERA, 255), (4, R.CANVAS, 255), (3, {}, 0), (1, dict(threshold=200), 7)):
        Hf, Wf = 13, 29
        blank = np.full((1, Hf, Wf, Cn), bg, np.uint8)
        got, _ = _check(model, blank, ("blank alone", Cn), **mode)
        assert got["ink"][0] == 0 and tuple(got["box"][0]) == (0, 0, Wf, Hf) and not got["image"].view(np.uint32).any()
        frames = _letters(10, 5, Hf, Wf, Cn, background=255 if mode.get("invert") else 0)
        frames[[0, 2, 4]] = bg
        if "threshold" in mode and not mode.get("invert"):
            frames[[1, 3]] = np.where(frames[[1, 3]] > 0, 255, bg)
        got, _ = _check(model, frames, ("blank between", Cn), **mode)
        assert got["ink"][[0, 2, 4]].tolist() == [0, 0, 0] and (got["ink"][[1, 3]] > 0).all()
        assert not got["image"][[0, 2, 4]].view(np.uint32).any() and got["image"][[1, 3]].any(axis=1).all()


# ------------------------------------------------------------------------------------------------ 4. slabs and workspace
@pytest.mark.parametrize("Hf", [1, 2, 63, 64, 65, 4096])
def test_every_slab_count(V, Hf):
    """every slab count the plan gives for this Hf (over Wf = 1 .. 4096, the narrowest frame of each count), with ink only in the
    first row, only in the last row, and only in one row of the middle slab: three frames per call"""
    model = _model(V)
    widths = {}
    for Wf in range(1, 4097):
        widths.setdefault(_plan(model, 1, Hf, Wf)[0], Wf)
    assert min(widths) == 1 and max(widths) == -(-Hf // max(-(-Hf // 64), 2))         # (Wf = 4096: bands of two rows at least)
    rng = np.random.default_rng(Hf)
    for slabs, Wf in sorted(widths.items()):
        slab_rows = -(-Hf // slabs)
        rows = (0, Hf - 1, min(Hf - 1, (slabs // 2) * slab_rows + int(rng.integers(0, slab_rows))))
        frames = np.zeros((3, Hf, Wf), np.uint8)
        for n, y in enumerate(rows):
            frames[n, y, rng.integers(0, Wf, 2)] = rng.integers(1, 256, 2)
        got, _ = _check(model, frames, (Hf, Wf, slabs), size=5)
        assert got["box"][:, 1].tolist() == list(rows) and (got["box"][:, 3] == 1).all()


def test_workspace_contents_and_size_do_not_matter(V):
    model = _model(V)
    frames = _letters(11, 3, 130, 90, 3)
    ref = R.thumbnails(frames, **R.CAMERA)
    slabs, need = _plan(model, 3, 130, 90)
    assert slabs == 2 and need == 3 * 2 * 32
    for kw in (dict(ws_fill=0), dict(ws_fill=0xFF), dict(ws_extra=4096, ws_fill=0x5A)):
        assert _same(_call(model, frames, **kw, **R.CAMERA), ref), kw
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=model.device).fill_(0x33)
    other = _letters(12, 7, 300, 40)
    assert _same(_call(model, other, ws=ws, **R.CANVAS), R.thumbnails(other, **R.CANVAS))       # another shape first,
    assert _same(_call(model, frames, ws=ws, **R.CAMERA), ref)                                  # then this one in the same bytes
    # too small, misaligned or missing: refused, nothing written
    for kw, word in ((dict(ws_bytes=need - 1), "workspace_bytes"), (dict(ws_bytes=0), "workspace_bytes"),
                     (dict(ws_ptr=ws.data_ptr() + 4), "16 bytes"), (dict(ws_ptr=None), "workspace_dev")):
        got = _call(model, frames, ws=ws, rc_want=1, **kw, **R.CAMERA)
        assert word in _err(model), (kw, _err(model))
        assert all((v == -7).all() for v in got.values()), kw


# ------------------------------------------------------------------------------------------------ 5. independence and repetition
def test_rows_alone_among_others_on_two_streams_and_again(V):
    model = _model(V)
    frames = _letters(13, 65, 40, 56, 4, blank=(7,))
    ref = R.thumbnails(frames, **R.CANVAS)
    got = _call(model, frames, **R.CANVAS)
    assert _same(got, ref) and _same(_call(model, frames, **R.CANVAS), got)
    for n in (0, 7, 33, 64):
        assert _same(_call(model, frames[n:n + 1], **R.CANVAS), {k: v[n:n + 1] for k, v in got.items()}), n
    assert _same(_call(model, frames[60:], **R.CANVAS), {k: v[60:] for k, v in got.items()})
    side = torch.cuda.Stream(device=model.device)
    with torch.cuda.stream(side):
        assert _same(_call(model, frames, **R.CANVAS), got)
    assert _same(_call(model, frames, **R.CANVAS), got)


def test_every_subset_of_outputs(V):
    """Each of the 15 non-empty subsets of the four outputs gives the bits of the full call.  A NULL pointer is the only way to
    leave an output out, so an output that is not asked for has no buffer whose prefill could be looked at; that a refused call
    leaves prefilled outputs alone is checked where calls are refused (the workspace and C ABI error tests)."""
    model = _model(V)
    frames = _letters(14, 5, 33, 47, 3, blank=(2,))
    full = _call(model, frames, **R.CAMERA)
    assert _same(full, R.thumbnails(frames, **R.CAMERA))
    n = 0
    for mask in range(1, 16):
        want = tuple(k for i, k in enumerate(OUTPUTS) if mask >> i & 1)
        got = _call(model, frames, want=want, **R.CAMERA)
        assert set(got) == set(want) and _same(got, full, want), want
        n += 1
    assert n == 15
    # the C call itself with three NULL outputs
    box = torch.full((5, 4), -7, dtype=torch.int32, device=model.device)
    dev = torch.from_numpy(frames).to(model.device)
    ws = torch.empty(_plan(model, 5, 33, 47)[1], dtype=torch.uint8, device=model.device)
    rc = model._L.avae_letter_thumbnail(model._h, dev.data_ptr(), 5, 33, 47, 3, 47 * 3, 33 * 47 * 3, 1, 108, 28, ws.data_ptr(), ws.numel(),
                                        None, box.data_ptr(), None, None, _stream(model))
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(box.cpu().numpy(), full["box"])


# ------------------------------------------------------------------------------------------------ 6. errors of the C ABI
def test_c_abi_errors_name_the_argument_and_launch_nothing(V):
    model = _model(V)
    frames = _letters(15, 2, 9, 11, 3)
    rs, fs = 33, 9 * 33
    for kw, needle in ((dict(rows=-1), "rows"), (dict(rows=(1 << 24) + 1), "rows"), (dict(Hf=0), "Hf"), (dict(Hf=4097), "Hf"),
                       (dict(Wf=0), "Wf"), (dict(Wf=4097), "Wf"), (dict(C=0), "C = "), (dict(C=2), "C = "), (dict(C=5), "C = "),
                       (dict(size=0), "size"), (dict(size=65), "size"), (dict(threshold=-2), "threshold"), (dict(threshold=256), "threshold"),
                       (dict(flags=4), "flags"), (dict(flags=-1), "flags"), (dict(row_stride=rs - 1), "row_stride"),
                       (dict(row_stride=0), "row_stride"), (dict(row_stride=-rs), "row_stride"), (dict(row_stride=(1 << 26) + 1), "row_stride"), (dict(row_stride=(1 << 62) + 1), "row_stride"),
                       (dict(frame_stride=fs - 1), "frame_stride"), (dict(frame_stride=0), "frame_stride"),
                       (dict(frame_stride=(1 << 38) + 1), "frame_stride"), (dict(frames_ptr=None), "frames_dev"), (dict(want=()), "output")):
        got = _call(model, frames, rc_want=1, **kw)
        msg = _err(model)
        assert msg.startswith("avae_letter_thumbnail: ") and needle in msg, (kw, msg)
        assert all((v == -7).all() for v in got.values()), kw
    # the limits themselves pass; rows == 0 is a no-op that needs no workspace
    assert _same(_call(model, frames, frame_stride=fs, row_stride=rs), R.thumbnails(frames))
    got = _call(model, frames, rows=0, ws_ptr=None, ws_bytes=0)
    assert all((v == -7).all() for v in got.values())
    assert model._L.avae_letter_thumbnail(None, None, 0, 1, 1, 1, 1, 1, 0, -1, 1, None, 0, None, None, None, None, None) == 1


# ------------------------------------------------------------------------------------------------ 7. the model level
def test_python_surface_refuses_bad_frames(V):
    model = _model(V)
    for frames, kw, word in ((np.zeros((1, 4, 4), np.float32), {}, "uint8"), (torch.zeros((1, 4, 4), device=model.device), {}, "uint8"),
                             (np.zeros((1, 4, 4, 2), np.uint8), {}, "channels"), (np.zeros((4, 4), np.uint8), {}, "[N, Hf, Wf]"),
                             (np.zeros((1, 4, 4), np.uint8), dict(size=65), "size"), (np.zeros((1, 4, 4), np.uint8), dict(threshold=300), "threshold")):
        with pytest.raises(ValueError) as e:
            model.letter_thumbnails(frames, **kw)
        assert word in str(e.value)
    empty = model.letter_thumbnails(np.zeros((0, 4, 4), np.uint8))
    assert empty["image"].shape == (0, 784) and empty["box"].shape == (0, 4) and empty["ink"].shape == (0,)


def test_frames_to_motion_is_the_two_calls(V):
    from vae_assoc_amd.motion import MotionBasis
    model = _model(V)
    basis = MotionBasis()
    frames = _letters(16, 5, 60, 80, 4, blank=(1,))
    thumbs = model.letter_thumbnails(frames, **R.CANVAS)
    want = model.predict_motion([thumbs["image"], None], basis)
    got = model.frames_to_motion(frames, basis, **R.CANVAS)
    assert _same(thumbs, R.thumbnails(frames, **R.CANVAS))
    for k in ("mu", "logvar", "trajectory", "saturated_frac"):
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert got["var"] is None and _same({k: got[k] for k in OUTPUTS}, thumbs)
    assert got["trajectory"].shape == (5, basis.n_points, basis.n_dof)
    dev = model.frames_to_motion(torch.from_numpy(frames).to(model.device), basis, **R.CANVAS)
    assert torch.is_tensor(dev["trajectory"]) and np.array_equal(dev["trajectory"].cpu().numpy().view(np.uint32), want["trajectory"].view(np.uint32))
    with pytest.raises(ValueError, match="do not fit"):
        model.frames_to_motion(frames, basis, size=27)
    with pytest.raises(ValueError, match="unknown thumbnail option"):
        model.frames_to_motion(frames, basis, margin=0.5)


def test_occlude_quadrant_drives_complete(V):
    model = _model(V)
    frames = _letters(17, 4, 50, 50)
    image = model.letter_thumbnails(torch.from_numpy(frames).to(model.device), **R.CANVAS)["image"]
    quadrants = np.array([[0, 0], [0, 1], [1, 0], [1, 1]])
    occluded, observed = V.occlude_quadrant(image, quadrants)
    assert torch.is_tensor(occluded) and occluded.device == image.device and observed.dtype == torch.uint8
    obs = observed.cpu().numpy().reshape(4, 28, 28)
    for n, (a, b) in enumerate(quadrants):
        assert obs[n].sum() == 784 - 196 and not obs[n, 14 * a:14 * a + 14, 14 * b:14 * b + 14].any()
    assert bool((occluded == image * observed).all())
    res = model.complete([occluded, None], [observed, None], n_iters=3)
    # the occluded elements are never read: the same result from the full picture under the same mask
    full = model.complete([image, None], [observed, None], n_iters=3)
    assert res["z"].shape == (4, NZ) and res["x"][0].shape == (4, 784) and res["x"][1].shape == (4, 147)
    assert np.array_equal(res["z"].cpu().numpy().view(np.uint32), full["z"].cpu().numpy().view(np.uint32))
    assert bool(torch.isfinite(res["objective"]).all())


def test_rendered_letters_end_to_end(V):
    """render_strokes of four seeded letters at H = 64, quantised to uint8 and placed at (37, 21) of a 120 x 160 frame: the window
    is the placed ink box plus 60 %, in integers, and the picture's ink mass is sum g / (255 S^2) size^2.  Every pixel is one
    float32 rounding (relative error <= 2^-24, the double division's 2^-53 beside it) of a non-negative number, so the sum of the
    pixels in float64 is within 2^-23 of that, relatively."""
    import ik_cases
    from vae_assoc_amd.kinematics import StrokeCanvas
    model = _model(V)
    canvas = StrokeCanvas(size=64)
    path = canvas.lift(ik_cases.letters(4, 100), np.zeros(3)).astype(np.float32)
    drawn = model.render_strokes(path, canvas)["image"].reshape(4, 64, 64)
    q = np.rint(np.clip(drawn, 0.0, 1.0) * 255.0).astype(np.uint8)
    assert (q.reshape(4, -1).max(1) > 0).all()
    frames = np.zeros((4, 120, 160), np.uint8)
    frames[:, 21:85, 37:101] = q
    out = model.letter_thumbnails(torch.from_numpy(frames).to(model.device))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert _same(out, R.thumbnails(frames))
    for n in range(4):
        ys, xs = np.nonzero(q[n].any(1))[0], np.nonzero(q[n].any(0))[0]
        x, y, w, h = 37 + xs[0], 21 + ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1
        L = max(w, h)
        b = 3 * L // 5
        S = L + b
        assert tuple(out["box"][n]) == (x, y, w, h) and out["ink"][n] == np.count_nonzero(q[n])
        assert tuple(out["window"][n]) == (x - b // 2 - (L - w) // 2, y - b // 2 - (L - h) // 2, S)
        mass = float(q[n].astype(np.int64).sum()) * 784.0 / (255.0 * S * S)
        assert abs(float(out["image"][n].astype(np.float64).sum()) - mass) <= 2.0 ** -23 * mass
