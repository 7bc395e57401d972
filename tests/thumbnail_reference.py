"""The definition of letter thumbnails (avae_letter_thumbnail, include/avae.h) in NumPy int64, and next to it
a second, independent form: the S x S canvas built the way the reference builds it (utils.py:240-254), enlarged ``size`` times
with ``np.kron`` and summed in blocks of S x S.  Both give the exact integer ``sum`` of the definition; the picture is one double
division and one rounding to float32 of it.  tests/test_thumbnail_cpu.py holds the two forms equal; tests/test_gpu_thumbnail.py
compares the kernels with the first one bit by bit."""
import numpy as np

CAMERA = dict(threshold=108, invert=True)
CANVAS = dict(invert=True)


def grey(frames, channel_order="rgb"):
    """uint8 frames [N, Hf, Wf] or [N, Hf, Wf, C] (C = 1, 3, 4) -> grey values int64 [N, Hf, Wf]"""
    f = np.asarray(frames)
    assert f.dtype == np.uint8
    if f.ndim == 3:
        return f.astype(np.int64)
    if f.shape[3] == 1:
        return f[..., 0].astype(np.int64)
    assert f.shape[3] in (3, 4) and channel_order in ("rgb", "bgr")
    c = f.astype(np.int64)
    r, b = (c[..., 0], c[..., 2]) if channel_order == "rgb" else (c[..., 2], c[..., 0])
    return (4899 * r + 9617 * c[..., 1] + 1868 * b + 8192) >> 14


def ink_values(v, threshold=None, invert=False):
    """grey values -> ink values g (int64, 0 .. 255)"""
    if threshold is not None and threshold >= 0:
        v = np.where(v > threshold, 255, 0).astype(np.int64)
    return 255 - v if invert else v


def bounding_box(g):
    """one frame's ink values [Hf, Wf] -> ((x, y, w, h), ink count); a blank frame is the whole frame with count 0"""
    mask = g != 0
    n = int(mask.sum())
    if n == 0:
        return (0, 0, g.shape[1], g.shape[0]), 0
    ys, xs = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    return (int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1)), n


def window_of(box):
    """(x, y, w, h) -> (L, b, S, oy, ox), integer arithmetic"""
    _, _, w, h = box
    L = max(w, h)
    b = (3 * L) // 5
    return L, b, L + b, b // 2 + (L - h) // 2, b // 2 + (L - w) // 2


def weights(j, S, size, k0, k1):
    """wx(j, k) for the canvas cells k0 <= k < k1, int64"""
    k = np.arange(k0, k1, dtype=np.int64)
    return np.maximum(0, np.minimum((j + 1) * S, (k + 1) * size) - np.maximum(j * S, k * size))


def sums_definition(g, box, size):
    """the integer sums [size, size] of the definition: sum_cells g wy wx over the crop (the rest of the canvas is zero)"""
    x, y, w, h = box
    _, _, S, oy, ox = window_of(box)
    crop = g[y:y + h, x:x + w].astype(np.int64)
    cols = np.zeros((size, w), np.int64)
    for i in range(size):
        ra, rb = max(i * S // size - oy, 0), min(-((-(i + 1) * S) // size) - oy, h)
        if rb > ra:
            cols[i] = (weights(i, S, size, ra + oy, rb + oy)[:, None] * crop[ra:rb]).sum(0)
    out = np.zeros((size, size), np.int64)
    for j in range(size):
        ca, cb = max(j * S // size - ox, 0), min(-((-(j + 1) * S) // size) - ox, w)
        if cb > ca:
            out[:, j] = (cols[:, ca:cb] * weights(j, S, size, ca + ox, cb + ox)[None, :]).sum(1)
    return out


def sums_kron(g, box, size):
    """the same sums the other way: the reference's canvas, every cell enlarged to size x size, block sums over S x S"""
    x, y, w, h = box
    L, b, S, _, _ = window_of(box)
    canvas = np.zeros((b + L, b + L), np.int64)
    canvas[(b // 2 + (L - h) // 2):(h + b // 2 + (L - h) // 2), (b // 2 + (L - w) // 2):(w + b // 2 + (L - w) // 2)] = g[y:y + h, x:x + w]
    big = np.kron(canvas, np.ones((size, size), np.int64))
    return big.reshape(size, S, size, S).sum((1, 3))


def picture(sums, S):
    """integer sums -> float32 picture: one division in double, one rounding"""
    return (sums.astype(np.float64) / np.float64(255 * S * S)).astype(np.float32)


def thumbnails(frames, size=28, threshold=None, invert=False, channel_order="rgb", sums=sums_definition):
    """uint8 frames -> dict of image float32 [N, size * size], box int32 [N, 4], window int32 [N, 3], ink int32 [N]"""
    v = grey(frames, channel_order)
    N = v.shape[0]
    out = dict(image=np.zeros((N, size * size), np.float32), box=np.zeros((N, 4), np.int32), window=np.zeros((N, 3), np.int32),
               ink=np.zeros(N, np.int32))
    for n in range(N):
        g = ink_values(v[n], threshold, invert)
        box, count = bounding_box(g)
        _, _, S, oy, ox = window_of(box)
        out["box"][n], out["ink"][n] = box, count
        out["window"][n] = (box[0] - ox, box[1] - oy, S)
        if count:
            out["image"][n] = picture(sums(g, box, size), S).reshape(-1)
    return out


def letter_frame(rng, Hf, Wf, C=1, box=None, background=255, alpha=True):
    """A frame of ``background`` (255: dark ink on white, for the inverting modes; 0: bright ink on black) with random ink inside
    ``box = (x, y, w, h)`` (default: somewhere inside) whose four edges all hold ink; colour frames get the same value in every
    colour channel and a random fourth channel."""
    if box is None:
        w, h = int(rng.integers(1, Wf + 1)), int(rng.integers(1, Hf + 1))
        box = (int(rng.integers(0, Wf - w + 1)), int(rng.integers(0, Hf - h + 1)), w, h)
    x, y, w, h = box
    f = np.full((Hf, Wf), background, np.uint8)
    dark = rng.integers(0, 100, (h, w))
    edge = 0 if background else 255
    patch = np.where(rng.random((h, w)) < 0.4, dark if background else 255 - dark, background).astype(np.uint8)
    patch[0, rng.integers(0, w)] = edge
    patch[-1, rng.integers(0, w)] = edge
    patch[rng.integers(0, h), 0] = edge
    patch[rng.integers(0, h), -1] = edge
    f[y:y + h, x:x + w] = patch
    if C == 1:
        return f
    out = np.repeat(f[:, :, None], C, axis=2)
    if C == 4 and alpha:
        out[:, :, 3] = rng.integers(0, 256, (Hf, Wf))
    return out


def ink_box_restated(buf, base, row_stride, Hf, Wf, C, threshold=None, invert=False, channel_order="rgb"):
    """k_ink_box's address arithmetic restated (csrc/avae_thumbnail.hip), for one frame whose first pixel is byte ``base`` of the
    flat uint8 buffer ``buf``, taken as the address (``base`` mod 16 is the row's residue): whole 16-byte chunks of a row as one
    aligned load, the pixels that start in a chunk taken from a 64-bit funnel of two of its five words, the pixels ahead of the
    first and behind the last whole chunk byte by byte.  Every load is asserted to be aligned and to lie inside a row's ``Wf C``
    bytes, and every pixel to be owned exactly once -> ((x, y, w, h), ink count)."""
    k0, k2 = (1868, 4899) if channel_order == "bgr" else (4899, 1868)
    level = threshold if threshold is not None and threshold >= 0 else (254 if invert else 0)
    nbytes = Wf * C
    inside = np.zeros(len(buf), bool)
    for y in range(Hf):
        inside[base + y * row_stride: base + y * row_stride + nbytes] = True

    def load(addr, n):
        assert addr % n == 0, "a load of %d bytes at residue %d" % (n, addr % n)
        assert 0 <= addr and addr + n <= len(buf) and inside[addr:addr + n].all(), "a load outside the row"
        return int.from_bytes(bytes(buf[addr:addr + n]), "little")

    def grey_of(px):
        if C == 1:
            return px & 255
        return (k0 * (px & 255) + 9617 * ((px >> 8) & 255) + k2 * ((px >> 16) & 255) + 8192) >> 14
    owned, cols, rows = set(), [], []

    def pixel(y, col, px):
        assert 0 <= col < Wf and (y, col) not in owned
        owned.add((y, col))
        if (grey_of(px) > level) != invert:
            cols.append(col)
            rows.append(y)
    for y in range(Hf):
        lo = base + y * row_stride
        lead = (16 - (lo & 15)) & 15
        nfull = (nbytes - lead) >> 4 if nbytes >= lead + 16 else 0
        for ch in range(nfull):
            off = lead + 16 * ch
            q = load(lo + off, 16)
            if C == 1:
                for j in range(16):
                    pixel(y, off + j, (q >> (8 * j)) & 255)
                continue
            rest, w4 = nbytes - (off + 16), 0
            if rest >= 4:
                w4 = load(lo + off + 16, 4)
            else:
                for j in range(3):
                    if j < rest:
                        w4 |= load(lo + off + 16 + j, 1) << (8 * j)
            w = [(q >> (32 * i)) & 0xffffffff for i in range(4)] + [w4]
            first = (C - off % C) % C
            px0 = (off + first) // C
            for k in range(6 if C == 3 else 4):
                b = C * k
                two = w[b >> 2] | (w[(b >> 2) + 1] << 32)
                if b + first < 16:
                    pixel(y, px0 + k, (two >> (8 * ((b & 3) + first))) & 0xffffffff)
        head = (lead + C - 1) // C if nfull else Wf
        tail0 = (lead + 16 * nfull + C - 1) // C if nfull else Wf
        for n in range(head + (Wf - tail0)):
            col = n if n < head else tail0 + (n - head)
            px = 0
            for j in range(min(C, 3)):
                px |= load(lo + col * C + j, 1) << (8 * j)
            pixel(y, col, px)
    assert len(owned) == Hf * Wf
    if not cols:
        return (0, 0, Wf, Hf), 0
    return (min(cols), min(rows), max(cols) - min(cols) + 1, max(rows) - min(rows) + 1), len(cols)
