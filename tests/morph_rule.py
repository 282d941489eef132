"""The binary-morphology rule of include/canny_hip.h, restated in numpy on unpacked frames.

Bit maps are uint8 [n_frames, h, ceil(w / 8)], rows MSB-first.  An element is (rows, kw, kh): bit i (LSB = 0) of rows[j] is
the offset (dx, dy) = (i - kw // 2, j - kh // 2).  Nothing here shares code with the library.
"""
import numpy as np

ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT = range(7)
OPS = (ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT)
RECT, CROSS, ELLIPSE = range(3)
BORDER_ZERO, BORDER_ONE, BORDER_NEUTRAL = range(3)
BORDERS = (BORDER_ZERO, BORDER_ONE, BORDER_NEUTRAL)


def element(shape, kw, kh):
    rx, ry = kw // 2, kh // 2
    rows = []
    for j in range(kh):
        m = 0
        for i in range(kw):
            dx, dy = i - rx, j - ry
            if shape == RECT or (shape == ELLIPSE and (rx == 0 or ry == 0)):
                on = True
            elif shape == CROSS:
                on = dx == 0 or dy == 0
            else:
                on = dx * dx * ry * ry + dy * dy * rx * rx <= rx * rx * ry * ry
            m |= int(on) << i
        rows.append(m)
    return rows


def element_array(rows, kw, kh):
    """bool [kh, kw]: a[j, i] = bit i of rows[j] -- the `structure` of scipy.ndimage."""
    return np.array([[(rows[j] >> i) & 1 for i in range(kw)] for j in range(kh)], bool)


def rows_of(array):
    a = np.asarray(array, bool)
    return [int(sum(int(v) << i for i, v in enumerate(r))) for r in a], a.shape[1], a.shape[0]


def reflect(rows, kw, kh):
    return rows_of(element_array(rows, kw, kh)[::-1, ::-1])[0]


def unpack(bits, w):
    """uint8 [..., ceil(w / 8)] -> bool [..., w]; pad bits dropped."""
    return np.unpackbits(np.asarray(bits, np.uint8), axis=-1)[..., :w].astype(bool)


def pack(px):
    """bool [..., w] -> uint8 [..., ceil(w / 8)], pad bits 0."""
    return np.packbits(np.asarray(px, bool), axis=-1)


def primitive(px, rows, kw, kh, erode, outside):
    """One step on bool [n, h, w]: erode: AND over b of in(p + b); dilate: OR over b of in(p - b)."""
    n, h, w = px.shape
    ax, ay = kw // 2, kh // 2
    p = np.full((n, h + 2 * ay, w + 2 * ax), bool(outside))
    p[:, ay:ay + h, ax:ax + w] = px
    out = np.full((n, h, w), bool(erode))
    for j in range(kh):
        for i in range(kw):
            if not (rows[j] >> i) & 1:
                continue
            dx, dy = i - ax, j - ay
            if erode:
                out &= p[:, ay + dy:ay + dy + h, ax + dx:ax + dx + w]
            else:
                out |= p[:, ay - dy:ay - dy + h, ax - dx:ax - dx + w]
    return out


def chain(px, rows, kw, kh, erode, border, iterations):
    outside = (1 if erode else 0) if border == BORDER_NEUTRAL else border
    for _ in range(iterations):
        px = primitive(px, rows, kw, kh, erode, outside)
    return px


def morph_px(px, op, rows, kw, kh, border=BORDER_NEUTRAL, iterations=1):
    px = np.asarray(px, bool)
    e = lambda a: chain(a, rows, kw, kh, True, border, iterations)
    d = lambda a: chain(a, rows, kw, kh, False, border, iterations)
    if op == ERODE:
        return e(px)
    if op == DILATE:
        return d(px)
    if op == OPEN:
        return d(e(px))
    if op == CLOSE:
        return e(d(px))
    if op == GRADIENT:
        return d(px) & ~e(px)
    if op == TOPHAT:
        return px & ~d(e(px))
    if op == BLACKHAT:
        return e(d(px)) & ~px
    raise ValueError(op)


def morph(bits, w, op, rows, kw, kh, border=BORDER_NEUTRAL, iterations=1):
    """bits uint8 [n, h, ceil(w / 8)] -> (out bits, counts int64 [n])."""
    out = morph_px(unpack(bits, w), op, rows, kw, kh, border, iterations)
    return pack(out), out.reshape(out.shape[0], -1).sum(axis=1).astype(np.int64)


# ---- the elements and patterns the CPU and the GPU tests share ------------------------------------------------------------
def named_elements():
    """name -> (rows, kw, kh)"""
    rng = np.random.default_rng(3400)
    el = {
        "1x1": (element(RECT, 1, 1), 1, 1),
        "rect3x3": (element(RECT, 3, 3), 3, 3),
        "rect1x31": (element(RECT, 1, 31), 1, 31),
        "rect31x1": (element(RECT, 31, 1), 31, 1),
        "rect31x31": (element(RECT, 31, 31), 31, 31),
        "rect5x3": (element(RECT, 5, 3), 5, 3),
        "rect3x5": (element(RECT, 3, 5), 3, 5),
        "cross5x5": (element(CROSS, 5, 5), 5, 5),
        "ellipse7x7": (element(ELLIPSE, 7, 7), 7, 7),
        "ellipse15x9": (element(ELLIPSE, 15, 9), 15, 9),
        "L": ([0b00001, 0b00001, 0b00001, 0b00001, 0b11111], 5, 5),
        "far_bit": ([1 << 30] + [0] * 30, 31, 31),  # the single offset (+15, -15)
        "ring3x3": ([0b111, 0b101, 0b111], 3, 3),
        "alternating31": ([0x55555555 & 0x7FFFFFFF], 31, 1),
    }
    for k in range(3):
        a = rng.random((31, 31)) < (0.1, 0.5, 0.9)[k]
        a[rng.integers(31), rng.integers(31)] = True
        el["random31_%d" % k] = rows_of(a)
    return el


RECT_NAMES = ("1x1", "rect3x3", "rect1x31", "rect31x1", "rect31x31", "rect5x3", "rect3x5")


def named_patterns(n, h, w, seed=0):
    """name -> bool [n, h, w] (pad bits are the caller's business)."""
    rng = np.random.default_rng(seed)
    z = np.zeros((n, h, w), bool)
    pats = {"zeros": z.copy(), "ones": ~z}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, w - 1), "bl": (h - 1, 0), "br": (h - 1, w - 1), "centre": (h // 2, w // 2)}.items():
        a = z.copy()
        a[:, y, x] = True
        pats["pixel_" + name] = a
    yy, xx = np.mgrid[0:h, 0:w]
    pats["checker"] = np.broadcast_to(((yy + xx) & 1).astype(bool), (n, h, w)).copy()
    a = z.copy()
    a[:, :, w // 2] = True
    pats["vline"] = a
    a = z.copy()
    a[:, h // 2, :] = True
    pats["hline"] = a
    for d in (0.05, 0.5, 0.95):
        pats["random%.2f" % d] = rng.random((n, h, w)) < d
    return pats


def pack_dirty(px, rng=None):
    """pack(), then every pad bit set (rng None) or random."""
    bits = pack(px)
    w = px.shape[-1]
    if w % 8:
        pad = (0xFF >> (w % 8)) & 0xFF
        if rng is None:
            bits[..., -1] |= pad
        else:
            bits[..., -1] |= rng.integers(0, 256, bits.shape[:-1]).astype(np.uint8) & pad
    return bits
