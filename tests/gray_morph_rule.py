"""The grey-level morphology and median rule of include/canny_hip.h, restated in numpy.

Planes are uint8 [n_frames, h, w].  An element is the binary morphology's (rows, kw, kh): bit i (LSB = 0) of rows[j] is the
offset (dx, dy) = (i - kw // 2, j - kh // 2).  Written from the formulas of the rule; nothing here shares code with the
library.
"""
import numpy as np

import morph_rule as M

ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT, MEDIAN = range(8)
OPS = (ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT, MEDIAN)
MORPH_OPS = OPS[:7]
BORDER_NEUTRAL, BORDER_REPLICATE, BORDER_CONSTANT = range(3)
BORDERS = (BORDER_NEUTRAL, BORDER_REPLICATE, BORDER_CONSTANT)
ROUTES = (0, 1, 2)


def padded(px, ay, ax, kind, border_mode, border_value):
    """int16 [n, h + 2 ay, w + 2 ax]: the planes with what the outside reads as in a step of `kind` ('erode', 'dilate',
    'median')."""
    px = np.asarray(px, np.uint8).astype(np.int16)
    pad = ((0, 0), (ay, ay), (ax, ax))
    if border_mode == BORDER_REPLICATE:
        return np.pad(px, pad, mode="edge")
    if border_mode == BORDER_CONSTANT:
        value = int(border_value)
    else:
        assert kind != "median", "the median has no neutral border"
        value = 255 if kind == "erode" else 0
    return np.pad(px, pad, mode="constant", constant_values=value)


def primitive(px, rows, kw, kh, erode, border_mode, border_value):
    """One step on uint8 [n, h, w]: erode: min over b of in(p + b); dilate: max over b of in(p - b)."""
    n, h, w = px.shape
    ax, ay = kw // 2, kh // 2
    p = padded(px, ay, ax, "erode" if erode else "dilate", border_mode, border_value)
    out = np.full((n, h, w), 255 if erode else 0, np.int16)
    for j in range(kh):
        for i in range(kw):
            if not (rows[j] >> i) & 1:
                continue
            dx, dy = i - ax, j - ay
            if erode:
                out = np.minimum(out, p[:, ay + dy:ay + dy + h, ax + dx:ax + dx + w])
            else:
                out = np.maximum(out, p[:, ay - dy:ay - dy + h, ax - dx:ax - dx + w])
    return out.astype(np.uint8)


def median_step(px, k, border_mode, border_value):
    """out(p) = the (k^2 - 1) / 2-th smallest of the k x k window."""
    n, h, w = px.shape
    a = k // 2
    p = padded(px, a, a, "median", border_mode, border_value)
    win = np.stack([p[:, j:j + h, i:i + w] for j in range(k) for i in range(k)], axis=-1)
    return np.sort(win, axis=-1)[..., (k * k - 1) // 2].astype(np.uint8)


def chain(px, rows, kw, kh, erode, border_mode, border_value, iterations):
    for _ in range(iterations):
        px = primitive(px, rows, kw, kh, erode, border_mode, border_value)
    return px


def sat_sub(a, b):
    return np.clip(a.astype(np.int16) - b.astype(np.int16), 0, 255).astype(np.uint8)


def gray_morph(px, op, rows, kw, kh, border_mode=BORDER_NEUTRAL, border_value=0, iterations=1):
    """uint8 [n, h, w] -> uint8 [n, h, w]"""
    px = np.asarray(px, np.uint8)
    e = lambda a: chain(a, rows, kw, kh, True, border_mode, border_value, iterations)
    d = lambda a: chain(a, rows, kw, kh, False, border_mode, border_value, iterations)
    if op == ERODE:
        return e(px)
    if op == DILATE:
        return d(px)
    if op == OPEN:
        return d(e(px))
    if op == CLOSE:
        return e(d(px))
    if op == GRADIENT:
        return sat_sub(d(px), e(px))
    if op == TOPHAT:
        return sat_sub(px, d(e(px)))
    if op == BLACKHAT:
        return sat_sub(e(d(px)), px)
    if op == MEDIAN:
        assert kw == kh and kw in (3, 5) and list(rows) == [(1 << kw) - 1] * kh and border_mode != BORDER_NEUTRAL
        for _ in range(iterations):
            px = median_step(px, kw, border_mode, border_value)
        return px
    raise ValueError(op)


# ---- the elements and planes the CPU and the GPU tests share ---------------------------------------------------------------
def named_elements():
    """name -> (rows, kw, kh): the binary morphology's named elements (the asymmetric L, far_bit and random ones among them)
    and the 5 x 5 rectangle of the median."""
    el = dict(M.named_elements())
    el["rect5x5"] = (M.element(M.RECT, 5, 5), 5, 5)
    el["rect15x15"] = (M.element(M.RECT, 15, 15), 15, 15)
    return el


RECT_NAMES = M.RECT_NAMES + ("rect5x5", "rect15x15")
MEDIAN_NAMES = ("rect3x3", "rect5x5")


def named_planes(n, h, w, seed=0):
    """name -> uint8 [n, h, w]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    full = lambda a: np.broadcast_to(np.asarray(a, np.uint8), (n, h, w)).copy()
    planes = {
        "random": rng.integers(0, 256, (n, h, w), dtype=np.uint8),
        "flat0": np.zeros((n, h, w), np.uint8),
        "flat255": np.full((n, h, w), 255, np.uint8),
        "two_valued": (rng.random((n, h, w)) < 0.5).astype(np.uint8) * 255,
        # ties, and the values around 128 and 255: a signed compare or a carry between packed lanes shows here
        "few_valued": np.array([0, 1, 127, 128, 254, 255], np.uint8)[rng.integers(0, 6, (n, h, w))],
        "ramp_x": full((xx * 255) // max(w - 1, 1)),
        "ramp_y": full((yy * 255) // max(h - 1, 1)),
        "ramp_xy": full((xx * 7 + yy * 13) % 256),
        "checker": full(((yy + xx) & 1) * 255),
    }
    bright = np.full((n, h, w), 3, np.uint8)
    bright[:, h // 2, w // 2] = 250
    bright[:, 0, 0] = 200
    dark = np.full((n, h, w), 252, np.uint8)
    dark[:, h // 2, w // 2] = 5
    dark[:, h - 1, w - 1] = 50
    planes["impulse_bright"] = bright
    planes["impulse_dark"] = dark
    return planes


PLANE_NAMES = tuple(named_planes(1, 2, 2))


def blobs_on_ramp(h=96, w=160, seed=39):
    """(plane uint8 [h, w], truth bool [h, w]): dark square blobs of 5..9 pixels on a horizontal brightness ramp, apart from
    each other and from the frame's edge by more than the 15 x 15 element of the chain."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    plane = (40 + (xx * 200) // (w - 1)).astype(np.uint8)
    truth = np.zeros((h, w), bool)
    for cy in range(16, h - 16, 32):
        for cx in range(16, w - 16, 32):
            s = int(rng.integers(5, 10))
            y0, x0 = cy + int(rng.integers(0, 8)), cx + int(rng.integers(0, 8))
            truth[y0:y0 + s, x0:x0 + s] = True
    plane[truth] -= 35                                              # the ramp's lowest value is 40
    return plane, truth
