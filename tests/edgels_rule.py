"""The sub-pixel edgel rule of include/canny_hip.h restated for the tests, twice: `edgel_scalar` in
plain Python ints with math.isqrt, one pixel at a time, and `edgels_at` in numpy int64 over a whole index list.  The
vectorised root is checked against its definition (r * r <= v < (r + 1) * (r + 1)) on every call, so it IS math.isqrt;
tests/test_edgels_rule.py compares the two forms with each other and with the host function."""
import math

import numpy as np

EDGEL_INTS = 4
MAG_MASK, DIR_SHIFT, REFINED, INVALID = 0x00FFFFFF, 24, 0x10000000, 0x80000000
STEPS = ((1, 0), (1, 1), (0, 1), (1, -1))  # (dx, dy) of dir 0..3


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


# ---- plain Python ints ------------------------------------------------------------------------------------------------
def sobel_pair_scalar(P, y: int, x: int):
    """The reference's 3x3 pair at one pixel: gx clamps columns and drops rows outside the frame, gy clamps rows and drops
    columns; both wrap through short."""
    h, w = P.shape
    cl, cr = max(x - 1, 0), min(x + 1, w - 1)
    ru, rd = max(y - 1, 0), min(y + 1, h - 1)
    g = lambda r, c: int(P[r, c])
    v = 2 * g(y, cr) - 2 * g(y, cl)
    if y != h - 1:
        v += g(rd, cr) - g(rd, cl)
    if y != 0:
        v += g(ru, cr) - g(ru, cl)
    u = 2 * g(rd, x) - 2 * g(ru, x)
    if x != w - 1:
        u += g(rd, cr) - g(ru, cr)
    if x != 0:
        u += g(rd, cl) - g(ru, cl)
    return _wrap16(v), _wrap16(u)


def mag_q4_scalar(gx: int, gy: int) -> int:
    return math.isqrt(256 * (gx * gx + gy * gy))


def dir_scalar(gx: int, gy: int) -> int:
    ax, ay = abs(gx), abs(gy)
    t22, y15 = ax * 13573, ay << 15
    t67 = t22 + (ax << 16)
    if gx == 0 and gy == 0:
        return 0
    if y15 < t22:
        return 0
    if y15 > t67:
        return 2
    return 1 if (gx < 0) == (gy < 0) else 3


def offset_scalar(a: int, b: int, c: int):
    """(t_q8, refined) from the three magnitudes alone (frame and gradient conditions are the caller's)."""
    dn = 2 * b - a - c
    if not (b >= a and b >= c and dn > 0):
        return 0, 0
    t = (256 * abs(c - a) + dn) // (2 * dn)
    return (t if c >= a else -t), 1


def edgel_scalar(P, index: int):
    """One record (4 Python ints, words 2 and 3 unsigned) for pixel index r * width + c of plane P."""
    h, w = P.shape
    if index >= h * w:
        return (0, 0, 0, INVALID)
    y, x = divmod(int(index), w)
    gx, gy = sobel_pair_scalar(P, y, x)
    b = mag_q4_scalar(gx, gy)
    d = dir_scalar(gx, gy)
    dx, dy = STEPS[d]
    t, refined = 0, 0
    if (gx or gy) and 0 <= x - dx and x + dx < w and 0 <= y - dy < h and 0 <= y + dy < h:
        a = mag_q4_scalar(*sobel_pair_scalar(P, y - dy, x - dx))
        c = mag_q4_scalar(*sobel_pair_scalar(P, y + dy, x + dx))
        t, refined = offset_scalar(a, b, c)
    return (256 * x + t * dx, 256 * y + t * dy, (gx & 0xFFFF) | (gy & 0xFFFF) << 16, b | d << DIR_SHIFT | refined * REFINED)


# ---- numpy, over index lists --------------------------------------------------------------------------------------------
def isqrt64(v):
    """floor(sqrt(v)) for non-negative int64 below 2^52, exact (asserted)."""
    v = np.asarray(v, np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert np.all(r * r <= v) and np.all((r + 1) * (r + 1) > v)
    return r


def mag_q4(gx, gy):
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    return isqrt64(256 * (gx * gx + gy * gy))


def direction(gx, gy):
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    ax, ay = np.abs(gx), np.abs(gy)
    t22, y15 = ax * 13573, ay << 15
    t67 = t22 + (ax << 16)
    d = np.where((gx < 0) == (gy < 0), 1, 3)
    d = np.where(y15 > t67, 2, d)
    d = np.where(y15 < t22, 0, d)
    return np.where((gx == 0) & (gy == 0), 0, d).astype(np.int64)


def offsets(a, b, c):
    """(t_q8, refined) arrays from magnitude triples."""
    a, b, c = (np.asarray(v, np.int64) for v in (a, b, c))
    dn = 2 * b - a - c
    ok = (b >= a) & (b >= c) & (dn > 0)
    safe = np.where(ok, dn, 1)
    t = (256 * np.abs(c - a) + safe) // (2 * safe)
    return np.where(ok, np.where(c >= a, t, -t), 0), ok.astype(np.int64)


def sobel_pairs(P, y, x):
    """The reference's pair at pixel arrays (y, x) of plane P (all inside the frame), int64."""
    P = np.asarray(P).astype(np.int64)
    h, w = P.shape
    cl, cr = np.maximum(x - 1, 0), np.minimum(x + 1, w - 1)
    ru, rd = np.maximum(y - 1, 0), np.minimum(y + 1, h - 1)
    v = 2 * P[y, cr] - 2 * P[y, cl]
    v = v + np.where(y != h - 1, P[rd, cr] - P[rd, cl], 0)
    v = v + np.where(y != 0, P[ru, cr] - P[ru, cl], 0)
    u = 2 * P[rd, x] - 2 * P[ru, x]
    u = u + np.where(x != w - 1, P[rd, cr] - P[ru, cr], 0)
    u = u + np.where(x != 0, P[rd, cl] - P[ru, cl], 0)
    return _wrap16(v), _wrap16(u)


def edgels_at(P, indices) -> np.ndarray:
    """Records (n, 4) int32 for the pixel indices r * width + c (any unsigned 32-bit values) of plane P (u8 or s16)."""
    P = np.asarray(P)
    h, w = P.shape
    idx = np.asarray(indices).astype(np.int64) & 0xFFFFFFFF
    out = np.zeros((idx.size, EDGEL_INTS), np.int64)
    bad = idx >= h * w
    out[bad, 3] = INVALID
    good = np.flatnonzero(~bad)
    if good.size:
        y, x = idx[good] // w, idx[good] % w
        gx, gy = sobel_pairs(P, y, x)
        b = mag_q4(gx, gy)
        d = direction(gx, gy)
        steps = np.array(STEPS, np.int64)
        dx, dy = steps[d, 0], steps[d, 1]
        xa, ya, xc, yc = x - dx, y - dy, x + dx, y + dy
        inside = (xa >= 0) & (xc < w) & (ya >= 0) & (ya < h) & (yc >= 0) & (yc < h) & ((gx != 0) | (gy != 0))
        cl = lambda v, n: np.clip(v, 0, n - 1)
        a = mag_q4(*sobel_pairs(P, cl(ya, h), cl(xa, w)))
        c = mag_q4(*sobel_pairs(P, cl(yc, h), cl(xc, w)))
        t, ok = offsets(a, b, c)
        ok &= inside
        t = np.where(ok, t, 0)
        out[good, 0] = 256 * x + t * dx
        out[good, 1] = 256 * y + t * dy
        out[good, 2] = (gx & 0xFFFF) | (gy & 0xFFFF) << 16
        out[good, 3] = b | d << DIR_SHIFT | ok * REFINED
    return out.astype(np.uint32).view(np.int32).reshape(-1, EDGEL_INTS) if idx.size else np.zeros((0, 4), np.int32)


def edgels_of_map(P, edges) -> np.ndarray:
    """Records of every non-zero pixel of an edge map, in raster order."""
    return edgels_at(P, np.flatnonzero(np.asarray(edges).reshape(-1)))


# ---- unpacking ----------------------------------------------------------------------------------------------------------
def unpack(rec):
    """(x, y as float pixels, gx, gy, mag as float grey levels, dir, refined, invalid) from (n, 4) int32 records."""
    r = np.asarray(rec, np.int32).reshape(-1, EDGEL_INTS)
    w2, w3 = r[:, 2].view(np.uint32), r[:, 3].view(np.uint32)
    gx = (w2 & 0xFFFF).astype(np.uint16).view(np.int16)
    gy = (w2 >> 16).astype(np.uint16).view(np.int16)
    return (r[:, 0] / 256.0, r[:, 1] / 256.0, gx, gy, (w3 & MAG_MASK) / 16.0, (w3 >> DIR_SHIFT) & 3,
            (w3 & REFINED) != 0, (w3 & INVALID) != 0)
