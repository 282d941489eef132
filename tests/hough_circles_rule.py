"""The Hough circle rule of include/canny_hip.h restated in numpy: Sobel pair at the set pixels, step
in float32, ray votes, five-way peaks in (votes descending, base ascending) order, radius by support, ordered acceptance.
Shared by tests/test_hough_circles_rule.py (the host-only entry points) and tests/test_gpu_hough_circles.py (every
accumulator cell and every record).  Nothing here calls the library."""
import numpy as np

F32 = np.float32


def sobel(img):
    """The reference's 3x3 pair (calculateXYGradient): gx clamps columns and drops rows outside the frame, gy clamps rows
    and drops columns.  int [H, W] -> (gx, gy) int16."""
    a = np.asarray(img, np.int32)
    h, w = a.shape
    d = a[:, np.r_[1:w, w - 1]] - a[:, np.r_[0, 0:w - 1]]
    gx = 2 * d
    gx[:-1] += d[1:]
    gx[1:] += d[:-1]
    e = a[np.r_[1:h, h - 1]] - a[np.r_[0, 0:h - 1]]
    gy = 2 * e
    gy[:, :-1] += e[:, 1:]
    gy[:, 1:] += e[:, :-1]
    return gx.astype(np.int16), gy.astype(np.int16)


def step(gx, gy):
    """(sx, sy) int32 of s16 gradients: conversion, root and quotient each rounded to float32 once; (0, 0) -> (0, 0)."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    q = (gx * gx + gy * gy).astype(np.uint32)
    m = np.sqrt(q.astype(F32))
    assert m.dtype == F32
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = np.rint((gx * 1024).astype(F32) / m)  # np.rint: half to even
        sy = np.rint((gy * 1024).astype(F32) / m)
    return np.where(q == 0, 0, sx).astype(np.int32), np.where(q == 0, 0, sy).astype(np.int32)


def accumulate(mask, gx, gy, min_radius, max_radius, cell_shift):
    """bool [H, W] and its gradient planes -> int32 accumulator (ah + 2, aw + 2) with its zero border."""
    h, w = mask.shape
    c = 1 << cell_shift
    acc = np.zeros(((h + c - 1) // c + 2, (w + c - 1) // c + 2), np.int32)
    y, x = np.nonzero(mask)
    sx, sy = step(np.asarray(gx)[y, x], np.asarray(gy)[y, x])
    keep = (sx != 0) | (sy != 0)
    y, x, sx, sy = (v[keep].astype(np.int64)[:, None] for v in (y, x, sx, sy))
    k = np.arange(min_radius, max_radius + 1, dtype=np.int64)[None, :]
    for s in (1, -1):
        px, py = (x * 1024 + s * k * sx) >> 10, (y * 1024 + s * k * sy) >> 10  # arithmetic shift: floor
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        np.add.at(acc, ((py[ok] >> cell_shift) + 1, (px[ok] >> cell_shift) + 1), 1)
    return acc


def peaks(acc, threshold):
    """All peaks of one accumulator in candidate order: (bases int64, votes int64)."""
    a = acc.astype(np.int64)
    c = a[1:-1, 1:-1]
    m = (c > threshold) & (c > a[1:-1, :-2]) & (c >= a[1:-1, 2:]) & (c > a[:-2, 1:-1]) & (c >= a[2:, 1:-1])
    ay, ax = np.nonzero(m)
    base, votes = (ay + 1) * acc.shape[1] + ax + 1, c[ay, ax]
    order = np.lexsort((base, -votes))
    return base[order], votes[order]


def circles(mask, acc, min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max):
    """What one frame returns: (records int32 [k, 6] of x2, y2, radius, votes, support, base; true number of peaks)."""
    base, votes = peaks(acc, threshold)
    stride, c, nr = acc.shape[1], 1 << cell_shift, max_radius - min_radius + 1
    y, x = (v.astype(np.int64) for v in np.nonzero(mask))
    out = []
    for b, v in zip(base[:centres_max].tolist(), votes[:centres_max].tolist()):
        x2, y2 = (2 * (b % stride - 1) + 1) * c, (2 * (b // stride - 1) + 1) * c
        d = (2 * x - x2) ** 2 + (2 * y - y2) ** 2
        s = np.floor(np.sqrt(d.astype(np.float64))).astype(np.int64)
        s -= s * s > d
        s += (s + 1) ** 2 <= d
        r = (s + 1) >> 1  # (2r - 1)^2 <= d < (2r + 1)^2
        count = np.bincount(r[(r >= min_radius) & (r <= max_radius)] - min_radius, minlength=nr).tolist()
        best = 0
        for i in range(1, nr):  # count[q] / q > count[r] / r in integers; the smaller radius keeps a tie
            if count[i] * (min_radius + best) > count[best] * (min_radius + i):
                best = i
        if count[best] <= support_threshold:
            continue
        if any((x2 - o[0]) ** 2 + (y2 - o[1]) ** 2 < (2 * min_dist) ** 2 for o in out):
            continue
        out.append((x2, y2, min_radius + best, v, count[best], b))
    return np.array(out, np.int32).reshape(len(out), 6), int(base.size)
