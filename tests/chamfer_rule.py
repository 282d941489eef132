"""The chamfer-matching rule of include/canny_hip.h, restated in numpy and Python ints.  The tests
compare the library's host form and its kernels with this file; test_chamfer_rule.py compares this file with a brute-force
triple loop.  Nothing here calls the library."""
import math

import numpy as np

EDT_NONE = 0x7FFFFFFF
MAX_EXTENT = 255


def dist2_of_mask(mask):
    """Exact squared Euclidean distance to the nearest non-zero pixel of a 2-D mask, int32; EDT_NONE everywhere for an
    empty mask.  Two separable min passes in int64: O(h * w * (h + w)), meant for the test frames."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    if not m.any():
        return np.full((h, w), EDT_NONE, np.int32)
    big = np.int64(1) << 40
    cols = np.arange(w, dtype=np.int64)
    row = np.where(m[:, None, :], (cols[None, :, None] - cols[None, None, :]) ** 2, big).min(axis=2)   # [h, w]
    rows = np.arange(h, dtype=np.int64)
    out = (row[None, :, :] + ((rows[:, None] - rows[None, :]) ** 2)[:, :, None]).min(axis=1)
    return out.astype(np.int32)


def cost_plane(dist2, trunc_q4):
    """min(isqrt(d2 * 256), trunc_q4) per element, int64; d2 is read as unsigned 32-bit."""
    v = (np.asarray(dist2).astype(np.int64) & 0xFFFFFFFF) * 256
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return np.minimum(r, trunc_q4)


def cost_of(d2, trunc_q4):
    return min(math.isqrt(int(d2) * 256), int(trunc_q4))


def scores(dist2, templates, trunc_q4):
    """S[t][y][x] for one frame: int64 [T, h, w]."""
    cost = cost_plane(dist2, trunc_q4)
    h, w = cost.shape
    pad = np.full((h + 2 * MAX_EXTENT, w + 2 * MAX_EXTENT), trunc_q4, np.int64)
    pad[MAX_EXTENT:MAX_EXTENT + h, MAX_EXTENT:MAX_EXTENT + w] = cost
    out = np.zeros((len(templates), h, w), np.int64)
    for t, tpl in enumerate(templates):
        for dx, dy in np.asarray(tpl).reshape(-1, 2).astype(np.int64):
            assert abs(dx) <= MAX_EXTENT and abs(dy) <= MAX_EXTENT
            out[t] += pad[MAX_EXTENT + dy:MAX_EXTENT + dy + h, MAX_EXTENT + dx:MAX_EXTENT + dx + w]
    return out


def candidates(S, templates, max_mean_q4):
    """The candidates of one frame, sorted by (mean_q12, base): int64 [n, 2] of (mean_q12, base)."""
    T, h, w = S.shape
    inf = np.int64(1) << 40
    P = np.full((T, h + 2, w + 2), inf, np.int64)
    P[:, 1:-1, 1:-1] = S
    c = P[:, 1:-1, 1:-1]
    K = np.array([len(np.asarray(t).reshape(-1, 2)) for t in templates], np.int64)[:, None, None]
    ok = (c <= max_mean_q4 * K) & (c < P[:, 1:-1, :-2]) & (c <= P[:, 1:-1, 2:]) & (c < P[:, :-2, 1:-1]) & (c <= P[:, 2:, 1:-1])
    base = np.flatnonzero(ok.ravel()).astype(np.int64)
    mean = (S.ravel()[base] * 256) // np.broadcast_to(K, S.shape).ravel()[base]
    order = np.lexsort((base, mean))
    return np.stack([mean[order], base[order]], axis=1)


def matches(dist2, templates, trunc_q4, max_mean_q4, min_dist, matches_max, S=None):
    """-> (records int32 [k, 6]: x, y, template, score, mean_q12, base; the true number of candidates; S)."""
    if S is None:
        S = scores(dist2, templates, trunc_q4)
    T, h, w = S.shape
    assert T * h * w < 2 ** 31
    cand = candidates(S, templates, max_mean_q4)
    acc = []
    for mean, base in cand[:matches_max]:
        t, r = divmod(int(base), h * w)
        y, x = divmod(r, w)
        if any((x - a[0]) ** 2 + (y - a[1]) ** 2 < min_dist * min_dist for a in acc):
            continue
        acc.append((x, y, t, int(S[t, y, x]), int(mean), int(base)))
    return np.array(acc, np.int32).reshape(-1, 6), len(cand), S


def ring_template(radius):
    """The pixels of the filled disc d^2 <= r^2 that have a 4-neighbour outside it, as (dx, dy) int16 [K, 2], raster order."""
    r = int(radius)
    ys, xs = np.mgrid[-r - 1:r + 2, -r - 1:r + 2]
    inside = xs * xs + ys * ys <= r * r
    edge = inside & ~(np.roll(inside, 1, 0) & np.roll(inside, -1, 0) & np.roll(inside, 1, 1) & np.roll(inside, -1, 1))
    return np.stack([xs[edge], ys[edge]], axis=1).astype(np.int16)
