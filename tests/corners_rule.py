"""The corner rule of include/canny_hip.h restated for the tests, twice: `corners` in numpy int64
over a whole plane (within the rule's bounds every intermediate stays below 2^63), and `response_scalar` /
`candidate_scalar` in plain Python ints with math.isqrt, one pixel at a time.  tests/test_corners_rule.py compares the two forms with each other
and with the host function."""
import math

import numpy as np

CORNER_WORDS = 4
MIN_EIGEN, HARRIS = 0, 1
MAX_SUM = 49 * 1020 * 1020


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


# ---- plain Python ints ------------------------------------------------------------------------------------------------
def ceil_sqrt(v: int) -> int:
    r = math.isqrt(v)
    return r + (r * r < v)


def response_of(sxx: int, syy: int, sxy: int, mode: int, k_q8: int) -> int:
    sxx, syy, sxy = int(sxx), int(syy), int(sxy)
    if mode == MIN_EIGEN:
        return sxx + syy - ceil_sqrt((sxx - syy) ** 2 + 4 * sxy * sxy)
    return 256 * (sxx * syy - sxy * sxy) - int(k_q8) * (sxx + syy) ** 2


def sobel_pair_scalar(P, y: int, x: int):
    """The reference's 3x3 pair at one pixel: gx clamps columns and drops rows outside the frame, gy clamps rows and drops
    columns."""
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


def response_scalar(P, y: int, x: int, mode: int, block: int, k_q8: int) -> int:
    """R at one pixel, from the plane alone."""
    h, w = P.shape
    r = block // 2
    sxx = syy = sxy = 0
    for v in range(y - r, y + r + 1):
        for u in range(x - r, x + r + 1):
            if 0 <= v < h and 0 <= u < w:
                gx, gy = sobel_pair_scalar(P, v, u)
                sxx, syy, sxy = sxx + gx * gx, syy + gy * gy, sxy + gx * gy
    return response_of(sxx, syy, sxy, mode, k_q8)


def threshold_of(rmax: int, quality_q16: int, min_response: int) -> int:
    return max(max(int(rmax), 0) * int(quality_q16) // 65536, int(min_response), 1)


def candidate_scalar(P, y: int, x: int, mode: int, block: int, k_q8: int, cut: int) -> bool:
    h, w = P.shape
    v = response_scalar(P, y, x, mode, block, k_q8)
    if v < cut:
        return False
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yy, xx = y + dy, x + dx
            if (dy == 0 and dx == 0) or not (0 <= yy < h and 0 <= xx < w):
                continue
            o = response_scalar(P, yy, xx, mode, block, k_q8)
            if (v <= o) if (dy < 0 or (dy == 0 and dx < 0)) else (v < o):
                return False
    return True


# ---- numpy ------------------------------------------------------------------------------------------------------------
def sobel(P):
    """The reference's pair at every pixel of plane P, int64 [H, W] each."""
    P = np.asarray(P).astype(np.int64)
    h, w = P.shape
    y, x = np.mgrid[0:h, 0:w]
    cl, cr = np.maximum(x - 1, 0), np.minimum(x + 1, w - 1)
    ru, rd = np.maximum(y - 1, 0), np.minimum(y + 1, h - 1)
    v = 2 * P[y, cr] - 2 * P[y, cl]
    v = v + np.where(y != h - 1, P[rd, cr] - P[rd, cl], 0)
    v = v + np.where(y != 0, P[ru, cr] - P[ru, cl], 0)
    u = 2 * P[rd, x] - 2 * P[ru, x]
    u = u + np.where(x != w - 1, P[rd, cr] - P[ru, cr], 0)
    u = u + np.where(x != 0, P[rd, cl] - P[ru, cl], 0)
    return _wrap16(v), _wrap16(u)


def box(a, block):
    """Sum over the block x block window centred on every pixel; positions outside the frame contribute 0."""
    r = block // 2
    h, w = a.shape
    p = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    p[r:r + h, r:r + w] = a
    out = np.zeros((h, w), np.int64)
    for dy in range(block):
        for dx in range(block):
            out += p[dy:dy + h, dx:dx + w]
    return out


def isqrt64(v):
    """floor(sqrt(v)) of an int64 array, v < 2^62; checked against its definition."""
    v = np.asarray(v, np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        r = np.where(r * r > v, r - 1, r)
        r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def response_array(sxx, syy, sxy, mode, k_q8):
    """R of int64 tensor arrays within the rule's bounds (every intermediate stays below 2^63)."""
    sxx, syy, sxy = (np.asarray(a, np.int64) for a in (sxx, syy, sxy))
    if mode == MIN_EIGEN:
        D = (sxx - syy) ** 2 + 4 * sxy * sxy
        f = isqrt64(D)
        return sxx + syy - (f + (f * f < D))
    return 256 * (sxx * syy - sxy * sxy) - int(k_q8) * (sxx + syy) ** 2


def response_plane(P, mode, block, k_q8):
    gx, gy = sobel(P)
    return response_array(box(gx * gx, block), box(gy * gy, block), box(gx * gy, block), mode, k_q8)


def candidates(R, cut):
    """Boolean plane of the candidates of a response plane under the threshold `cut`."""
    h, w = R.shape
    low = np.iinfo(np.int64).min
    p = np.full((h + 2, w + 2), low, np.int64)
    p[1:-1, 1:-1] = R
    ok = R >= cut
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            o = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            ok &= (R > o) if (dy < 0 or (dy == 0 and dx < 0)) else (R >= o)
    return ok


def corners(P, mode=MIN_EIGEN, block=3, k_q8=0, quality_q16=655, min_response=0, min_dist=0, corners_max=256, R=None):
    """(records int64 [k, 4]: x, y, response, rank; candidate count; Rmax; R) of one plane."""
    P = np.asarray(P)
    h, w = P.shape
    if R is None:
        R = response_plane(P, mode, block, k_q8)
    rmax = int(R.max())
    cut = threshold_of(rmax, quality_q16, min_response)
    ys, xs = np.nonzero(candidates(R, cut))
    vals = R[ys, xs]
    order = np.lexsort((ys * w + xs, -vals))
    sel = order[:corners_max]
    rec, md2 = [], min_dist * min_dist
    for rank, i in enumerate(sel):
        x, y = int(xs[i]), int(ys[i])
        if any((x - a[0]) ** 2 + (y - a[1]) ** 2 < md2 for a in rec):
            continue
        rec.append((x, y, int(vals[i]), rank))
    return np.array(rec, np.int64).reshape(-1, CORNER_WORDS), len(ys), rmax, R


# ---- designed planes ----------------------------------------------------------------------------------------------------
def blur14641(P):
    """The 1-4-6-4-1 binomial both ways, edges replicated, floor(/256)."""
    a = np.asarray(P).astype(np.int64)
    k = (1, 4, 6, 4, 1)
    p = np.pad(a, ((0, 0), (2, 2)), mode="edge")
    a = sum(k[i] * p[:, i:i + a.shape[1]] for i in range(5))
    p = np.pad(a, ((2, 2), (0, 0)), mode="edge")
    a = sum(k[i] * p[i:i + a.shape[0], :] for i in range(5))
    return (a // 256).astype(np.uint8)


def square_plane():
    """64 x 64, 200 on rows and columns 20..43, blurred: four corners."""
    P = np.zeros((64, 64), np.uint8)
    P[20:44, 20:44] = 200
    return blur14641(P)


def checkerboard_plane():
    """64 x 64 board of 8 x 8 squares of 0 / 200, blurred: 196 candidates in two groups of equal responses."""
    y, x = np.mgrid[0:64, 0:64]
    return blur14641(((((y // 8) + (x // 8)) & 1) * 200).astype(np.uint8))


# ---- the arithmetic test's triples ----------------------------------------------------------------------------------------
def arith_triples(n_random=1 << 20, seed=29):
    """int32 [n, 3] tensors (sxx, syy, sxy) within the rule's bounds: the corners of the domain, triples whose D is a
    perfect square or one beside a perfect square, and n_random random ones."""
    M = MAX_SUM
    t = [(a, b, c) for a in (0, 1, M - 1, M) for b in (0, 1, M - 1, M) for c in (-M, -M + 1, -1, 0, 1, M - 1, M)]
    for m in (1, 2, 3, 1000, 12345, 5000000, M // 4):        # (3m)^2 + (4m)^2 = (5m)^2
        t += [(3 * m + s, s, 2 * m) for s in (0, 7, M - 3 * m)] + [(s, 3 * m + s, -2 * m) for s in (0, 7, M - 3 * m)]
    for b in (0, 1, 2, 3, 77, 5049, 1 << 20, M):             # 1 + 4b^2 = (2b)^2 + 1
        t += [(s + 1, s, b) for s in (0, 5, M - 1)] + [(s, s + 1, -b) for s in (0, 5, M - 1)]
        t += [(s, s, b) for s in (0, 5, M)]                  # 4b^2 = (2b)^2
    for b in (1, 2, 3, 77, 1000, 5048):                      # (2b^2)^2 + 4b^2 = (2b^2 + 1)^2 - 1
        t += [(2 * b * b + s, s, b) for s in (0, 9)] + [(s, 2 * b * b + s, -b) for s in (0, 9)]
    rng = np.random.default_rng(seed)
    r = np.stack([rng.integers(0, M + 1, n_random), rng.integers(0, M + 1, n_random),
                  rng.integers(-M, M + 1, n_random)], axis=1)
    # half of the random ones small, where the root's rounding matters most relative to R
    r[::2] //= rng.integers(1, 1 << 20, (n_random + 1) // 2)[:, None]
    out = np.concatenate([np.array(t, np.int64), r]).astype(np.int32)
    assert (out[:, :2] >= 0).all() and (np.abs(out.astype(np.int64)) <= M).all()
    return out
