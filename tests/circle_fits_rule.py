"""The circle-fit rule of include/canny_hip.h restated in plain Python ints: for every Hough circle
record the least-squares (Kasa) circle through the sub-pixel edgels of the pixels in the record's band, the mean-distance
radius, the residuals and the sector mask, with one optional trimmed refit.  The pixels come from the bin rule of
tests/hough_circles_rule.py widened by `band`, the edgels from tests/edgels_rule.py.  Shared by
tests/test_circle_fits_rule.py (the host-only entry points) and tests/test_gpu_circle_fits.py.  Nothing here calls the
library.  `finish_np` is the numpy int64 restatement of the finishing arithmetic for moment sets small enough for it; the
CPU test pins it against `finish`."""
import math

import numpy as np

import edgels_rule as er

FIT_INTS = 8
GATE, REFINED_ONLY = 1, 2
MAXD_MASK, TRIM_FAILED, DEGENERATE, INVALID = 0x00FFFFFF, 0x08000000, 0x10000000, 0x80000000
MAX_AXIS, MAX_BAND, MAX_RADIUS = 16384, 4, 1024
MOMENT_WORDS = 12  # n, Su, Sv, Sz, Suu, Suv, Svv, Suz low, Suz high, Svz low, Svz high, band
MATRIX_BITS = 31


def rdiv(a: int, b: int) -> int:
    """a / b rounded to nearest, halves away from zero; b > 0."""
    q = (2 * abs(a) + b) // (2 * b)
    return q if a >= 0 else -q


def u32(v: int) -> int:
    return v & 0xFFFFFFFF


def centred(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz):
    """(A, B, C, P, Q) of step 4."""
    return (n * Suu - Su * Su, n * Suv - Su * Sv, n * Svv - Sv * Sv, n * Suz - Su * Sz, n * Svz - Sv * Sz)


def shifted(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz):
    """(s, a, b, c, det) of step 5: the matrix after its shift and its determinant."""
    A, B, C, _, _ = centred(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz)
    s = max(0, max(A, C, abs(B)).bit_length() - MATRIX_BITS)
    a, b, c = A >> s, B >> s, C >> s
    return s, a, b, c, a * c - b * b


def finish(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz, band):
    """Steps 4 and 5 from the moments: (mx, my, degenerate), the move of the centre in 1/65536 px."""
    if n < 3:
        return 0, 0, True
    _, _, _, P, Q = centred(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz)
    s, a, b, c, det = shifted(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz)
    if det <= 0:
        return 0, 0, True
    limit = 65536 * (band + 2)
    e = 7 - s
    Y = det << max(-e, 0)
    out = []
    for num in (P * c - Q * b, Q * a - P * b):
        X = abs(num) << max(e, 0)
        if 2 * X >= Y * (2 * limit + 1):  # the rounded quotient would exceed the limit
            return 0, 0, True
        q = (2 * X + Y) // (2 * Y)
        out.append(q if num >= 0 else -q)
    return out[0], out[1], False


def sector(dx: int, dy: int) -> int:
    """0..15: four quadrants counter-clockwise from +x towards +y, four sectors each; a boundary line belongs to the sector
    that starts at it; (0, 0) -> 0."""
    if dx > 0 and dy >= 0:
        quad, p, q = 0, dx, dy
    elif dx <= 0 and dy > 0:
        quad, p, q = 1, dy, -dx
    elif dx < 0 and dy <= 0:
        quad, p, q = 2, -dx, -dy
    elif dx >= 0 and dy < 0:
        quad, p, q = 3, -dy, dx
    else:
        return 0
    return 4 * quad + (2 * q >= p) + (q >= p) + (q >= 2 * p)


def moments_of(uv, radius):
    R2 = (256 * radius) ** 2
    n = len(uv)
    z = [u * u + v * v - R2 for u, v in uv]
    return (n, sum(u for u, _ in uv), sum(v for _, v in uv), sum(z), sum(u * u for u, _ in uv),
            sum(u * v for u, v in uv), sum(v * v for _, v in uv), sum(u * t for (u, _), t in zip(uv, z)),
            sum(v * t for (_, v), t in zip(uv, z)))


def fit_set(uv, radius, band):
    """Steps 4 to 6 on one used set: None if degenerate, else (mx, my, r_q16, [d_q8])."""
    mx, my, deg = finish(*moments_of(uv, radius), band)
    if deg:
        return None
    rho = [math.isqrt((256 * u - mx) ** 2 + (256 * v - my) ** 2) for u, v in uv]
    r = 65536 * radius + rdiv(sum(p - 65536 * radius for p in rho), len(uv))
    return mx, my, r, [(p - r + 128) >> 8 for p in rho]


def band_pixels(E, rec, band):
    """Step 2: the pixel indices (raster order) of one valid record."""
    E = np.asarray(E)
    x2, y2, radius = (int(v) for v in rec[:3])
    y, x = (v.astype(np.int64) for v in np.nonzero(E))
    d = (2 * x - x2) ** 2 + (2 * y - y2) ** 2
    lo = max(radius - band, 1)
    sel = (d >= (2 * lo - 1) ** 2) & (d < (2 * (radius + band) + 1) ** 2)
    return y[sel] * E.shape[1] + x[sel]


def used_pixels(E, P, rec, band, options):
    """Steps 2 and 3: the (u, v) pairs of one valid record."""
    width = np.asarray(E).shape[1]
    x2, y2 = int(rec[0]), int(rec[1])
    idx = band_pixels(E, rec, band)
    out = []
    for i, (xq, yq, w2, w3) in zip(idx.tolist(), er.edgels_at(P, idx).astype(np.int64).tolist()):
        w2, w3 = w2 & 0xFFFFFFFF, w3 & 0xFFFFFFFF
        if options & GATE:
            gx, gy = er._wrap16(w2 & 0xFFFF), er._wrap16(w2 >> 16)
            wx, wy = 2 * (i % width) - x2, 2 * (i // width) - y2
            dot = gx * wx + gy * wy
            if (gx == 0 and gy == 0) or 4 * dot * dot < 3 * (gx * gx + gy * gy) * (wx * wx + wy * wy):
                continue
        if options & REFINED_ONLY and not w3 & er.REFINED:
            continue
        out.append((xq - 128 * x2, yq - 128 * y2))
    return out


def fit_of(E, P, rec, band, trim_q8, options):
    """One record (8 Python ints, each an unsigned 32-bit word) for one circle record of frame (E, P)."""
    height, width = np.asarray(E).shape
    x2, y2, radius = (int(v) for v in rec[:3])
    if not (1 <= radius <= MAX_RADIUS and 0 <= x2 < 2 * width and 0 <= y2 < 2 * height):
        return [0, 0, 0, 0, INVALID, 0, 0, 0]
    uv = used_pixels(E, P, rec, band, options)
    first = fit_set(uv, radius, band)
    if first is None:
        return [u32(32768 * x2), u32(32768 * y2), 65536 * radius, len(uv), DEGENERATE, 0, 0, 0]
    flags = 0
    mx, my, r, ds = first
    if trim_q8 > 0:
        kept = [p for p, d in zip(uv, ds) if abs(d) <= trim_q8]
        second = fit_set(kept, radius, band)
        if second is None:
            flags = TRIM_FAILED
        else:
            uv, (mx, my, r, ds) = kept, second
    sectors = 0
    for u, v in uv:
        sectors |= 1 << sector(256 * u - mx, 256 * v - my)
    Sdd, maxd = sum(d * d for d in ds), max(abs(d) for d in ds)
    return [u32(32768 * x2 + mx), u32(32768 * y2 + my), u32(r), len(uv), (maxd & MAXD_MASK) | flags, sectors,
            u32(Sdd), u32(Sdd >> 32)]


def fits_of(E, P, recs, band, trim_q8, options) -> np.ndarray:
    """(k, 8) int32 records for (k, 6) circle records of one frame."""
    recs = np.asarray(recs, np.int32).reshape(-1, 6)
    out = [fit_of(E, P, r, band, trim_q8, options) for r in recs]
    return np.array(out, np.uint32).reshape(len(out), FIT_INTS).view(np.int32)


# ---- moment sets as the hooks take them ------------------------------------------------------------------------------------
def pack_moments(sets) -> np.ndarray:
    """[(n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz, band)] of Python ints -> (k, 12) int64: Suz and Svz as two's-complement
    128-bit values, low word first."""
    out = np.zeros((len(sets), MOMENT_WORDS), np.uint64)
    m64 = (1 << 64) - 1
    for i, (n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz, band) in enumerate(sets):
        out[i] = [v & m64 for v in (n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Suz >> 64, Svz, Svz >> 64, band)]
    return out.view(np.int64)


def finish_words(sets) -> np.ndarray:
    """What the hooks return for the sets: (k, 4) int32 of mx, my, n, DEGENERATE or 0."""
    out = []
    for s in sets:
        mx, my, deg = finish(*s)
        out.append([u32(mx), u32(my), u32(s[0]), DEGENERATE if deg else 0])
    return np.array(out, np.uint32).reshape(len(out), 4).view(np.int32)


def finish_np(m) -> np.ndarray:
    """The finishing arithmetic in numpy int64 for (k, 10) SMALL sets: n <= 2^4, |Su|, |Sv| <= 2^11, |Sz| <= 2^15, second
    moments <= 2^17, |Suz|, |Svz| <= 2^22 (asserted).  Then A, C, |B| < 2^22 (so s = 0 and the shift changes nothing),
    det < 2^42, |P|, |Q| < 2^27, the numerators below 2^50, X < 2^57 and Y * (2 * limit + 1) < 2^62: everything fits.  Same
    output as finish_words."""
    m = np.asarray(m, np.int64).reshape(-1, 10)
    n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz, band = (m[:, i] for i in range(10))
    for cols, bound in (((0,), 1 << 4), ((1, 2), 1 << 11), ((3,), 1 << 15), ((4, 5, 6), 1 << 17), ((7, 8), 1 << 22),
                        ((9,), MAX_BAND)):
        assert np.all(np.abs(m[:, cols]) <= bound)
    A, B, C = n * Suu - Su * Su, n * Suv - Su * Sv, n * Svv - Sv * Sv
    P, Q = n * Suz - Su * Sz, n * Svz - Sv * Sz
    det = A * C - B * B
    deg = (n < 3) | (det <= 0)
    limit = 65536 * (band + 2)
    Y = np.where(deg, 1, det)
    res = []
    for num in (P * C - Q * B, Q * A - P * B):
        X = np.abs(num) << 7
        deg |= 2 * X >= Y * (2 * limit + 1)
        q = (2 * X + Y) // (2 * Y)
        res.append(np.where(num >= 0, q, -q))
    out = np.zeros((m.shape[0], 4), np.int64)
    out[:, 0], out[:, 1] = np.where(deg, 0, res[0]), np.where(deg, 0, res[1])
    out[:, 2], out[:, 3] = n, np.where(deg, DEGENERATE, 0)
    return out.astype(np.uint32).view(np.int32)


def unpack(fits):
    """(cx, cy, r as float px, n, maxd px, rms px, sector count, trim_failed, degenerate, invalid) arrays."""
    r = np.asarray(fits, np.int32).reshape(-1, FIT_INTS)
    w4, w5 = r[:, 4].view(np.uint32), r[:, 5].view(np.uint32)
    sdd = r[:, 6].view(np.uint32).astype(np.float64) + r[:, 7].view(np.uint32).astype(np.float64) * 4294967296.0
    n = r[:, 3].astype(np.float64)
    rms = np.sqrt(sdd / np.maximum(n, 1)) / 256.0
    nsec = np.array([bin(int(v) & 0xFFFF).count("1") for v in w5], np.int64)
    return (r[:, 0] / 65536.0, r[:, 1] / 65536.0, r[:, 2] / 65536.0, r[:, 3], (w4 & MAXD_MASK) / 256.0, rms, nsec,
            (w4 & TRIM_FAILED) != 0, (w4 & DEGENERATE) != 0, (w4 & INVALID) != 0)


# ---- frames the tests share ----------------------------------------------------------------------------------------------
def ring(h, w, cx, cy, r, a0=0.0, a1=360.0):
    """bool [h, w]: the pixels within half a pixel of the circle (cx, cy, r), between the angles a0 and a1 (degrees)."""
    yy, xx = np.mgrid[:h, :w]
    d = np.hypot(xx - cx, yy - cy)
    a = np.degrees(np.arctan2(yy - cy, xx - cx)) % 360.0
    return (np.abs(d - r) < 0.5) & ((a - a0) % 360.0 <= (a1 - a0))


def drawn_masks(h, w):
    """{name: bool [h, w]}: rings, arcs, two concentric rings 2 px apart, a ring crossed by a line -- scaled to the frame."""
    s = min(h, w)
    cx, cy = w / 2.0 + 0.25, h / 2.0 - 0.25
    big, small = max(s * 0.4, 1.0), max(s * 0.2, 1.0)
    rings = ring(h, w, cx, cy, big) | ring(h, w, w * 0.25, h * 0.3, small) | ring(h, w, 2.0, cy, small)
    arcs = ring(h, w, cx, cy, big, 20, 130) | ring(h, w, cx, cy, small, 200, 340) | ring(h, w, w - 3.0, h - 3.0, big, 150, 300)
    twin = ring(h, w, cx, cy, big) | ring(h, w, cx, cy, max(big - 2.0, 0.5))
    crossed = ring(h, w, cx, cy, big)
    crossed[int(cy), :] = True
    crossed[:, int(cx)] |= (np.arange(h) % 2 == 0)
    return {"rings": rings, "arcs": arcs, "twin": twin, "crossed": crossed}


def mask_kinds(h, w, seed):
    rng = np.random.default_rng(seed)
    out = {"empty": np.zeros((h, w), bool), "all": np.ones((h, w), bool), "random": rng.random((h, w)) < 0.15}
    out.update(drawn_masks(h, w))
    return out


def disk_plane(h, w, cx, cy, R, soft=1.0, dark=40, step=180):
    """uint8 [h, w]: round(dark + step * Phi((R - |p - c|) / soft)), a blurred bright disk."""
    yy, xx = np.mgrid[:h, :w]
    t = (R - np.hypot(xx - cx, yy - cy)) / soft
    phi = 0.5 * (1.0 + np.vectorize(math.erf)(t / math.sqrt(2.0)))
    return np.rint(dark + step * phi).astype(np.uint8)


def hough_records(E, P, min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max):
    """The circle records (k, 6) int32 of tests/hough_circles_rule.py for the map E with the gradient of plane P."""
    import hough_circles_rule as cr
    gx, gy = cr.sobel(P)
    acc = cr.accumulate(E, gx, gy, min_radius, max_radius, cell_shift)
    return cr.circles(E, acc, min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max)[0]


def designed_moments():
    """Moment sets (n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz, band) at the limits and at the branches of the finishing
    arithmetic."""
    U, Z, N = 128 * 2057 + 128, (1 << 29) + (1 << 28), (1 << 17) - 1  # the largest |u|, a |z| near 2^29.5, the largest n
    h = N // 2
    sets = []
    # the largest n with the points in the four corners of the band's box: a full-size, well-conditioned matrix (s = 39)
    for sz in (1, -1):
        for band in (0, 4):
            sets.append((4 * (N // 4), 0, 0, 0, 4 * (N // 4) * U * U, 0, 4 * (N // 4) * U * U, sz * (N // 4) * U * Z * 2,
                         -sz * (N // 4) * U * Z, band))
    # ... and a right-hand side that runs past the limit: degenerate by the move
    sets.append((2 * h, 0, 0, 0, 2 * h * U * U, 0, 2 * h * U * U, 2 * h * U * Z, 2 * h * U * Z, 0))
    # half the points at (U, U), half at (-U, -U): collinear, determinant 0 at the largest shift
    sets.append((2 * h, 0, 0, 0, 2 * h * U * U, 2 * h * U * U, 2 * h * U * U, h * U * Z, h * U * Z, 2))
    # determinants at and beside 0 without a shift: (A, B, C) = (4, 2, 1), (4, 2, 2), (5, 3, 2), (2, 3, 4)
    for suu, suv, svv in ((4, 2, 1), (4, 2, 2), (5, 3, 2), (2, 3, 4), (1, 0, 0), (0, 0, 1)):
        for suz, svz in ((3, -2), (-7, 5), (0, 0)):
            sets.append((1, 0, 0, 0, suu, suv, svv, suz, svz, 1))  # n = 1: below three points, degenerate whatever else
            sets.append((3, 0, 0, 0, suu, suv, svv, suz, svz, 1))
            sets.append((3, 1, -1, 7, suu + 1, suv, svv + 1, suz, svz, 0))
    # the determinant is a multiple of n: the values beside 0 are +n and -n ((A, B, C) = (2, -1, 2), (2, 5, 11), (3, -5, 7))
    for suz, svz in ((3, -2), (-7, 5)):
        sets += [(3, -2, -2, 1, 2, 1, 2, suz, svz, 1), (3, -2, -2, 1, 2, 3, 5, suz, svz, 1), (4, -1, -1, 1, 1, -1, 2, suz, svz, 1)]
    # n = 0, 1, 2
    sets += [(0, 0, 0, 0, 0, 0, 0, 0, 0, 1), (1, 5, 5, 1, 25, 25, 25, 5, 5, 1), (2, 0, 0, 0, 50, 0, 50, 3, 3, 1)]
    # the move exactly at the limit and one unit beyond: A = C = 3 * 2^20, B = 0, P = k so that 128 * P / A = limit (+ 1)
    for band in range(5):
        limit = 65536 * (band + 2)
        for k in (limit, limit + 1, -limit, -limit - 1):
            sets.append((3, 0, 0, 0, 128 << 10, 0, 128 << 10, k << 10, -(k << 10) + 1, band))
    # halves: 128 * P / A = q + 1/2 exactly, both signs (n = 4, Suu = Svv = 256: 128 * 4 p / 1024 = p / 2)
    for p in (1, -1, 3, -3, 101, -101):
        sets.append((4, 0, 0, 0, 256, 0, 256, p, -p, 0))
    # shifts of 1 and 2 around the 31-bit boundary, negative P and Q
    for e in (30, 31, 32, 33):
        a = (1 << e) - 1
        sets.append((3, 0, 0, 0, a // 3 + 1, -(a // 7), a // 3 + 5, -(a // 11), a // 13, 3))
    return sets


def random_moments(rng, k):
    """(k, 10) int64 SMALL sets for finish_np: 3..16 points with |u|, |v| <= 90 around a circle of radius 60, z taken as
    u^2 + v^2 - 60^2 (the arithmetic does not care where z came from), some sets collinear."""
    out = np.zeros((k, 10), np.int64)
    for i in range(k):
        n = int(rng.integers(3, 17))
        a = rng.random(n) * 2 * np.pi * rng.choice([0.2, 0.5, 1.0])
        r = 60 + rng.normal(0, 1.5, n)
        u = np.clip(np.rint(r * np.cos(a) + rng.integers(-20, 21)), -90, 90).astype(np.int64)
        v = np.clip(np.rint(r * np.sin(a) + rng.integers(-20, 21)), -90, 90).astype(np.int64)
        if i % 50 == 0:
            v = 2 * u // 3  # collinear
        z = np.clip(u * u + v * v - 3600, -2000, 2000)
        out[i] = [n, u.sum(), v.sum(), z.sum(), (u * u).sum(), (u * v).sum(), (v * v).sum(), (u * z).sum(), (v * z).sum(),
                  int(rng.integers(0, 5))]
    return out
