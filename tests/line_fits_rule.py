"""The line-fit rule of include/canny_hip.h restated in plain Python ints: for every Hough segment
record the total-least-squares line through the sub-pixel edgels of the segment's pixels, the sub-pixel end points on it
and the residuals.  The support comes from the full-plane vote of tests/hough_segments_rule.py (no search window: this is
the definition), the edgels from tests/edgels_rule.py.  Shared by tests/test_line_fits_rule.py (the host-only entry point)
and tests/test_gpu_line_fits.py.  Nothing here calls the library; the tests pass the library's own tables in."""
import math

import numpy as np

import edgels_rule as er
import hough_segments_rule as sr

FIT_INTS = 12
GATE, REFINED_ONLY = 1, 2
MAXD_MASK, DEGENERATE, INVALID = 0x00FFFFFF, 0x10000000, 0x80000000
MAX_AXIS, MAX_RHO = 16384, 8.0
F32 = np.float32


def rdiv(a: int, b: int) -> int:
    """a / b rounded to nearest, halves away from zero; b > 0."""
    q = (2 * abs(a) + b) // (2 * b)
    return q if a >= 0 else -q


def finish(n, Su, Sv, Suu, Suv, Svv, ddx, ddy):
    """Steps 4-6 from the moments: (mu, mv, dx_q30, dy_q30, degenerate).  mu, mv are the centroid relative to the first
    end point in 1/65536 px (0 if n == 0)."""
    mu = rdiv(256 * Su, n) if n else 0
    mv = rdiv(256 * Sv, n) if n else 0
    A, B, C = n * Suu - Su * Su, n * Suv - Su * Sv, n * Svv - Sv * Sv
    s = max(0, max(A, C, abs(B)).bit_length() - 28)
    A, B, C = A >> s, B >> s, C >> s
    D, E = A - C, 2 * B
    h = math.isqrt(D * D + E * E)
    if n < 2 or h == 0:
        return mu, mv, 0, 0, True
    if D >= 0:
        wx, wy = h + D, E
    else:
        wx, wy = abs(E), (h - D) * (1 if E >= 0 else -1)
    if wx * ddx + wy * ddy < 0:
        wx, wy = -wx, -wy
    k = 31 - max(abs(wx), abs(wy)).bit_length()  # >= 1: |w| < 2^30.3
    wx, wy = wx << k, wy << k
    ln = math.isqrt(wx * wx + wy * wy)
    return mu, mv, rdiv(wx << 30, ln), rdiv(wy << 30, ln), False


def u32(v: int) -> int:
    return v & 0xFFFFFFFF


def used_pixels(E, P, rec, n_lines_r, major_x, plane_vote, options):
    """The (u, v) pairs of one valid record: steps 2 and 3."""
    x0, y0, x1, y1 = (int(v) for v in rec[:4])
    ta, tb = (x0, x1) if major_x else (y0, y1)
    sup = np.asarray(E, bool) & (plane_vote == n_lines_r)
    if major_x:
        sup[:, :ta] = False
        sup[:, tb + 1:] = False
    else:
        sup[:ta, :] = False
        sup[tb + 1:, :] = False
    idx = np.flatnonzero(sup.reshape(-1))
    ddx, ddy = x1 - x0, y1 - y0
    out = []
    for xq, yq, w2, w3 in er.edgels_at(P, idx).astype(np.int64):
        w2, w3 = int(w2) & 0xFFFFFFFF, int(w3) & 0xFFFFFFFF
        gx, gy = er._wrap16(w2 & 0xFFFF), er._wrap16(w2 >> 16)
        if options & GATE:
            dot = gx * ddx + gy * ddy
            if (gx == 0 and gy == 0) or 4 * dot * dot > (gx * gx + gy * gy) * (ddx * ddx + ddy * ddy):
                continue
        if options & REFINED_ONLY and not w3 & er.REFINED:
            continue
        out.append((int(xq) - 256 * x0, int(yq) - 256 * y0))
    return out


def fit_of(E, P, bases, numrho, tab_cos, tab_sin, rec, options, planes=None):
    """One record (12 Python ints, each an unsigned 32-bit word) for one segment record of frame (E, P)."""
    E = np.asarray(E)
    height, width = E.shape
    x0, y0, x1, y1, k = (int(v) for v in rec[:5])
    bad = [0] * FIT_INTS
    bad[9] = INVALID
    if not 0 <= k < len(bases):
        return bad
    base = int(bases[k])
    n, r = base // (numrho + 2) - 1, base % (numrho + 2) - 1
    if not (0 <= n < len(tab_cos) and 0 <= r < numrho):
        return bad
    if not (0 <= x0 < width and 0 <= x1 < width and 0 <= y0 < height and 0 <= y1 < height):
        return bad
    major_x = bool(np.abs(F32(tab_sin[n])) >= np.abs(F32(tab_cos[n])))
    if (x0 > x1) if major_x else (y0 > y1):
        return bad
    planes = {} if planes is None else planes
    if n not in planes:
        planes[n] = sr.vote_plane(height, width, tab_cos[n], tab_sin[n], numrho)
    uv = used_pixels(E, P, rec, r, major_x, planes[n], options)
    cnt = len(uv)
    Su, Sv = sum(u for u, _ in uv), sum(v for _, v in uv)
    Suu, Suv, Svv = sum(u * u for u, _ in uv), sum(u * v for u, v in uv), sum(v * v for _, v in uv)
    ddx, ddy = x1 - x0, y1 - y0
    mu, mv, dx, dy, degenerate = finish(cnt, Su, Sv, Suu, Suv, Svv, ddx, ddy)
    cx, cy = 65536 * x0 + mu, 65536 * y0 + mv
    if degenerate:
        return [u32(v) for v in (65536 * x0, 65536 * y0, 65536 * x1, 65536 * y1, cx, cy, 0, 0, cnt, DEGENERATE, 0, 0)]
    Sdd, maxd, pmin, pmax = 0, 0, None, None
    for u, v in uv:
        U, V = 256 * u - mu, 256 * v - mv
        d = (V * dx - U * dy + (1 << 37)) >> 38
        p = (U * dx + V * dy + (1 << 29)) >> 30
        Sdd += d * d
        maxd = max(maxd, abs(d))
        pmin = p if pmin is None else min(pmin, p)
        pmax = p if pmax is None else max(pmax, p)
    along = lambda p, q: (p * q + (1 << 29)) >> 30
    words = (cx + along(pmin, dx), cy + along(pmin, dy), cx + along(pmax, dx), cy + along(pmax, dy), cx, cy, dx, dy, cnt,
             maxd & MAXD_MASK, Sdd & 0xFFFFFFFF, Sdd >> 32)
    return [u32(v) for v in words]


def line_fits(E, P, bases, numrho, tab_cos, tab_sin, segments, options=0) -> np.ndarray:
    """(n, 12) int32 records for the (n, 6) segment records of one frame."""
    seg = np.asarray(segments, np.int64).reshape(-1, sr.SEGMENT_INTS)
    planes = {}
    out = [fit_of(E, P, bases, numrho, tab_cos, tab_sin, rec, options, planes) for rec in seg]
    return np.array(out, np.uint32).view(np.int32).reshape(len(out), FIT_INTS)


def unpack(fits):
    """Floats from (n, 12) int32 records: dict of p0, p1, centre (n, 2 px), direction (n, 2 unit), n, rms and maxd in px,
    degenerate, invalid."""
    f = np.asarray(fits, np.int32).reshape(-1, FIT_INTS)
    w9 = f[:, 9].view(np.uint32)
    n = f[:, 8].astype(np.int64)
    sdd = f[:, 10].view(np.uint32).astype(np.float64) + f[:, 11].view(np.uint32).astype(np.float64) * 4294967296.0
    return {"p0": f[:, 0:2] / 65536.0, "p1": f[:, 2:4] / 65536.0, "centre": f[:, 4:6] / 65536.0,
            "direction": f[:, 6:8] / float(1 << 30), "n": n, "rms": np.sqrt(sdd / np.maximum(n, 1)) / 256.0,
            "maxd": (w9 & MAXD_MASK) / 256.0, "degenerate": (w9 & DEGENERATE) != 0, "invalid": (w9 & INVALID) != 0}


# ---- frames and the whole pipeline, for both test files -------------------------------------------------------------------
_PHI = np.vectorize(lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))))


def soft(inside):
    """round(40 + 180 Phi(d / 1.0)) for a plane of signed distances d (positive inside a shape): a blurred step edge."""
    return np.round(40.0 + 180.0 * _PHI(inside)).astype(np.uint8)


def halfplane(height, width, theta_deg, dist):
    """Signed distance x cos(theta) + y sin(theta) - dist of every pixel."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    t = math.radians(theta_deg)
    return xx * math.cos(t) + yy * math.sin(t) - dist


def drawn_frame(height, width, kind):
    """A uint8 frame whose Canny map holds straight blurred edges: kind 0 a bright axis-parallel box, 1 a slanted band, 2 a
    bright cross (two bars that cross at right angles), 3 a triangle with slanted sides, anything else flat (an empty map)."""
    H = lambda th, d: halfplane(height, width, th, d)
    flat = np.full((height, width), -50.0)
    if kind == 0:
        d = np.minimum.reduce([H(0, width * 0.12), -H(0, width * 0.8), H(90, height * 0.2), -H(90, height * 0.75)])
    elif kind == 1:
        c = width * 0.5 * math.cos(math.radians(23)) + height * 0.5 * math.sin(math.radians(23))
        d = np.minimum(H(23, c - min(height, width) * 0.15), -H(23, c + min(height, width) * 0.15))
    elif kind == 2:
        d = np.maximum(np.minimum(H(90, height * 0.5 - 4.2), -H(90, height * 0.5 + 4.2)),
                       np.minimum(H(0, width * 0.4 - 5.3), -H(0, width * 0.4 + 5.3)))
    elif kind == 3:
        d = np.minimum.reduce([H(60, width * 0.25), -H(120, -width * 0.2 + height * 0.1), -H(90, height * 0.85)])
    else:
        d = flat
    return soft(d)


def pipeline(mask, P, numrho, tab_cos, tab_sin, rho, theta, threshold, lines_max, min_length, max_gap, exclusive, options):
    """(bases, true line count, segments [k, 6], fits [k, 12]) of one frame by the three rules."""
    import hough_rule as hr
    mask = np.asarray(mask, bool)
    acc = hr.accumulate(np.flatnonzero(mask.reshape(-1)), mask.shape[1], numrho, tab_cos, tab_sin)
    _, _, bases, count = hr.lines(acc, threshold, lines_max, rho, theta)
    seg = sr.segments(mask, bases, numrho, tab_cos, tab_sin, min_length, max_gap, exclusive)
    return bases, count, seg, line_fits(mask, P, bases, numrho, tab_cos, tab_sin, seg, options)


# ---- the finishing arithmetic on moment sets -------------------------------------------------------------------------------
def finish_words(m):
    """What the arithmetic hooks return for one set (n, Su, Sv, Suu, Suv, Svv, ddx, ddy): six signed 32-bit ints."""
    mu, mv, dx, dy, degenerate = finish(*(int(v) for v in m))
    wrap = lambda v: ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    return [wrap(mu), wrap(mv), dx, dy, int(m[0]), wrap(DEGENERATE) if degenerate else 0]


def moments_of(points, ddx=1, ddy=0):
    """The set of a list of (u, v) pairs."""
    return [len(points), sum(u for u, _ in points), sum(v for _, v in points), sum(u * u for u, _ in points),
            sum(u * v for u, v in points), sum(v * v for _, v in points), ddx, ddy]


def abc_set(A, B, C, ddx=1, ddy=0):
    """A set with n = 2 whose step-4 values are exactly (A, B, C), A, C >= -1: Su, Sv in {0, 1} give every parity."""
    su, sv = A & 1, C & 1
    if (B + su * sv) & 1:  # B = 2 Suv - Su Sv
        raise ValueError("B + Su * Sv must be even")
    return [2, su, sv, (A + su) // 2, (B + su * sv) // 2, (C + sv) // 2, ddx, ddy]


def designed_moments():
    """The designed sets of both arithmetic tests (a list of 8-int lists), each within the rule's limits."""
    out = []
    big, n = (1 << 22) + 128, 1 << 18
    for U, V in ((big, big), (big, -big), (-big, 3), (5, big), (big, 0), (0, big)):
        # n / 2 points at (U, V) and n / 2 at (-U, -V), then the same moved to one side: the largest sums there are
        out.append([n, 0, 0, n * U * U, n * U * V, n * V * V, 1, 1])
        out.append([n, 0, 0, n * U * U, n * U * V, n * V * V, -1, -1])
        half = [(U, V)] * 3 + [(U - (U > 0) + (U < 0), V - 7 * (V > 0))] * 3
        out.append(moments_of(half, 3, -2))
    out.append([n, n * big, n * big, n * big * big, n * big * big, n * big * big, 1, 0])  # every point the same: h = 0
    # D^2 + E^2 at perfect squares and one beside them, s = 0: E = 2 B, D = E^2 / 2 -+ 1 -> q^2 +- 1; Pythagorean triples
    for B in (1, 2, 3, 100, 4097, 11584, 11585):
        E = 2 * B
        for D in (E * E // 2 - 1, E * E // 2, E * E // 2 + 1):
            for sign in (1, -1):
                A, C = (D, 0) if sign > 0 else (0, D)
                if (B + (A & 1) * (C & 1)) % 2 == 0:
                    out.append(abc_set(A, B, C))
                    out.append(abc_set(A, -B, C, -1, 1))
    for p, q in ((2, 1), (3, 2), (10001, 5000), (11000, 3001)):
        D, Eh = p * p - q * q, p * q  # E = 2 p q, h = p^2 + q^2 exactly
        for k in (1, 3):
            if max(k * D, k * Eh) < 1 << 28 and (k * Eh) % 2 == 0:
                out.append(abc_set(k * D, k * Eh, 0))
                out.append(abc_set(0, -k * Eh, k * D, 0, 1))
    out.append(abc_set(3 * 89000000, 2 * 89000000, 0))  # 3 : 4 : 5 at the top of s = 0: D^2 + E^2 = 25 k^2 > 2^57
    out.append(abc_set(0, -2 * 89000000, 3 * 89000000, -1, -1))
    for D in (1, 2, (1 << 28) - 1):  # D < 0 with E = 0: w = (0, h - D); and D > 0 with E = 0
        out.append(abc_set(0, 0, D, 0, 1))
        out.append(abc_set(0, 0, D, 0, -1))
        out.append(abc_set(D, 0, 0, -1, 0))
    out.append(abc_set(4, 0, 4))  # D = E = 0: a round blob, degenerate
    out.append([0, 0, 0, 0, 0, 0, 1, 0])
    out.append([1, 77, -5, 77 * 77, -385, 25, 1, 0])
    out.append(moments_of([(3, 4), (3, 4)]))  # two coincident edgels
    out.append(moments_of([(0, 0), (1, 0)], -1, 0))
    out.append(moments_of([(-300, 700), (900, -100), (50, 60)], -1, 1))
    return out


def random_moments(rng, count):
    """`count` sets from random point sets of 2 to 6 points, coordinates up to +-(2^22 + 128) at several scales; (count, 8)
    int64.  With so few points every intermediate of the rule fits in 64 bits, which finish_np relies on."""
    k = rng.integers(2, 7, count)
    scale = rng.choice([1 << 4, 1 << 10, 1 << 16, (1 << 22) + 129], count)
    u = rng.integers(-scale[:, None], scale[:, None], (count, 6))
    v = rng.integers(-scale[:, None], scale[:, None], (count, 6))
    line = rng.random(count) < 0.5  # half of them nearly collinear
    v = np.where(line[:, None], u // 3 + rng.integers(-3, 4, (count, 6)), v)
    live = np.arange(6)[None, :] < k[:, None]
    u, v = np.where(live, u, 0), np.where(live, v, 0)
    m = np.stack([k, u.sum(1), v.sum(1), (u * u).sum(1), (u * v).sum(1), (v * v).sum(1),
                  rng.integers(-300, 301, count), rng.integers(-300, 301, count)], axis=1).astype(np.int64)
    return m


def _isqrt_np(v):
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        r -= r * r > v
    for _ in range(2):
        r += (r + 1) * (r + 1) <= v
    assert np.all(r * r <= v) and np.all((r + 1) * (r + 1) > v)
    return r


def _rdiv_np(a, b):
    q = (2 * np.abs(a) + b) // (2 * b)
    return np.where(a >= 0, q, -q)


def finish_np(m):
    """finish_words for (count, 8) int64 sets whose A, B, C stay below 2^62 (asserted in floats): numpy int64."""
    m = np.asarray(m, np.int64)
    n, su, sv, suu, suv, svv, ddx, ddy = (m[:, i] for i in range(8))
    assert np.all(n >= 2) and np.abs(n.astype(np.float64) * np.maximum(suu, svv)).max() < 2.0 ** 62
    mu, mv = _rdiv_np(256 * su, n), _rdiv_np(256 * sv, n)
    A, B, C = n * suu - su * su, n * suv - su * sv, n * svv - sv * sv
    top = np.maximum(np.maximum(A, C), np.abs(B))
    bl = np.zeros(len(m), np.int64)
    for bit in range(63):
        bl = np.where(top >> bit != 0, bit + 1, bl)
    s = np.maximum(0, bl - 28)
    A, B, C = A >> s, B >> s, C >> s
    D, E = A - C, 2 * B
    h = _isqrt_np(D * D + E * E)
    deg = h == 0
    wx = np.where(D >= 0, h + D, np.abs(E))
    wy = np.where(D >= 0, E, np.where(E >= 0, h - D, -(h - D)))
    flip = wx * ddx + wy * ddy < 0
    wx, wy = np.where(flip, -wx, wx), np.where(flip, -wy, wy)
    top = np.maximum(np.abs(wx), np.abs(wy))
    bl = np.zeros(len(m), np.int64)
    for bit in range(32):
        bl = np.where(top >> bit != 0, bit + 1, bl)
    wx, wy = wx << (31 - bl), wy << (31 - bl)
    ln = np.maximum(_isqrt_np(wx * wx + wy * wy), 1)
    dx, dy = np.where(deg, 0, _rdiv_np(wx << 30, ln)), np.where(deg, 0, _rdiv_np(wy << 30, ln))
    flag = np.where(deg, np.int64(DEGENERATE) - (1 << 32), 0)
    return np.stack([mu, mv, dx, dy, n, flag], axis=1).astype(np.int32)
