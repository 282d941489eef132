"""The shape rule of include/canny_hip.h restated in plain Python, for the tests.

The input is one stored chain P_0 .. P_{n-1}: pixel indices r * width + c, read as (x, y) = (c, r); the chain is closed,
P_n means P_0.  Everything is relative to the anchor P_0: u_i = x_i - x_0, v_i = y_i - y_0.  Every sum is reduced
mod 2^64 and read back as a signed 64-bit word.

  1. polygon moments over the n cyclic steps, a_i = u_i v_{i+1} - u_{i+1} v_i:
       area2 = sum a_i                      m10_6 = sum a_i (u_i + u_{i+1})             m01_6 likewise in v
       m20_12 = sum a_i (u_i^2 + u_i u_{i+1} + u_{i+1}^2)                               m02_12 likewise in v
       m11_24 = sum a_i (2 u_i v_i + u_i v_{i+1} + u_{i+1} v_i + 2 u_{i+1} v_{i+1})
  2. point sums over the n chain points: s10 = sum u, s01 = sum v, s20 = sum u^2, s11 = sum u v, s02 = sum v^2.
  3. the convex hull of the point set: strictly extreme points only, beginning at the smallest x (then the smallest y),
     every turn cross(H_{k+1} - H_k, H_{k+2} - H_{k+1}) > 0; hull_area2 = sum x_k y_{k+1} - x_{k+1} y_k.
  4. the minimum-area rectangle with a side on a hull edge: for edge k, d = H_{k+1} - H_k, len2 = |d|^2,
     along_i = dot(H_i - H_k, d), across_i = cross(d, H_i - H_k), E_k = max along - min along, N_k = max across; the chosen
     edge is the smallest k that minimises E_k N_k / len2_k, compared exactly.  V_h = 1: all zero.
  5. measures, 20 words: hull_vertices, points, anchor, area2, m10_6, m01_6, m20_12, m11_24, m02_12, s10, s01, s20, s11,
     s02, hull_area2, rect_edge, rect_along_min, rect_along_max, rect_across, rect_len2.

shape(chain, width) -> (hull: list of pixel indices, measures: 20 ints)
csr(chain_offsets, points, point_capacity, width)
    -> (hull_offsets u64 [R + 1], hull int32 [total], measures int64 [R, 20]); a record whose chain ends beyond
       point_capacity has no hull vertices and the measures (-1, 0, ..., 0).

Nothing here is shared with the library: Python ints, a sort and the monotone chain."""
import numpy as np

WORDS = 20
(HULL_VERTICES, POINTS, ANCHOR, AREA2, M10_6, M01_6, M20_12, M11_24, M02_12, S10, S01, S20, S11, S02, HULL_AREA2, RECT_EDGE,
 RECT_ALONG_MIN, RECT_ALONG_MAX, RECT_ACROSS, RECT_LEN2) = range(WORDS)


def wrap(v):
    """v mod 2^64, read as a signed word."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def moments(xs, ys):
    """The eleven sums of rules 1 and 2 of the closed chain (xs, ys), in the order of the measures."""
    n = len(xs)
    u, v = [x - xs[0] for x in xs], [y - ys[0] for y in ys]
    area2 = m10 = m01 = m20 = m11 = m02 = 0
    for i in range(n):
        u0, v0, u1, v1 = u[i], v[i], u[(i + 1) % n], v[(i + 1) % n]
        a = u0 * v1 - u1 * v0
        area2 += a
        m10 += a * (u0 + u1)
        m01 += a * (v0 + v1)
        m20 += a * (u0 * u0 + u0 * u1 + u1 * u1)
        m02 += a * (v0 * v0 + v0 * v1 + v1 * v1)
        m11 += a * (2 * u0 * v0 + u0 * v1 + u1 * v0 + 2 * u1 * v1)
    s = [sum(u), sum(v), sum(a * a for a in u), sum(a * b for a, b in zip(u, v)), sum(b * b for b in v)]
    return [wrap(t) for t in [area2, m10, m01, m20, m11, m02] + s]


def hull(xs, ys):
    """The hull vertices [(x, y)] of the point set in the rule's order."""
    pts = sorted(set(zip(xs, ys)))
    if len(pts) <= 1:
        return pts

    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and _cross(out[-1][0] - out[-2][0], out[-1][1] - out[-2][1],
                                           p[0] - out[-1][0], p[1] - out[-1][1]) <= 0:
                out.pop()
            out.append(p)
        return out

    return chain(pts)[:-1] + chain(pts[::-1])[:-1]


def rectangle(h):
    """(hull_area2, rect_edge, along_min, along_max, across, len2) of the hull h."""
    v = len(h)
    if v <= 1:
        return [0] * 6
    area2 = sum(_cross(h[k][0], h[k][1], h[(k + 1) % v][0], h[(k + 1) % v][1]) for k in range(v))
    best = None
    for k in range(v):
        dx, dy = h[(k + 1) % v][0] - h[k][0], h[(k + 1) % v][1] - h[k][1]
        along = [(x - h[k][0]) * dx + (y - h[k][1]) * dy for x, y in h]
        across = [_cross(dx, dy, x - h[k][0], y - h[k][1]) for x, y in h]
        assert min(across) >= 0
        e, n, len2 = max(along) - min(along), max(across), dx * dx + dy * dy
        if best is None or e * n * best[2] < best[0] * best[1] * len2:
            best = (e, n, len2, k, min(along), max(along))
    return [area2, best[3], best[4], best[5], best[1], best[2]]


def shape(chain, width):
    chain = [int(p) for p in chain]
    if not chain:                       # no contours call stores one; the library answers with zeros
        return [], [0] * WORDS
    xs, ys = [p % width for p in chain], [p // width for p in chain]
    h = hull(xs, ys)
    m = [len(h), len(chain), chain[0]] + moments(xs, ys) + rectangle(h)
    assert len(m) == WORDS
    return [y * width + x for x, y in h], m


def csr(chain_offsets, points, point_capacity, width):
    co = [int(v) for v in chain_offsets]
    n_rec = len(co) - 1
    hoff = np.zeros(n_rec + 1, np.uint64)
    measures = np.zeros((n_rec, WORDS), np.int64)
    verts = []
    for j in range(n_rec):
        if co[j + 1] > point_capacity:
            measures[j, 0] = -1
        else:
            h, measures[j] = shape(points[co[j]:co[j + 1]], width)
            verts.extend(h)
        hoff[j + 1] = len(verts)
    return hoff, np.array(verts, np.int32), measures
