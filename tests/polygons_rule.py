"""The polygon rule of include/canny_hip.h restated in plain Python, for the tests.

The input is one stored chain P_0 .. P_{n-1}: pixel indices r * width + c, read as (x, y) = (c, r); the chain is closed,
P_n means P_0.  The parameters are epsilon_q8 (absolute, 1/256 pixel) and ratio_q16 (relative to the chain's own length,
1/65536, < 65536); they add.

  1. length_q8 = 256 * (axis steps) + 362 * (diagonal steps) over the n cyclic steps; a step between equal points (n == 1)
     counts nothing.
  2. eps = min(epsilon_q8 + ((ratio_q16 * length_q8) >> 16), 2^24).
  3. n == 1: the polygon is [P_0].  Otherwise k = the smallest i that maximises |P_i - P_0|^2; 0 and k are vertices.
  4. simplify (0, k) and (k, n).  simplify (a, b), b - a >= 2: c_i = |cross(P_b - P_a, P_i - P_a)| for a < i < b, m = the
     smallest i that maximises c_i; if c_m^2 * 2^16 > eps^2 * |P_b - P_a|^2, m is a vertex and (a, m), (m, b) are
     simplified in turn.  INVARIANT (asserted): the two ends of every run are different pixels.
  5. the polygon: the vertex positions in chain order, as the pixel indices P_i.
  6. measures (vertices, length_q8, area2, convex).

polygon(chain, width, eps_q8, ratio_q16) -> (positions: list of int, measures: 4 ints)
csr(chain_offsets, points, point_capacity, width, eps_q8, ratio_q16)
    -> (vertex_offsets u64 [R + 1], vertices int32 [total], measures int64 [R, 4]); a record whose chain ends beyond
       point_capacity has no vertices and the measures (-1, 0, 0, 0).

Nothing here is shared with the library: recursion, Python ints."""
import sys

import numpy as np

EPS_MAX = 1 << 24


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def length_q8(xs, ys):
    n = len(xs)
    axis = diag = 0
    for i in range(n):
        dx, dy = xs[(i + 1) % n] - xs[i], ys[(i + 1) % n] - ys[i]
        if dx and dy:
            diag += 1
        elif dx or dy:
            axis += 1
    return 256 * axis + 362 * diag


def tolerance(eps_q8, ratio_q16, length):
    assert 0 <= ratio_q16 < 65536 and eps_q8 >= 0
    return min(eps_q8 + ((ratio_q16 * length) >> 16), EPS_MAX)


def positions(xs, ys, eps):
    """The vertex positions of the closed chain (xs, ys) at the tolerance eps (q8), ascending."""
    n = len(xs)
    if n == 0:
        return []
    if n == 1:
        return [0]
    d2 = [(xs[i] - xs[0]) ** 2 + (ys[i] - ys[0]) ** 2 for i in range(n)]
    k = d2.index(max(d2))
    keep = {0, k}
    px, py = list(xs) + [xs[0]], list(ys) + [ys[0]]          # position n means P_0

    def simplify(a, b):
        assert (px[a], py[a]) != (px[b], py[b]), "the two ends of a run are different pixels"
        if b - a < 2:
            return
        bx, by = px[b] - px[a], py[b] - py[a]
        c = [abs(_cross(bx, by, px[i] - px[a], py[i] - py[a])) for i in range(a + 1, b)]
        cm = max(c)
        m = a + 1 + c.index(cm)
        if cm * cm * 65536 > eps * eps * (bx * bx + by * by):
            keep.add(m)
            simplify(a, m)
            simplify(m, b)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2 * n + 1000))
    try:
        simplify(0, k)
        simplify(k, n)
    finally:
        sys.setrecursionlimit(limit)
    return sorted(keep)


def measures_of(vx, vy, length):
    v = len(vx)
    area = sum(_cross(vx[i], vy[i], vx[(i + 1) % v], vy[(i + 1) % v]) for i in range(v))
    turns = [_cross(vx[(i + 1) % v] - vx[i], vy[(i + 1) % v] - vy[i], vx[(i + 2) % v] - vx[(i + 1) % v],
                    vy[(i + 2) % v] - vy[(i + 1) % v]) for i in range(v)]
    pos, neg = any(t > 0 for t in turns), any(t < 0 for t in turns)
    return v, length, abs(area), int(v >= 3 and pos != neg)


def polygon(chain, width, eps_q8=0, ratio_q16=0):
    chain = [int(p) for p in chain]
    xs, ys = [p % width for p in chain], [p // width for p in chain]
    length = length_q8(xs, ys)
    pos = positions(xs, ys, tolerance(eps_q8, ratio_q16, length))
    return pos, measures_of([xs[i] for i in pos], [ys[i] for i in pos], length)


def csr(chain_offsets, points, point_capacity, width, eps_q8=0, ratio_q16=0):
    co = [int(v) for v in chain_offsets]
    n_rec = len(co) - 1
    voff = np.zeros(n_rec + 1, np.uint64)
    measures = np.zeros((n_rec, 4), np.int64)
    verts = []
    for j in range(n_rec):
        if co[j + 1] > point_capacity:
            measures[j] = (-1, 0, 0, 0)
        else:
            chain = points[co[j]:co[j + 1]]
            pos, measures[j] = polygon(chain, width, eps_q8, ratio_q16)
            verts.extend(int(chain[i]) for i in pos)
        voff[j + 1] = len(verts)
    return voff, np.array(verts, np.int32), measures
