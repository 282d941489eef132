"""The edge-curve rule of include/canny_hip.h restated in plain Python, for the tests: edge
linking.  Every set pixel of a map is taken once, in order along its curve; curves are split where they meet; open and
closed curves are told apart.  All integers, purely a function of the map.

Directions are numbered clockwise on the displayed image, as (row, column) steps: 0 E (0,+1), 1 SE (+1,+1), 2 S (+1,0),
3 SW (+1,-1), 4 W (0,-1), 5 NW (-1,-1), 6 N (-1,0), 7 NE (-1,+1); pixels outside the frame are unset.

  1. Links.  Two set 8-neighbours are linked if they are 4-neighbours; diagonal neighbours are linked only if neither of
     the two pixels 4-adjacent to both is set.  deg(p) = the number of p's links.
  2. Nodes.  A node is a set pixel with deg != 2 (isolated 0, curve end 1, junction 3 or 4); the others are path pixels.
  3. Curves.  An isolated pixel p is the curve [p].  From a node p along a link in direction d the walk steps to the
     neighbour and, while that is a path pixel, leaves it by its other link; it ends at a node e that it enters by the
     link that points back from e in direction d'.  The path has the keys 8 * index(p) + d and 8 * index(e) + d' and is
     emitted once, from the smaller, as p, the path pixels, e.  A link-graph component of path pixels only is a closed
     curve: it starts at its smallest index p0, leaves by the smaller of p0's two directions (both among 0..3), lists
     every pixel once and does not repeat p0; its key is 8 * p0 + that direction.
  4. A curve is kept if it has at least min_length points; kept curves are ordered by key.
  5. Record (start, end, points, flags): flags bit 0 CLOSED, bit 1 start is a junction, bit 2 end is a junction, bit 3
     ISOLATED, bits 4..6 the direction of the first step, bits 8..10 the direction of the step that reaches `end`.

curves(mask, min_length) -> (records int32 [K, 4], chains: list of K int32 arrays)
csr(maps, min_length)    -> (records [total, 4], offsets u64 [N + 1], chain_offsets u64 [total + 1], points int32 [P],
                             point_offsets u64 [N + 1])

Nothing here is shared with the library: links are looked up pixel by pixel in a dict."""
import numpy as np

DY = (0, 1, 1, 1, 0, -1, -1, -1)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
CLOSED, START_JUNCTION, END_JUNCTION, ISOLATED = 1, 2, 4, 8
FIRST_DIR_SHIFT, LAST_DIR_SHIFT = 4, 8
START, END, POINTS, FLAGS = 0, 1, 2, 3


def link_sets(mask):
    """{pixel index: tuple of the directions of its links, ascending} for every set pixel of mask (bool [H, W])."""
    m = np.asarray(mask) != 0
    h, w = m.shape

    def at(y, x):
        return 0 <= y < h and 0 <= x < w and bool(m[y, x])

    out = {}
    for y, x in zip(*np.nonzero(m)):
        y, x = int(y), int(x)
        ds = []
        for d in range(8):
            if not at(y + DY[d], x + DX[d]):
                continue
            if d & 1 and (at(y + DY[d], x) or at(y, x + DX[d])):
                continue            # a diagonal that a staircase corner already bridges
            ds.append(d)
        out[y * w + x] = tuple(ds)
    return out


def _follow(links, w, p, d, closed):
    """The walk from p along direction d.  Open: to the first node.  Closed candidate: until it is back at p (the list),
    or None as soon as it meets a node or a pixel with a smaller index."""
    pts, cur, last = [p], p, d
    while True:
        cur += DY[d] * w + DX[d]
        if closed and cur == p:
            return pts, last
        if closed and (len(links[cur]) != 2 or cur < p):
            return None
        pts.append(cur)
        last = d
        if len(links[cur]) != 2:
            return pts, last
        back = (d + 4) & 7
        a, b = links[cur]
        d = b if a == back else a


def all_curves(mask):
    """Every curve of the map in key order: list of (record tuple, points list)."""
    w = np.asarray(mask).shape[1]
    links = link_sets(mask)
    out = []
    for p in sorted(links):
        ds = links[p]
        if not ds:
            out.append(((p, p, 1, ISOLATED), [p]))
        elif len(ds) != 2:
            for d in ds:
                pts, last = _follow(links, w, p, d, False)
                e = pts[-1]
                if 8 * p + d > 8 * e + ((last + 4) & 7):
                    continue        # emitted from the other end
                flags = (d << FIRST_DIR_SHIFT) | (last << LAST_DIR_SHIFT)
                flags |= START_JUNCTION if len(ds) >= 3 else 0
                flags |= END_JUNCTION if len(links[e]) >= 3 else 0
                out.append(((p, e, len(pts), flags), pts))
        elif ds[1] <= 3:
            got = _follow(links, w, p, ds[0], True)
            if got is not None:
                pts, last = got
                out.append(((p, pts[-1], len(pts), CLOSED | (ds[0] << FIRST_DIR_SHIFT) | (last << LAST_DIR_SHIFT)), pts))
    return out


def curves(mask, min_length=1):
    kept = [(r, p) for r, p in all_curves(mask) if len(p) >= min_length]
    records = np.array([r for r, _ in kept], np.int32).reshape(len(kept), 4)
    return records, [np.array(p, np.int32) for _, p in kept]


def csr(maps, min_length=1):
    res = [curves(m, min_length) for m in maps]
    n = len(res)
    offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([r.shape[0] for r, _ in res], dtype=np.uint64)
    chains = [c for _, cs in res for c in cs]
    chain_offsets = np.zeros(len(chains) + 1, np.uint64)
    chain_offsets[1:] = np.cumsum([c.size for c in chains], dtype=np.uint64)
    point_offsets[1:] = np.cumsum([sum(c.size for c in cs) for _, cs in res], dtype=np.uint64)
    records = np.concatenate([r for r, _ in res]) if n else np.zeros((0, 4), np.int32)
    points = np.concatenate(chains).astype(np.int32) if chains else np.zeros(0, np.int32)
    return records, offsets, chain_offsets, points, point_offsets


def check_invariants(mask):
    """What follows from the rule, asserted on one map: every link lies on exactly one curve, path and isolated pixels are
    listed once, a node of degree k >= 1 is listed k times and only as a first or last point, consecutive points are
    linked, deg <= 4."""
    w = np.asarray(mask).shape[1]
    links = link_sets(mask)
    assert all(len(ds) <= 4 for ds in links.values()), "deg <= 4"
    listed, ends, used = {}, {}, {}
    for (start, end, n, flags), pts in all_curves(mask):
        assert n == len(pts) and start == pts[0] and end == pts[-1]
        steps = list(zip(pts, pts[1:])) + ([(pts[-1], pts[0])] if flags & CLOSED else [])
        for a, b in steps:
            d = [k for k in range(8) if b - a == DY[k] * w + DX[k] and k in links[a]]
            assert len(d) == 1 and abs(a % w - b % w) <= 1, f"points {a} -> {b} are not linked"
            key = (min(a, b), max(a, b))
            used[key] = used.get(key, 0) + 1
        for i, p in enumerate(pts):
            listed[p] = listed.get(p, 0) + 1
            if len(links[p]) != 2:
                assert i in (0, n - 1), f"node {p} inside a curve"
                ends[p] = ends.get(p, 0) + 1
        if n > 1:
            assert (flags >> FIRST_DIR_SHIFT) & 7 == [k for k in range(8) if pts[1] - pts[0] == DY[k] * w + DX[k]
                                                       and k in links[pts[0]]][0]
    n_links = sum(len(ds) for ds in links.values())
    assert n_links % 2 == 0 and len(used) == n_links // 2 and set(used.values()) <= {1}, "every link on exactly one curve"
    for p, ds in links.items():
        want = 1 if len(ds) in (0, 2) else len(ds)
        assert listed.get(p, 0) == want, f"pixel {p} of degree {len(ds)} listed {listed.get(p, 0)} times"


def _draw(rows):
    return np.array([[c == "#" for c in r] for r in rows], bool)


def designed_maps():
    """Small maps that each exercise one case of the rule, by name."""
    import components_rule as cr

    sq = np.zeros((7, 7), bool)
    sq[1:6, 1:6] = True
    sq[2:5, 2:5] = False                                  # a 5 x 5 square ring: 16 points, CLOSED
    diamond = np.zeros((11, 11), bool)
    for i in range(5):                                    # diagonal links only: 16 points, CLOSED
        diamond[1 + i, 5 + i] = diamond[5 + i, 9 - i] = diamond[9 - i, 5 - i] = diamond[5 - i, 1 + i] = True
    saw = np.zeros((12, 23), bool)                        # a ring whose top is a sawtooth: several candidates, one owner
    for x in range(1, 22):
        saw[2 + (x - 1) % 4 if (x - 1) % 4 < 3 else 3, x] = True
    saw[2:10, 1] = saw[2:10, 21] = True
    saw[10, 1:22] = True
    saw[2, 1] = saw[2, 21] = False
    plus = np.zeros((9, 9), bool)
    plus[4, 1:8] = plus[1:8, 4] = True
    x_map = np.zeros((9, 9), bool)
    for i in range(1, 8):
        x_map[i, i] = x_map[i, 8 - i] = True
    t_map = np.zeros((8, 11), bool)
    t_map[1, 1:10] = t_map[1:7, 5] = True
    lollipop = _draw([".........",
                     "..####...",
                     "..#..#...",
                     "..#..#...",
                     "..####...",
                     "..#......",
                     "..#......",
                     "........."])
    eight = _draw(["......",          # two diamond loops through one junction pixel of degree 4
                   "..#...",
                   ".#.#..",
                   "..#...",
                   ".#.#..",
                   "..#...",
                   "......"])
    two_nodes = _draw([".....",
                       ".##..",
                       "....."])
    two_junctions = _draw(["..#..#..",
                                "..#..#..",
                                ".######.",
                                "..#..#..",
                                "..#..#.."])
    return {
        "square_ring": sq, "diamond_ring": diamond, "sawtooth_ring": saw, "plus": plus, "x": x_map, "t": t_map,
        "lollipop": lollipop, "figure_eight": eight, "two_nodes": two_nodes, "two_junctions": two_junctions,
        "all_set": np.ones((8, 9), bool), "checkerboard": cr.checkerboard(8, 9), "staircase": cr.staircase(8, 9),
        "serpentine": cr.serpentine(64, 64), "1x1": np.ones((1, 1), bool), "1x70": np.ones((1, 70), bool),
        "70x1": np.ones((70, 1), bool),
    }


def random_maps(h=37, w=53, densities=(0.05, 0.2, 0.35, 0.5, 0.7, 0.9), seeds=(0, 1, 2)):
    return {f"random_{d}_{s}": np.random.default_rng(1000 * s + int(100 * d)).random((h, w)) < d
            for d in densities for s in seeds}


def embed(m, h, w):
    """m in the top-left corner of an h x w map of zeros."""
    out = np.zeros((h, w), bool)
    out[:m.shape[0], :m.shape[1]] = m
    return out
