"""The connected-component rule of include/canny_hip.h restated in numpy, for the tests.

components(mask, min_area) -> (labels int32 [H, W], stats int32 [K, 6]):
  the set pixels are partitioned by 8-connectivity; a component has area = its pixel count and first = its smallest index
  r * width + c; components with area >= min_area are kept and numbered 1..K by ascending first; labels holds the number
  on the component's pixels and 0 elsewhere; stats[k - 1] = (left, top, width, height, area, first).

Nothing here is shared with the library: rows are cut into runs (whole-row runs, not 64-pixel words), runs of adjacent
rows that touch (columns a - 1 .. b + 1) become graph edges, and the graph is resolved by repeated hooking of roots onto the
smaller neighbouring root followed by full pointer jumping.  Runs are numbered in raster order, so the smallest run of a
component starts at the component's first pixel."""
import numpy as np

LEFT, TOP, WIDTH, HEIGHT, AREA, FIRST = range(6)


def _runs(mask):
    h, w = mask.shape
    padded = np.zeros((h, w + 2), np.int8)
    padded[:, 1:-1] = mask
    d = np.diff(padded, axis=1)                 # +1 at a run's first column, -1 one past its last
    rows, x0 = np.nonzero(d == 1)               # row-major: raster order of the runs
    _, x1 = np.nonzero(d == -1)
    return rows.astype(np.int64), x0.astype(np.int64), x1.astype(np.int64) - 1


def _edges(rows, x0, x1, w):
    """Pairs (a, b) of runs with row[b] = row[a] + 1 that touch: x0[b] <= x1[a] + 1 and x1[b] >= x0[a] - 1."""
    stride = w + 4
    key_start, key_end = rows * stride + x0 + 1, rows * stride + x1 + 1   # both ascending (runs are disjoint, in order)
    below = (rows + 1) * stride
    lo = np.searchsorted(key_end, below + x0, side="left")                # first run below with x1[b] + 1 >= x0[a]
    hi = np.searchsorted(key_start, below + x1 + 2, side="right")         # past the last with x0[b] + 1 <= x1[a] + 2
    cnt = np.maximum(hi - lo, 0)
    a = np.repeat(np.arange(rows.size), cnt)
    b = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return a, b


def _roots(n, a, b):
    p = np.arange(n)
    while a.size:
        pa, pb = p[a], p[b]
        live = pa != pb
        if not live.any():
            break
        a, b, pa, pb = a[live], b[live], pa[live], pb[live]
        m = np.minimum(pa, pb)
        np.minimum.at(p, pa, m)
        np.minimum.at(p, pb, m)
        while True:                              # full pointer jumping
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    return p


def components(mask, min_area=1):
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    rows, x0, x1 = _runs(mask)
    n = rows.size
    if n == 0:
        return np.zeros((h, w), np.int32), np.zeros((0, 6), np.int32)
    root = _roots(n, *_edges(rows, x0, x1, w))
    length = x1 - x0 + 1
    area = np.bincount(root, weights=length, minlength=n).astype(np.int64)
    left, right = np.full(n, w), np.full(n, -1)
    bottom = np.full(n, -1)
    np.minimum.at(left, root, x0)
    np.maximum.at(right, root, x1)
    np.maximum.at(bottom, root, rows)
    is_root = root == np.arange(n)
    kept = np.flatnonzero(is_root & (area >= min_area))   # ascending run number = ascending first pixel
    number = np.zeros(n, np.int64)
    number[kept] = np.arange(1, kept.size + 1)
    stats = np.stack([left[kept], rows[kept], right[kept] - left[kept] + 1, bottom[kept] - rows[kept] + 1, area[kept],
                      rows[kept] * w + x0[kept]], axis=1).astype(np.int32)
    k = number[root]
    delta = np.zeros(h * w + 1, np.int64)
    np.add.at(delta, rows * w + x0, k)
    np.add.at(delta, rows * w + x1 + 1, -k)
    labels = np.cumsum(delta[:-1]).reshape(h, w).astype(np.int32)
    return labels, stats


def csr(maps, min_area=1):
    """(labels [N, H, W], stats [total, 6], offsets uint64 [N + 1]) of a stack of maps."""
    res = [components(m, min_area) for m in maps]
    offsets = np.zeros(len(res) + 1, np.uint64)
    offsets[1:] = np.cumsum([s.shape[0] for _, s in res], dtype=np.uint64)
    return np.stack([l for l, _ in res]), np.concatenate([s for _, s in res]), offsets


# ---- directed masks ------------------------------------------------------------------------------------------------
def serpentine(h, w):
    """A one-pixel-wide path: every second row full, joined alternately at the right and the left end."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m


def spiral(n):
    """A one-pixel-wide square spiral, walked inwards with one blank ring between the turns: one component."""
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx                       # the cell after the next one
        if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
            dy, dx = dx, -dy                            # turn right
            turns += 1
            continue
        y, x, turns = ny, nx, 0
        m[y, x] = True
    return m


def staircase(h, w):
    """An anti-diagonal one-pixel staircase x + y = c: pixels touch only diagonally; where the frame reaches it, c = 127
    takes it from (63, 64) to (64, 63), across the corner of four 64 x 64 tiles."""
    m = np.zeros((h, w), bool)
    c = 127 if h > 64 and w > 64 else w - 1
    y = np.arange(h)
    ok = (c - y >= 0) & (c - y < w)
    m[y[ok], c - y[ok]] = True
    return m


def checkerboard(h, w):
    """Isolated pixels on a pitch of 2: the largest possible number of components, every area 1."""
    m = np.zeros((h, w), bool)
    m[0::2, 0::2] = True
    return m


def combs(h, w):
    """Two combs whose teeth interleave without touching: exactly two components."""
    m = np.zeros((h, w), bool)
    m[0, :] = True
    m[h - 1, :] = True
    m[0:h - 2, 0::4] = True        # teeth hanging from the top row
    m[2:h, 2::4] = True            # teeth standing on the bottom row
    return m


def directed_masks(h, w):
    return {"diagonal_pair": _diag_pair(h, w), "staircase": staircase(h, w), "checkerboard": checkerboard(h, w),
            "all_set": np.ones((h, w), bool), "all_clear": np.zeros((h, w), bool), "spiral": _embed(spiral(min(h, w)), h, w),
            "serpentine": serpentine(h, w), "combs": combs(h, w)}


def _embed(m, h, w):
    out = np.zeros((h, w), bool)
    out[:m.shape[0], :m.shape[1]] = m
    return out


def _diag_pair(h, w):
    m = np.zeros((h, w), bool)
    if h >= 2 and w >= 2:
        y, x = min(h - 1, 64), min(w - 1, 64)   # across the tile corner where the frame reaches it
        m[y - 1, x] = True
        m[y, x - 1] = True
    return m
