"""The distance-transform rule of include/canny_hip.h restated in numpy, for the tests.

For a mask with set pixels S:
  dist2[r, c]   = min over (r', c') in S of (r - r')^2 + (c - c')^2          (an integer; 0 on set pixels)
  nearest[r, c] = the smallest index r' * width + c' among the pixels of S that attain it
  dist          = sqrt(dist2 as float64) rounded to float32
  S empty: dist2 = NONE everywhere, nearest = -1, dist = +inf.

brute() is that definition taken literally (all pairs).  separable() is a vectorised restatement for larger frames and is
checked against brute() by tests/test_edt_rule.py.  Nothing here is shared with the library: separable() searches rows
outwards from each pixel and stops when no farther row can matter; it builds no envelope of parabolas."""
import numpy as np

NONE = 0x7FFFFFFF


def _empty(h, w):
    return np.full((h, w), NONE, np.int32), np.full((h, w), -1, np.int32)


def brute(mask, pairs_per_chunk=1 << 22):
    """(dist2 int32 [H, W], nearest int32 [H, W]) from all pixel / set-pixel pairs, in chunks of pixels."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    ys, xs = np.nonzero(mask)                        # raster order: ascending index
    if ys.size == 0:
        return _empty(h, w)
    index = ys * w + xs
    r, c = np.divmod(np.arange(h * w), w)
    d2 = np.empty(h * w, np.int64)
    nn = np.empty(h * w, np.int64)
    step = max(1, pairs_per_chunk // ys.size)
    for a in range(0, h * w, step):
        d = (r[a:a + step, None] - ys) ** 2 + (c[a:a + step, None] - xs) ** 2
        k = d.argmin(axis=1)                         # the first minimum: the smallest index
        d2[a:a + step] = d[np.arange(k.size), k]
        nn[a:a + step] = index[k]
    return d2.reshape(h, w).astype(np.int32), nn.reshape(h, w).astype(np.int32)


def nearest_in_row(mask):
    """[H, W] int64: the column of the set pixel of the same row nearest to each pixel, the left one of two equally near,
    -1 where the row has none."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    cols = np.arange(w)
    far = 4 * w + 4
    left = np.maximum.accumulate(np.where(mask, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(mask, cols, far)[:, ::-1], axis=1)[:, ::-1]
    take_right = (right < far) & ((left < 0) | (right - cols < cols - left))
    return np.where(take_right, right, left)


def separable(mask, band=64):
    """The same two planes as brute().  Per row the nearest set column (left on ties); then every pixel looks at the rows
    x, x - 1, x + 1, x - 2, ... of its column: an earlier (smaller) row wins ties, and the search of a band of rows ends
    when the row offset alone exceeds every distance found."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    if not mask.any():
        return _empty(h, w)
    g = nearest_in_row(mask)
    hh = np.where(g >= 0, (np.arange(w) - g) ** 2, 1 << 31).astype(np.uint32)     # 2^31 + k^2 < 2^32: no wrap-around
    best = np.full((h, w), 0xFFFFFFFF, np.uint32)
    best_r = np.zeros((h, w), np.int32)
    rows = np.arange(h, dtype=np.int32)[:, None]
    for x0 in range(0, h, band):
        x1 = min(h, x0 + band)
        b, br = best[x0:x1], best_r[x0:x1]
        k = 0
        while k < h:
            k2 = np.uint32(k * k)
            lo = max(x0, k)                          # rows x >= k look up at row x - k: smaller than every row seen so far
            if lo < x1:
                cand = hh[lo - k:x1 - k] + k2
                m = cand <= b[lo - x0:]
                np.copyto(b[lo - x0:], cand, where=m)
                np.copyto(br[lo - x0:], rows[lo - k:x1 - k], where=m)
            hi = min(x1, h - k)                      # rows x < h - k look down at row x + k: larger than every row seen
            if k and x0 < hi:
                cand = hh[x0 + k:hi + k] + k2
                m = cand < b[:hi - x0]
                np.copyto(b[:hi - x0], cand, where=m)
                np.copyto(br[:hi - x0], rows[x0 + k:hi + k], where=m)
            k += 1
            if k * k > int(b.max()):
                break
    nearest = best_r.astype(np.int64) * w + np.take_along_axis(g, best_r.astype(np.int64), axis=0)
    return best.astype(np.int32), nearest.astype(np.int32)


def dist_of(dist2):
    """The float plane the rule derives from dist2."""
    d2 = np.asarray(dist2)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return np.where(d2 == NONE, np.float32(np.inf), d).astype(np.float32)


def transform(mask):
    """(dist2, dist, nearest) of one mask: by the definition where the pairs are few (sparse masks, where the outward
    search of separable() runs longest), by the vectorised form otherwise."""
    mask = np.asarray(mask) != 0
    d2, nn = brute(mask) if int(mask.sum()) * mask.size <= 1 << 26 else separable(mask)
    return d2, dist_of(d2), nn


def stack(masks):
    res = [transform(m) for m in masks]
    return tuple(np.stack([r[k] for r in res]) for k in range(3))


# ---- directed masks ------------------------------------------------------------------------------------------------
def serpentine(h, w):
    """A one-pixel-wide path: every second row full, joined alternately at the right and the left end."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m


def spiral(n):
    """A one-pixel-wide square spiral, walked inwards with one blank ring between the turns."""
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


def _single(h, w, y, x):
    m = np.zeros((h, w), bool)
    m[y, x] = True
    return m


def directed_masks(h, w):
    """Named masks [h, w]: the cases in which the tie rule, the sentinels and the borders decide the result."""
    out = {"empty": np.zeros((h, w), bool), "full": np.ones((h, w), bool),
           "top_left": _single(h, w, 0, 0), "top_right": _single(h, w, 0, w - 1),
           "bottom_left": _single(h, w, h - 1, 0), "bottom_right": _single(h, w, h - 1, w - 1),
           "centre": _single(h, w, h // 2, w // 2)}
    m = np.zeros((h, w), bool)
    m[h // 3] = True
    out["one_row"] = m
    m = np.zeros((h, w), bool)
    m[:, (2 * w) // 3] = True
    out["one_column"] = m
    m = np.zeros((h, w), bool)
    m[0::2, 0::2] = True
    out["checkerboard"] = m                              # ties everywhere
    m = np.zeros((h, w), bool)                          # two pixels equally far from every pixel of the row between them
    k = min(h // 2, 5)
    m[h // 2 - k, w // 2] = True
    m[min(h - 1, h // 2 + k), w // 2] = True
    out["tie_above_below"] = m
    m = np.zeros((h, w), bool)                          # ... and of the column between them
    k = min(w // 2, 7)
    m[h // 2, w // 2 - k] = True
    m[h // 2, min(w - 1, w // 2 + k)] = True
    out["tie_left_right"] = m
    return out


def directed_masks_large(h, w):
    named = directed_masks(h, w)
    named["serpentine"] = serpentine(h, w)
    s = spiral(min(h, w))
    m = np.zeros((h, w), bool)
    m[:s.shape[0], :s.shape[1]] = s
    named["spiral"] = m
    return named
