"""The thinning rule of include/canny_hip.h, restated in numpy on unpacked frames.

Bit maps are uint8 [n_frames, h, ceil(w / 8)], rows MSB-first.  Neighbours of P1 = (y, x): P2 = (y-1, x), P3 = (y-1, x+1),
P4 = (y, x+1), P5 = (y+1, x+1), P6 = (y+1, x), P7 = (y+1, x-1), P8 = (y, x-1), P9 = (y-1, x-1); everything outside the frame
reads 0.  One full iteration is sub-iteration 0 on the whole frame, then sub-iteration 1 on the result.  Nothing here shares
code with the library.
"""
import numpy as np

from morph_rule import pack, pack_dirty, unpack  # noqa: F401  (re-exported for the tests)

ZHANGSUEN, GUOHALL = 0, 1
METHODS = (ZHANGSUEN, GUOHALL)
MAX_ITERATIONS = 16384
# (dy, dx) of P2 .. P9
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))

# the named mutants of the rule (tests/test_thin_rule.py shows that each changes a named map)
MUTANTS = ("swapped_subs", "b_le_7", "no_wrap", "replicate", "gh_max")


def neighbours(px, replicate=False):
    """bool [..., h, w] -> the eight planes P2 .. P9 (int8)."""
    h, w = px.shape[-2:]
    p = np.pad(px.astype(np.int8), ((0, 0),) * (px.ndim - 2) + ((1, 1), (1, 1)), mode="edge" if replicate else "constant")
    return [p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in RING]


def deletions(px, method, sub, mutant=None):
    """bool [..., h, w]: the pixels sub-iteration `sub` deletes from px."""
    if mutant == "swapped_subs":
        sub = 1 - sub
    p2, p3, p4, p5, p6, p7, p8, p9 = neighbours(px, replicate=mutant == "replicate")
    ring = [p2, p3, p4, p5, p6, p7, p8, p9]
    if method == ZHANGSUEN:
        b = sum(ring)
        pairs = 7 if mutant == "no_wrap" else 8
        a = sum((1 - ring[i]) * ring[(i + 1) % 8] for i in range(pairs))
        ok = (b >= 2) & (b <= (7 if mutant == "b_le_7" else 6)) & (a == 1)
        if sub == 0:
            ok &= (p2 * p4 * p6 == 0) & (p4 * p6 * p8 == 0)
        else:
            ok &= (p2 * p4 * p8 == 0) & (p2 * p6 * p8 == 0)
    elif method == GUOHALL:
        c = (1 - p2) * (p3 | p4) + (1 - p4) * (p5 | p6) + (1 - p6) * (p7 | p8) + (1 - p8) * (p9 | p2)
        n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8)
        n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
        n = np.maximum(n1, n2) if mutant == "gh_max" else np.minimum(n1, n2)
        if sub == 0:
            m = (p6 | p7 | (1 - p9)) & p8
        else:
            m = (p2 | p3 | (1 - p5)) & p4
        ok = (c == 1) & (n >= 2) & (n <= 3) & (m == 0)
    else:
        raise ValueError(method)
    return px & ok


def iteration(px, method, mutant=None):
    """One full iteration of bool [..., h, w] -> (the maps, pixels deleted per frame)."""
    n = 0
    for sub in (0, 1):
        d = deletions(px, method, sub, mutant)
        n = n + d.sum(axis=(-2, -1))
        px = px & ~d
    return px, n


def thin_px(px, method, max_iterations=0, mutant=None):
    """bool [h, w] -> (out, iterations, converged): the map after min(k, D) full iterations, D for k = 0."""
    if not 0 <= max_iterations <= MAX_ITERATIONS:
        raise ValueError(max_iterations)
    px = np.asarray(px, bool)
    it = 0
    while max_iterations == 0 or it < max_iterations:
        nxt, n = iteration(px, method, mutant)
        if n == 0:
            return px, it, 1
        px, it = nxt, it + 1
    return px, it, 0


def thin(bits, w, method, max_iterations=0):
    """bits uint8 [n, h, ceil(w / 8)] -> (out bits, info int64 [n, 4]: set bits, iterations, deleted, converged)."""
    if not 0 <= max_iterations <= MAX_ITERATIONS:
        raise ValueError(max_iterations)
    px = unpack(bits, w)
    out = px.copy()
    info = np.zeros((px.shape[0], 4), np.int64)
    it = 0
    while max_iterations == 0 or it < max_iterations:   # all frames side by side: a frame at its fixed point stays there
        nxt, n = iteration(out, method)
        info[:, 1] += n > 0
        info[:, 3] |= n == 0
        if not (n > 0).any():
            break
        out, it = nxt, it + 1
    info[:, 0] = out.sum(axis=(1, 2))
    info[:, 2] = px.sum(axis=(1, 2)) - info[:, 0]
    return pack(out), info


# ---- a second, independent restatement: one pixel at a time, for tiny maps ---------------------------------------------------
def thin_loop(px, method, max_iterations=0):
    a = [[int(v) for v in row] for row in np.asarray(px, bool)]
    h, w = len(a), len(a[0])

    def at(y, x):
        return a[y][x] if 0 <= y < h and 0 <= x < w else 0

    it = 0
    while max_iterations == 0 or it < max_iterations:
        total = 0
        for sub in (0, 1):
            gone = []
            for y in range(h):
                for x in range(w):
                    if not a[y][x]:
                        continue
                    r = [at(y + dy, x + dx) for dy, dx in RING]
                    p2, p3, p4, p5, p6, p7, p8, p9 = r
                    if method == ZHANGSUEN:
                        trans = sum(1 for i in range(8) if r[i] == 0 and r[(i + 1) % 8] == 1)
                        guard = (p2 and p4 and p6) or (p4 and p6 and p8) if sub == 0 else (p2 and p4 and p8) or (p2 and p6 and p8)
                        if 2 <= sum(r) <= 6 and trans == 1 and not guard:
                            gone.append((y, x))
                    else:
                        c = sum(1 for u, v, q in ((p2, p3, p4), (p4, p5, p6), (p6, p7, p8), (p8, p9, p2)) if not u and (v or q))
                        n1 = sum(1 for u, v in ((p9, p2), (p3, p4), (p5, p6), (p7, p8)) if u or v)
                        n2 = sum(1 for u, v in ((p2, p3), (p4, p5), (p6, p7), (p8, p9)) if u or v)
                        m = ((p6 or p7 or not p9) and p8) if sub == 0 else ((p2 or p3 or not p5) and p4)
                        if c == 1 and 2 <= min(n1, n2) <= 3 and not m:
                            gone.append((y, x))
            for y, x in gone:
                a[y][x] = 0
            total += len(gone)
        if total == 0:
            return np.array(a, bool), it, 1
        it += 1
    return np.array(a, bool), it, 0


# ---- a model of the fused route: tiles with a halo, `fuse` full iterations a launch -----------------------------------------
def fused_model(px, method, max_iterations=0, tile=(16, 16), fuse=1, halo=None):
    """The frame cut into tiles; a launch stages every tile with `halo` pixels around it (2 * fuse unless given; clipped to the
    frame, beyond the staged region reads 0), runs min(fuse, remaining) iterations on the staged region alone and keeps the
    tile; deletions are counted over the tiles' own pixels.  -> (out, iterations, converged) like thin_px."""
    px = np.asarray(px, bool)
    h, w = px.shape
    th, tw = tile
    halo = 2 * fuse if halo is None else halo
    it = 0
    while max_iterations == 0 or it < max_iterations:
        n_it = fuse if max_iterations == 0 else min(fuse, max_iterations - it)
        out = np.zeros_like(px)
        deleted = np.zeros(n_it, np.int64)
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                ya, yb, xa, xb = max(0, y0 - halo), min(h, y0 + th + halo), max(0, x0 - halo), min(w, x0 + tw + halo)
                s = px[ya:yb, xa:xb].copy()
                core = (slice(y0 - ya, min(y0 + th, h) - ya), slice(x0 - xa, min(x0 + tw, w) - xa))
                for i in range(n_it):
                    before = int(s[core].sum())
                    s, n = iteration(s, method)
                    deleted[i] += before - int(s[core].sum())
                    if n == 0:
                        break  # a fixed point of the staged region
                out[y0:y0 + th, x0:x0 + tw] = s[core]
        done = int(np.argmax(deleted == 0)) if (deleted == 0).any() else n_it
        px = out
        it += done
        if done < n_it:
            return px, it, 1
    return px, it, 0


# ---- the maps the CPU and the GPU tests share ---------------------------------------------------------------------------
def demo_scene():
    """bool [96, 160]: an 8-pixel-thick ring and a 7-pixel-thick bar."""
    yy, xx = np.mgrid[:96, :160]
    r2 = (yy - 48) ** 2 + (xx - 40) ** 2
    return ((r2 >= 22 ** 2) & (r2 <= 30 ** 2)) | ((np.abs(yy - 20) <= 3) & (xx >= 90) & (xx <= 150))


def bar(h, w, y0, t, x0=0, x1=None):
    a = np.zeros((h, w), bool)
    a[y0:y0 + t, x0:w if x1 is None else x1] = True
    return a


def square2():
    a = np.zeros((6, 6), bool)
    a[2:4, 2:4] = True
    return a


def diagonal2(n=12, pad=2, x_off=0):
    d = np.eye(n, dtype=bool) | np.eye(n, k=1, dtype=bool)
    a = np.zeros((n + 2 * pad, n + 2 * pad + x_off), bool)
    a[pad:pad + n, pad + x_off:pad + x_off + n] = d
    return a


def blobs(h, w, seed, size=5):
    from scipy.ndimage import uniform_filter
    rng = np.random.default_rng(seed)
    return uniform_filter(rng.random((h, w)), size) > 0.5


def components8(px):
    from scipy.ndimage import label
    return int(label(px, structure=np.ones((3, 3), int))[1])
