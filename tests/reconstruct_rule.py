"""The reconstruction rule of include/canny_hip.h, restated in numpy on unpacked frames.

Bit maps are uint8 [n_frames, h, ceil(w / 8)], rows MSB-first; a column >= w is outside the frame.  M = the in-frame set of the
mask, B = the border ring, R_c(S, G) = the pixels of G joined to a pixel of S & G by a c-connected path inside G.
SEEDED: R_c(marker, M).  FILL_HOLES: frame \\ R_c'(B, frame \\ M), c' = 12 - c.  CLEAR_BORDER: M \\ R_c(B, M).
Nothing here shares code with the library.
"""
import numpy as np

from morph_rule import pack, pack_dirty, unpack  # noqa: F401  (re-exported for the tests)
from thin_rule import demo_scene  # noqa: F401

SEEDED, FILL_HOLES, CLEAR_BORDER = 0, 1, 2
OPS = (SEEDED, FILL_HOLES, CLEAR_BORDER)
CONNECTIVITIES = (4, 8)
INFO = 3
TILE = (64, 512)   # rows x columns of a tile of the kernels

# the named slips (tests/test_reconstruct_rule.py shows that each changes its designed map)
MUTANTS = ("eight_at_4", "same_connectivity", "pad_conducts", "rows_wrap", "frames_touch", "no_word_carry", "no_tile_carry",
           "halo_wrong_row", "first_chunk_only")


def border(h, w):
    b = np.zeros((h, w), bool)
    b[0], b[-1], b[:, 0], b[:, -1] = True, True, True, True
    return b


def dilate(s, c, mutant=None):
    """bool [..., h, w] -> the pixels with a c-neighbour (or themselves) in s; outside the frame nothing is set."""
    h, w = s.shape[-2:]
    if mutant == "eight_at_4":
        c = 8
    p = np.pad(s, ((0, 0),) * (s.ndim - 2) + ((1, 1), (1, 1)))
    cut = lambda dy, dx: p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    out = s | cut(-1, 0) | cut(1, 0)
    left, right = cut(0, -1), cut(0, 1)   # the neighbour at x - 1, at x + 1
    if mutant == "rows_wrap":             # the row is one stretch of memory: x - 1 of column 0 is the row before's last pixel
        flat = s.reshape(s.shape[:-2] + (h * w,))
        z = np.zeros(flat.shape[:-1] + (1,), bool)
        left = np.concatenate([z, flat[..., :-1]], -1).reshape(s.shape)
        right = np.concatenate([flat[..., 1:], z], -1).reshape(s.shape)
    if mutant == "no_word_carry":         # a horizontal step never leaves its 64-column word
        x = np.arange(w)
        left, right = left & (x % 64 != 0), right & (x % 64 != 63)
    out = out | left | right
    if c == 8:
        out = out | cut(-1, -1) | cut(-1, 1) | cut(1, -1) | cut(1, 1)
    return out


def propagate(start, g, c, mutant=None):
    """R_c(start, g) on bool [..., h, w] by iterated geodesic dilation."""
    s = start & g
    while True:
        t = dilate(s, c, mutant) & g
        if np.array_equal(t, s):
            return s
        s = t


def reconstruct_px(marker, mask, op, c, mutant=None):
    """bool [..., h, w] (marker None unless op is SEEDED) -> (out, start set)."""
    if c not in CONNECTIVITIES or op not in OPS or (marker is None) != (op != SEEDED):
        raise ValueError((op, c))
    mask = np.asarray(mask, bool)
    if mutant == "frames_touch" and mask.ndim == 3:   # the batch is one tall frame
        n, h, w = mask.shape
        tall = lambda a: None if a is None else np.asarray(a, bool).reshape(1, n * h, w)
        out, start = reconstruct_px(tall(marker), tall(mask), op, c)
        return out.reshape(n, h, w), start.reshape(n, h, w)
    b = border(*mask.shape[-2:])
    if op == SEEDED:
        start = np.asarray(marker, bool) & mask
        return propagate(start, mask, c, mutant), start
    if op == FILL_HOLES:
        start = b & ~mask
        return ~propagate(start, ~mask, c if mutant == "same_connectivity" else 12 - c, mutant), start
    start = b & mask
    return mask & ~propagate(start, mask, c, mutant), start


def reconstruct(marker_bits, mask_bits, w, op, c, mutant=None):
    """bits uint8 [n, h, ceil(w / 8)] -> (out bits, info int64 [n, 3]: set bits of the output, of M, of the start set)."""
    if mutant == "pad_conducts":          # the pad columns belong to the frame
        w8 = mask_bits.shape[-1] * 8
        out, info = reconstruct(marker_bits, mask_bits, w8, op, c)
        return pack(unpack(out, w)), info
    mask = unpack(mask_bits, w)
    marker = None if marker_bits is None else unpack(marker_bits, w)
    out, start = reconstruct_px(marker, mask, op, c, mutant)
    info = np.stack([out.sum(axis=(1, 2)), mask.sum(axis=(1, 2)), start.sum(axis=(1, 2))], axis=1).astype(np.int64)
    return pack(out), info


# ---- the rule a second time: a stack flood, one pixel at a time ---------------------------------------------------------------
def flood_px(marker, mask, op, c):
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    steps = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
    if op == FILL_HOLES:
        g, c = ~mask, 12 - c
    else:
        g = mask
    on_border = lambda y, x: y == 0 or y == h - 1 or x == 0 or x == w - 1
    reached = [[False] * w for _ in range(h)]
    stack = []
    for y in range(h):
        for x in range(w):
            if g[y, x] and (marker[y][x] if op == SEEDED else on_border(y, x)):
                reached[y][x] = True
                stack.append((y, x))
    while stack:
        y, x = stack.pop()
        for dy, dx in steps[:c]:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and g[yy, xx] and not reached[yy][xx]:
                reached[yy][xx] = True
                stack.append((yy, xx))
    r = np.array(reached, bool).reshape(h, w)
    return r if op == SEEDED else (~r if op == FILL_HOLES else mask & ~r)


# ---- a model of the tile flood's launches ------------------------------------------------------------------------------------
def tile_model(marker, mask, c, tile=TILE, mutant=None):
    """bool [h, w]: the launches of the tile flood.  In a launch every tile runs to its own fixed point: its own pixels of the
    mask conduct, and the pixels of the one-pixel ring around it that the previous launch's state holds are seeds only.
    -> (the state when a launch changes nothing, the launches run, that last one included)."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    th, tw = tile
    state = np.asarray(marker, bool) & mask
    launches = 0
    while True:
        launches += 1
        prev = np.pad(state, 1)
        gpad = np.pad(mask, 1)
        nxt = state.copy()
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                y1, x1 = min(y0 + th, h), min(x0 + tw, w)
                s = prev[y0:y1 + 2, x0:x1 + 2].copy()          # the tile and its ring, in padded coordinates
                if mutant == "halo_wrong_row":                  # the side columns of the ring come from the row below
                    s[:-1, 0], s[:-1, -1] = prev[y0 + 1:y1 + 2, x0], prev[y0 + 1:y1 + 2, x1 + 1]
                core = np.zeros(s.shape, bool)
                core[1:-1, 1:-1] = True
                if mutant == "no_tile_carry":
                    s &= core
                g = (gpad[y0:y1 + 2, x0:x1 + 2] & core) | (s & ~core)
                nxt[y0:y1, x0:x1] = propagate(s, g, c)[1:-1, 1:-1]
        if np.array_equal(nxt, state) or (mutant == "first_chunk_only" and launches == 4):
            return nxt, launches
        state = nxt


# ---- the maps the CPU and the GPU tests share ---------------------------------------------------------------------------------
def zigzag(h, w):
    """Every second column, consecutive columns joined alternately at the bottom and at the top row: one long path."""
    a = np.zeros((h, w), bool)
    a[:, 0::2] = True
    cols = np.arange(1, w - 1, 2)
    a[h - 1, cols[0::2]] = True
    a[0, cols[1::2]] = True
    return a


def diamond():
    """The 7 x 7 ring closed only by diagonal steps."""
    a = np.zeros((7, 7), bool)
    for i in range(4):
        a[3 - i, i] = a[3 + i, i] = a[3 - i, 6 - i] = a[3 + i, 6 - i] = True
    return a


def first_pixel(px):
    """The marker that holds the first set pixel of bool [h, w] in raster order."""
    m = np.zeros_like(px)
    if px.any():
        m.reshape(-1)[np.flatnonzero(px)[0]] = True
    return m


def designed(name):
    """name -> dict(marker bool [n, h, w] or None, mask bool [n, h, w], op, c, slip: the mutant that changes it, dirty: the
    pad bits of the packed inputs are set).  Each map is named for the slip it catches."""
    z = lambda h, w, n=1: np.zeros((n, h, w), bool)
    d = dict(op=SEEDED, c=4, dirty=False)
    if name == "diagonal_line":            # 8-steps taken at c = 4
        mask = z(20, 30)
        mask[0, np.arange(20), np.arange(20) + 3] = True
        d.update(mask=mask, marker=first_pixel(mask[0])[None], slip="eight_at_4")
    elif name == "diamond_ring":           # the background given the same connectivity as the foreground
        mask = np.zeros((1, 11, 13), bool)
        mask[0, 2:9, 3:10] = diamond()
        d.update(mask=mask, marker=None, op=FILL_HOLES, c=8, slip="same_connectivity")
    elif name == "pad_bridge":             # pad bits conduct: two bars joined only through columns >= w of a dirty input
        mask = z(9, 13)
        mask[0, 2, 5:] = mask[0, 4, 5:] = True   # both end at column 12; the set pad bits of rows 2 .. 4 would join them
        marker = z(9, 13)
        marker[0, 2, 5] = True
        d.update(mask=mask, marker=marker, dirty=True, slip="pad_conducts")
    elif name == "row_wrap":               # a pixel at column w - 1 and one at column 0 of the next row
        mask = z(6, 21)
        mask[0, 2, 15:] = mask[0, 3, :6] = True
        d.update(mask=mask, marker=first_pixel(mask[0])[None], slip="rows_wrap")
    elif name == "frames_touch":           # the last row of frame f and the first of f + 1
        mask = z(7, 70, 3)
        mask[0, 4:, 30:40] = mask[1, :, 30:40] = mask[2, :3, 30:40] = True
        marker = z(7, 70, 3)
        marker[1, 3, 35] = True
        d.update(mask=mask, marker=marker, c=8, slip="frames_touch")
    elif name == "word_carry":             # a bar over columns 63 / 64
        mask = z(5, 130)
        mask[0, 2, 40:100] = True
        d.update(mask=mask, marker=first_pixel(mask[0])[None], slip="no_word_carry")
    elif name == "tile_carry":             # bars over columns 511 / 512 and rows 63 / 64
        mask = z(70, 530)
        mask[0, 10, 500:525] = mask[0, 60:68, 20] = True
        marker = z(70, 530)
        marker[0, 10, 500] = marker[0, 60, 20] = True
        d.update(mask=mask, marker=marker, slip="no_tile_carry")
    elif name == "halo_row":               # the halo word read from the wrong row: one-pixel-high bars across column 512
        mask = z(12, 530)                  # in a frame with nothing in the rows next to them, 4-connected
        mask[0, 3, 490:528] = mask[0, 8, 505:520] = True
        marker = z(12, 530)
        marker[0, 3, 490] = marker[0, 8, 519] = True
        d.update(mask=mask, marker=marker, slip="halo_wrong_row")
    elif name == "zigzag":                 # stopping after the first chunk of launches
        mask = zigzag(65, 40)[None]
        d.update(mask=mask, marker=first_pixel(mask[0])[None], slip="first_chunk_only")
    else:
        raise KeyError(name)
    return d


DESIGNED = ("diagonal_line", "diamond_ring", "pad_bridge", "row_wrap", "frames_touch", "word_carry", "tile_carry", "halo_row",
            "zigzag")


def blobs(h, w, seed, size=5, level=0.5):
    from scipy.ndimage import uniform_filter
    rng = np.random.default_rng(seed)
    return uniform_filter(rng.random((h, w)), size) > level
