"""Designed candidate maps for the stage hysteresis kernels, and a numpy model of the tile sweeps that can slip.

The propagation code (load_tile / process_tile_with in canny_kernels.hip) is case analysis: nine halo words, four
straight pulls, four diagonal entries through the side borders, four corner pixels, the (1,0) -> (0,1) quirk mask, the
carry-chain row flood and eight guarded pushes.  A random candidate plane offers every link a second path, so a missing
one stays hidden.  The maps here are built so that ONE link carries everything behind it; tests/test_hyst_maps.py shows on
the CPU that each map is that sharp (the model below, made to slip in one line, changes a named frame), and
tests/test_gpu_hyst_maps.py sends the same batches through the kernels.

Model.  model_sweeps() restates the device's scheme on boolean planes in the device's tile numbering
(t = (frame * tiles_y + ty) * tiles_x + tx, neighbours at t + dy * tiles_x + dx): every tile of a sweep sees the planes as
the previous sweep left them, floods to its fixed point with the kernel's round (3x3 pull with the halo, then fill_runs)
and schedules the neighbours its changed border faces.  The device may be quicker than the model (a tile can see what a
neighbour stored in the same sweep) but not slower.

What a slip of the fill cannot show.  A round's `nb` already holds d << 1 and d >> 1, so a row flood that fills one
direction only (or nothing) reaches the same fixed point a few rounds later: "fill_up_only" and "fill_down_only" never
change a map, on the model or on the device.  They are kept in SLIPS and checked where they can be seen, on one
application of fill_runs (tests/test_hyst_maps.py); the two slips of the same lines that do change maps are the dropped
`& p` of either direction ("fill_up_nomask", "fill_down_nomask": the carry lands in the zero beyond the run and leaks).

Values: weak 60, strong 200, thresholds 50 / 150 unless a builder says otherwise.
"""
import heapq

import numpy as np

T = 64
LO, HI = 50, 150
WEAK, STRONG = 60, 200

PULLS = ("su", "sd", "lb", "rb")
SIDE_DIAGONALS = ("lb_up", "lb_dn", "rb_up", "rb_dn")
CORNERS = ("ul", "ur", "dl", "dr")
# lane k of the push block takes neighbour PUSH_DIRS[k]: up, down, left, right, then the four corners
PUSH_DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
SLIPS = (tuple("pull_" + p for p in PULLS + SIDE_DIAGONALS + CORNERS) + ("lb_up_lane0_shuffled",)
         + tuple(f"push_{k}" for k in range(8))
         + ("quirk_absent", "quirk_tile_row_0", "quirk_tile_col_0", "quirk_frame_0_only")
         + ("fill_up_only", "fill_down_only", "fill_up_nomask", "fill_down_nomask")
         + ("frame_guard_vertical", "frame_guard_row_end"))
FILL_SLIPS = ("fill_up_only", "fill_down_only", "fill_up_nomask", "fill_down_nomask")
INVISIBLE_SLIPS = ("fill_up_only", "fill_down_only")  # see the module docstring


# ---- the model ------------------------------------------------------------------------------------------------------
def _pack(b):
    """bool [..., 64] -> uint64 [...], bit k = column k (the device's word layout)."""
    return np.packbits(b, axis=-1, bitorder="little").view("<u8")[..., 0]


def _unpack(w):
    return np.unpackbits(np.ascontiguousarray(w)[..., None].view(np.uint8), axis=-1, bitorder="little").astype(bool)


def fill_runs(p, g, slip=None):
    """fill_runs of canny_kernels.hip on bool rows [..., 64]: every run of p that holds a bit of g, through the carry
    chain of p + g in either direction."""
    P, G = _pack(p), _pack(g)
    Pr, Gr = _pack(p[..., ::-1]), _pack(g[..., ::-1])
    up = (P + G) ^ P
    down = (Pr + Gr) ^ Pr
    if slip != "fill_up_nomask":
        up &= P
    if slip != "fill_down_nomask":
        down &= Pr
    out = g.copy()
    if slip != "fill_down_only":
        out |= _unpack(up)
    if slip != "fill_up_only":
        out |= _unpack(down)[..., ::-1]
    return out


def _to_tiles(plane):
    """bool [n, H, W] -> [n * ty * tx, 64, 64], padded with False, in the device's tile order."""
    n, h, w = plane.shape
    ty, tx = -(-h // T), -(-w // T)
    pad = np.zeros((n, ty * T, tx * T), bool)
    pad[:, :h, :w] = plane
    return np.ascontiguousarray(pad.reshape(n, ty, T, tx, T).transpose(0, 1, 3, 2, 4)).reshape(n * ty * tx, T, T)


def _from_tiles(tiles, n, h, w):
    ty, tx = -(-h // T), -(-w // T)
    return tiles.reshape(n, ty, tx, T, T).transpose(0, 1, 3, 2, 4).reshape(n, ty * T, tx * T)[:, :h, :w]


def model_sweeps(cand, lo=LO, hi=HI, slip=None):
    """The synchronous tile model on a candidate plane [H, W] or batch [n, H, W].  Returns (edge map as the device
    writes it -- int16, 255 where reached, 0 elsewhere, all 0 if hi > 255 --, sweeps run, the last one, which
    schedules nothing, included).  slip: one of SLIPS, a mistake made on purpose."""
    assert slip is None or slip in SLIPS, slip
    cand = np.asarray(cand)
    single = cand.ndim == 2
    if single:
        cand = cand[None]
    n, h, w = cand.shape
    ty_n, tx_n = -(-h // T), -(-w // T)
    tiles = n * ty_n * tx_n
    C = _to_tiles(cand >= lo)
    S = _to_tiles((cand >= lo) & (cand >= hi))
    todo = np.arange(tiles)
    sweeps = 0
    while todo.size:
        before = S
        S = S.copy()
        t = todo
        k = t.size
        tt = t % (ty_n * tx_n)
        f, ty, tx = t // (ty_n * tx_n), tt // tx_n, tt % tx_n
        has_u, has_d, has_l, has_r = ty > 0, ty < ty_n - 1, tx > 0, tx < tx_n - 1
        if slip == "frame_guard_vertical":   # tile numbering alone decides what lies above and below
            has_u, has_d = t - tx_n >= 0, t + tx_n < tiles
        if slip == "frame_guard_row_end":    # ... and what lies left and right
            has_l, has_r = t - 1 >= 0, t + 1 < tiles

        def halo(ok, dt, pick):
            """pick(before[t + dt]) where ok, zeros elsewhere."""
            src = np.clip(t + dt, 0, tiles - 1)
            v = pick(before[src])
            return np.where(ok.reshape((k,) + (1,) * (v.ndim - 1)), v, False)

        su = halo(has_u, -tx_n, lambda a: a[:, T - 1, :])
        sd = halo(has_d, tx_n, lambda a: a[:, 0, :])
        lb = halo(has_l, -1, lambda a: a[:, :, T - 1])
        rb = halo(has_r, 1, lambda a: a[:, :, 0])
        ul = halo(has_u & has_l, -tx_n - 1, lambda a: a[:, T - 1, T - 1])
        ur = halo(has_u & has_r, -tx_n + 1, lambda a: a[:, T - 1, 0])
        dl = halo(has_d & has_l, tx_n - 1, lambda a: a[:, 0, T - 1])
        dr = halo(has_d & has_r, tx_n + 1, lambda a: a[:, 0, 0])
        zero_row, zero_col, zero_px = np.zeros_like(su), np.zeros_like(lb), np.zeros_like(ul)
        if slip == "pull_su": su = zero_row
        if slip == "pull_sd": sd = zero_row
        if slip == "pull_ul": ul = zero_px
        if slip == "pull_ur": ur = zero_px
        if slip == "pull_dl": dl = zero_px
        if slip == "pull_dr": dr = zero_px
        lb_up = np.concatenate([ul[:, None], lb[:, :-1]], axis=1)   # lane r: the left tile's row r - 1
        lb_dn = np.concatenate([lb[:, 1:], dl[:, None]], axis=1)
        rb_up = np.concatenate([ur[:, None], rb[:, :-1]], axis=1)
        rb_dn = np.concatenate([rb[:, 1:], dr[:, None]], axis=1)
        if slip == "lb_up_lane0_shuffled": lb_up[:, 0] = lb[:, 0]   # a shuffle from lane -1 returns the lane's own
        if slip == "pull_lb": lb = zero_col
        if slip == "pull_rb": rb = zero_col
        if slip == "pull_lb_up": lb_up = zero_col
        if slip == "pull_lb_dn": lb_dn = zero_col
        if slip == "pull_rb_up": rb_up = zero_col
        if slip == "pull_rb_dn": rb_dn = zero_col
        in_left, in_right = lb | lb_up | lb_dn, rb | rb_up | rb_dn
        quirk = (ty == 0) & (tx == 0)
        if slip == "quirk_absent": quirk = np.zeros(k, bool)
        if slip == "quirk_tile_row_0": quirk = ty == 0
        if slip == "quirk_tile_col_0": quirk = tx == 0
        if slip == "quirk_frame_0_only": quirk = t == 0

        c, s0 = C[t], before[t]
        s = s0.copy()
        live = np.arange(k)   # tiles whose last round still added something
        while live.size:
            sl, cl = s[live], c[live]
            up = np.concatenate([su[live][:, None, :], sl[:, :-1, :]], axis=1)
            dn = np.concatenate([sl[:, 1:, :], sd[live][:, None, :]], axis=1)
            d = up | sl | dn
            dfl = d.copy()   # what column x may pull from column x - 1
            q = quirk[live]
            dfl[q, 0, 0] = up[q, 0, 0] | sl[q, 0, 0]
            nb = d.copy()
            nb[:, :, 1:] |= dfl[:, :, :-1]
            nb[:, :, :-1] |= d[:, :, 1:]
            nb[:, :, 0] |= in_left[live]
            nb[:, :, T - 1] |= in_right[live]
            gsel = sl | (cl & nb)
            grew = (gsel != sl).any(axis=(1, 2))
            if not grew.any():
                break
            live = live[grew]
            s[live] = fill_runs(cl[grew], gsel[grew], slip if slip in FILL_SLIPS else None)

        chg = s & ~s0
        changed = chg.any(axis=(1, 2))
        S[t[changed]] = s[changed]
        top, bot, lef, rig = chg[:, 0, :], chg[:, T - 1, :], chg[:, :, 0], chg[:, :, T - 1]
        hits = (top.any(1), bot.any(1), lef.any(1), rig.any(1), top[:, 0], top[:, T - 1], bot[:, 0], bot[:, T - 1])
        nxt = []
        for lane, ((dy, dx), hit) in enumerate(zip(PUSH_DIRS, hits)):
            if slip == f"push_{lane}":
                continue
            there = (has_u if dy < 0 else has_d if dy > 0 else True) & (has_l if dx < 0 else has_r if dx > 0 else True)
            nb_t = t + dy * tx_n + dx
            nxt.append(nb_t[changed & hit & there & (nb_t >= 0) & (nb_t < tiles)])
        todo = np.unique(np.concatenate(nxt))
        sweeps += 1
    out = _from_tiles(S, n, h, w).astype(np.int16) * (255 if hi <= 255 else 0)
    return (out[0] if single else out), sweeps


def earliest_sweep(cand, lo=LO, hi=HI):
    """For one frame: a lower bound, for every connectable pixel, on the sweep in which ANY schedule of the tiles can
    set it (-1: strong from the start; unreachable pixels keep a large number).  A tile runs at most once per sweep, so
    along a path from a strong pixel the tiles entered within one sweep are all different; the bound is the least
    number of times a path has to start a new sweep because it enters a tile it has used in the current one.  (The
    quirk's missing link is ignored: more links only lower the bound.)"""
    cand = np.asarray(cand)
    h, w = cand.shape
    conn = cand >= lo
    best = {}
    heap = []
    for y, x in zip(*np.nonzero(conn & (cand >= hi))):
        state = (int(y), int(x), frozenset([(int(y) // T, int(x) // T)]))
        best[state] = -1
        heap.append((-1, state[0], state[1], tuple(sorted(state[2]))))
    heapq.heapify(heap)
    out = np.full((h, w), 1 << 30, np.int64)
    while heap:
        cost, y, x, used = heapq.heappop(heap)
        used = frozenset(used)
        if best.get((y, x, used), 1 << 30) < cost:
            continue
        out[y, x] = min(out[y, x], cost)
        here = (y // T, x // T)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                py, px = y + dy, x + dx
                if (dy or dx) and 0 <= py < h and 0 <= px < w and conn[py, px]:
                    tile = (py // T, px // T)
                    if tile == here:
                        nc, nu = cost, used
                    elif tile not in used:
                        nc, nu = cost, used | {tile}
                    else:
                        nc, nu = cost + 1, frozenset([tile])
                    nc = max(nc, 0)   # a pixel that is not strong is set by a sweep: 0 at the earliest
                    if nc < best.get((py, px, nu), 1 << 30):
                        best[(py, px, nu)] = nc
                        heapq.heappush(heap, (nc, py, px, tuple(sorted(nu))))
    return out


# ---- drawing --------------------------------------------------------------------------------------------------------
def _walk(points):
    """The pixels of a polyline whose legs are horizontal, vertical or diagonal."""
    out = [tuple(points[0])]
    for (y0, x0), (y1, x1) in zip(points, points[1:]):
        steps = max(abs(y1 - y0), abs(x1 - x0))
        assert abs(y1 - y0) in (0, steps) and abs(x1 - x0) in (0, steps), (points, "leg is not straight")
        for i in range(1, steps + 1):
            out.append((y0 + (y1 - y0) * i // steps, x0 + (x1 - x0) * i // steps))
    return out


def _draw(frame, points, value=WEAK):
    for y, x in _walk(points):
        frame[y, x] = value


# ---- link atlas -----------------------------------------------------------------------------------------------------
LINK_SHAPES = ((192, 192), (190, 189))   # classify8 + rows finalize / generic kernels with a partial last tile row, column
LINK_LANES = (0, 31, 32, 63)             # receiving positions along the border (closed under the flips used below)


def _link_case_from_above(x, dx):
    """192 x 192 canvas, 3 x 3 tiles.  The far pixels (64..66, 64 + x) of the centre tile hang on the link pixel
    (63, 64 + x + dx) of the tile above (dx = 0: straight, +-1: diagonal; at the ends of the border the link pixel lies
    in a corner tile).  The link pixel is fed through a delay line: a serpentine on rows 4, 6, 8, 10 that straddles a
    vertical tile border away from the link and crosses it four times, seeded at its far end."""
    frame = np.zeros((192, 192), np.int16)
    link_x = 64 + x + dx
    sx = link_x // T   # the source tile is (0, sx)
    if sx == 0:
        b, side = 63, +1     # partner (0, 1), source-side columns b - 2 .. b
    elif sx == 2:
        b, side = 127, -1    # partner (0, 1), source-side columns b + 1 .. b + 3
    elif link_x < 96:
        b, side = 127, +1    # partner (0, 2)
    else:
        b, side = 63, -1     # partner (0, 0)
    near, far = (b - 2, b + 3) if side > 0 else (b + 3, b - 2)   # column ends: in the source tile / in the partner
    _draw(frame, [(4, near), (4, far), (6, far), (6, near), (8, near), (8, far), (10, far), (10, near)])
    _draw(frame, [(10, near), (40, near), (40, link_x), (63, link_x)])
    dest = (64, 64 + x)
    _draw(frame, [dest, (66, 64 + x)])
    frame[4, near] = STRONG
    return frame, {"seed": (4, near), "link": (63, link_x), "dest": dest, "far": [(64, 64 + x), (65, 64 + x), (66, 64 + x)]}


def _transform(frame, meta, how):
    def pt(p):
        y, x = p
        if how in ("down", "right"):
            y = 191 - y
        if how in ("left", "right"):
            y, x = x, y
        return (y, x)
    f = frame
    if how in ("down", "right"):
        f = f[::-1]
    if how in ("left", "right"):
        f = f.T
    m = {k: ([pt(p) for p in v] if isinstance(v, list) else pt(v)) for k, v in meta.items()}
    return np.ascontiguousarray(f), m


def link_atlas(shape):
    """Every crossing into the centre tile (1, 1): from above, below, left and right at lanes 0, 31, 32 and 63, straight
    and in both diagonal forms, the four corners among them.  Returns (batch [n, H, W], list of dicts with seed, link,
    dest, far, name).  Built on 192 x 192 and cut to `shape`: every designed pixel lies in [3, 188]^2."""
    frames, metas, seen = [], [], set()
    for how in ("up", "down", "left", "right"):
        for x in LINK_LANES:
            for dx in (-1, 0, 1):
                frame, meta = _link_case_from_above(x, dx)
                frame, meta = _transform(frame, meta, how)
                if (meta["link"], meta["dest"]) in seen:   # the corner cases come round twice
                    continue
                seen.add((meta["link"], meta["dest"]))
                ys, xs = np.nonzero(frame)
                assert ys.min() >= 3 and xs.min() >= 3 and ys.max() <= 188 and xs.max() <= 188
                ly, lx = meta["link"]
                meta["name"] = f"link from tile ({ly // T},{lx // T}) pixel {meta['link']} to {meta['dest']}"
                frames.append(frame[:shape[0], :shape[1]])
                metas.append(meta)
    return np.stack(frames), metas


# ---- row-flood atlas ------------------------------------------------------------------------------------------------
def _row_frame(width, runs, seeds):
    row = np.zeros((1, width), np.int16)
    for s, e in runs:
        row[0, s:e + 1] = WEAK
    for x in seeds:
        row[0, x] = STRONG
    return row


def row_atlas():
    """1 x 64 frames: every run [s, e] seeded at its first, last and middle pixel (6,049 frames, the full word seeded at
    bit 0 and at bit 63 among them)."""
    frames = []
    for s in range(T):
        for e in range(s, T):
            for seed in sorted({s, e, (s + e) // 2}):
                frames.append(_row_frame(T, [(s, e)], [seed]))
    return np.stack(frames)


def row_gap_atlas():
    """1 x 64 frames with two and three runs separated by ONE zero, seeded in one run only: a carry must not leak."""
    frames = []
    for k in range(1, T - 1):   # runs [0, k-1] and [k+1, 63]
        for seed in sorted({0, k - 1}):
            frames.append(_row_frame(T, [(0, k - 1), (k + 1, T - 1)], [seed]))
        for seed in sorted({k + 1, T - 1}):
            frames.append(_row_frame(T, [(0, k - 1), (k + 1, T - 1)], [seed]))
    for a in (1, 2, 20, 31):
        for b in (a + 2, 33, 40, 62):
            runs = [(0, a - 1), (a + 1, b - 1), (b + 1, T - 1)]
            for which, (s, e) in enumerate(runs):
                for seed in sorted({s, e, (s + e) // 2}):
                    frames.append(_row_frame(T, runs, [seed]))
    return np.stack(frames)


def row_wide_atlas():
    """1 x 130 frames (three words, the last two pixels wide) whose run spans the word boundaries, seeded at either end."""
    frames = []
    for s, e in ((60, 70), (63, 64), (0, 129), (1, 128), (62, 129), (0, 65), (127, 128), (64, 127), (126, 129)):
        for seed in (s, e):
            frames.append(_row_frame(130, [(s, e)], [seed]))
    for runs, seed in (([(0, 62), (64, 129)], 62), ([(0, 62), (64, 129)], 64), ([(0, 63), (65, 126), (128, 129)], 65),
                       ([(0, 63), (65, 126), (128, 129)], 126)):
        frames.append(_row_frame(130, runs, [seed]))
    return np.stack(frames)


# ---- inside one tile ------------------------------------------------------------------------------------------------
def in_tile_atlas():
    """64 x 64 frames: one-pixel diagonal staircases (one row per round of the tile's loop) in both directions and
    seeded at either end, a square spiral seeded outside and inside, a vertical serpentine seeded at either end."""
    frames, names = [], []
    for pts, name in (([(0, 0), (63, 63)], "diagonal"), ([(0, 63), (63, 0)], "anti-diagonal")):
        for end in (0, 1):
            f = np.zeros((T, T), np.int16)
            _draw(f, pts)
            f[pts[end]] = STRONG
            frames.append(f)
            names.append(f"{name} seeded at {pts[end]}")
    spiral, lo_, hi_ = [(0, 0)], 0, T - 1
    while hi_ - lo_ >= 2:
        spiral += [(lo_, hi_), (hi_, hi_), (hi_, lo_), (lo_ + 2, lo_), (lo_ + 2, lo_ + 2)]
        lo_, hi_ = lo_ + 2, hi_ - 2
    serp = []
    for i, x in enumerate(range(0, T, 2)):
        serp += [(0, x), (T - 1, x)] if i % 2 == 0 else [(T - 1, x), (0, x)]
    for pts, name in ((spiral, "spiral"), (serp, "serpentine")):
        for end in (0, -1):
            f = np.zeros((T, T), np.int16)
            _draw(f, pts)
            f[pts[end]] = STRONG
            frames.append(f)
            names.append(f"{name} seeded at {pts[end]}")
    return np.stack(frames), names


# ---- zigzag ---------------------------------------------------------------------------------------------------------
def zigzag():
    """64 x 128: rows 0, 2, 4, ... each cross the column 63|64 border, joined alternately at column 67 and column 60,
    seed at (0, 60): 32 crossings, 16 re-entries of the start tile."""
    f = np.zeros((T, 2 * T), np.int16)
    pts = []
    for i, y in enumerate(range(0, T, 2)):
        pts += [(y, 60), (y, 67)] if i % 2 == 0 else [(y, 67), (y, 60)]
    _draw(f, pts)
    f[0, 60] = STRONG
    return f[None]


def reported_iterations_floor(cand, lo=LO, hi=HI):
    """Lower bound on last_hysteresis_iterations for a batch, from the maps alone.  The host reports hf[0] + 1
    (lane_wait), and hf[0] is the largest iter + 1 of a sweep that scheduled a tile.  A pixel that cannot be set before
    sweep e >= 1 is set by a tile that a sweep >= e - 1 scheduled, so hf[0] >= e and the report is at least e + 1; with no
    such pixel the report is at least 1."""
    e = 0
    for frame in cand:
        es = earliest_sweep(frame, lo, hi)
        reach = es < (1 << 30)
        if reach.any():
            e = max(e, int(es[reach].max()))
    return e + 1


# ---- quirk atlas ----------------------------------------------------------------------------------------------------
QUIRK_SHAPES = ((128, 128), (126, 125))
QUIRK_ORIGINS = ((0, 0), (0, 64), (64, 0), (64, 64))


def quirk_atlas(shape):
    """Twelve frames: frame f holds (oy+2, ox) = 200, (oy+1, ox) = 60, (oy, ox+1) = 60 at the origin of tile
    QUIRK_ORIGINS[f % 4].  At the image origin (0, 1) stays 0 -- in frames 0, 4 and 8 alike --, at every other tile
    origin it is promoted.  A thirteenth frame holds all four.  Metadata as for the link atlas (link = the weak
    pixel (oy+1, ox), far = [(oy, ox+1)])."""
    frames, metas = [], []
    for f in range(13):
        frame = np.zeros(shape, np.int16)
        for oy, ox in (QUIRK_ORIGINS if f == 12 else (QUIRK_ORIGINS[f % 4],)):
            frame[oy + 2, ox], frame[oy + 1, ox], frame[oy, ox + 1] = STRONG, WEAK, WEAK
        oy, ox = QUIRK_ORIGINS[f % 4]
        frames.append(frame)
        metas.append({"seed": (oy + 2, ox), "link": (oy + 1, ox), "dest": (oy, ox + 1), "far": [(oy, ox + 1)],
                      "name": f"quirk pattern at {'every tile origin' if f == 12 else (oy, ox)}, frame {f}"})
    return np.stack(frames), metas


# ---- frame isolation ------------------------------------------------------------------------------------------------
ISOLATION_SHAPES = ((128, 128), (126, 125))


def isolation_atlas(shape):
    """name -> (batch, indices of the frames that must come back empty).  Neighbouring frames and neighbouring tile rows
    are adjacent in the tile numbering and nowhere else:
      last_to_first   frames 0 and 2 strong along their last row and column, frame 1 weak along its first row and column
      first_to_last   the mirror image: frames 0 and 2 weak along the last, frame 1 strong along the first
      changing_row    frame 0's last row CHANGES (a strong pixel with a weak run, away from the corners) above two frames
                      of weak first rows: nothing may be scheduled at all
      row_end         one frame: strong at (r, W-1) in tile row 0, weak at (r + 64, 0)."""
    h, w = shape
    def edge_frame(last, value):
        f = np.zeros(shape, np.int16)
        f[h - 1 if last else 0, :] = value
        f[:, w - 1 if last else 0] = value
        return f
    out = {"last_to_first": (np.stack([edge_frame(True, STRONG), edge_frame(False, WEAK), edge_frame(True, STRONG)]), [1]),
           "first_to_last": (np.stack([edge_frame(True, WEAK), edge_frame(False, STRONG), edge_frame(True, WEAK)]), [0, 2])}
    e = np.zeros(shape, np.int16)
    e[h - 1, 10:21] = WEAK
    e[h - 1, 10] = STRONG
    out["changing_row"] = (np.stack([e, edge_frame(False, WEAK), edge_frame(False, WEAK)]), [1, 2])
    r = np.zeros(shape, np.int16)
    for row in (0, 31, 61):
        r[row, w - 1] = STRONG
        r[row + T, 0] = WEAK
    out["row_end"] = (r[None], [])
    return out


# ---- value atlas ----------------------------------------------------------------------------------------------------
VALUE_PAIRS = ((1, 2), (254, 255), (255, 255), (1, 300), (300, 32767), (1, 40000), (40000, 50000), (200, 100), (0, 255),
               (-3, 1), (300, 200))   # the last one is order dependent in the reference: lo > 255 >= hi
VALUE_WIDTHS = (64, 61)
ERR_DOMAIN = 5


def _s16(v):
    return int(np.clip(v, -32768, 32767))


def value_frames(lo, hi, width):
    """8 x width frames, two per value of (lo-1, lo, hi-1, hi, -32768, 32767) (cut to the short range): frame (v, half)
    holds v in rows 0, 2, 4, 6 at the columns with x % 8 == row + half, so the two frames put v at each of the 8 positions
    of an 8-pixel group, lanes 0 and 63 included, and 32767 right below each of them.  The rest is a value of the other
    class: lo-1 around connectable values, hi around the others."""
    frames = []
    for v in (lo - 1, lo, hi - 1, hi, -32768, 32767):
        v = _s16(v)
        for half in (0, 1):
            f = np.full((8, width), _s16(lo - 1) if v >= lo else _s16(hi), np.int16)
            for row in (0, 2, 4, 6):
                cols = np.arange(row + half, width, 8)
                f[row, cols] = v
                f[row + 1, cols] = 32767
            frames.append(f)
    return np.stack(frames)


def value_random(lo, hi, shape):
    """Three frames: two of full-range shorts, one of the six values above drawn at random."""
    rng = np.random.default_rng([lo + 65536, hi + 65536, shape[0], shape[1]])
    f = rng.integers(-32768, 32768, (3,) + shape).astype(np.int16)
    f[1] = rng.choice(np.array([_s16(lo - 1), _s16(lo), _s16(hi - 1), _s16(hi), -32768, 32767], np.int16), shape)
    return f


def value_in_domain(lo, hi, width):
    """Three 8 x width frames of values >= lo only (what a call with lo <= 0 accepts), and the same batch with lo - 1 in
    the last pixel of the last frame."""
    rng = np.random.default_rng([1000 + width, lo + 65536])
    f = rng.choice(np.array([_s16(lo), _s16(lo + 1), _s16(hi - 1), _s16(hi), 32767], np.int16), (3, 8, width))
    bad = f.copy()
    bad[-1, -1, -1] = _s16(lo - 1)
    return f, bad


def value_status(cand, lo, hi):
    """The status dev_hysteresis must return: CANNY_HIP_ERR_DOMAIN exactly where the reference's result depends on its
    scan order, 0 otherwise."""
    return ERR_DOMAIN if (lo <= 0 and bool((np.asarray(cand) < lo).any())) or (lo > 255 >= hi) else 0
