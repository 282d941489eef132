"""Adversarial smoothed planes for the Sobel+NMS kernels: chosen (gx, gy) pairs at known pixels.

A 3x3 block of a plane fixes the Sobel gradient of its centre pixel, so a plane tiled with 3x3 blocks carries one
independent, chosen (gx, gy) pair per block.  The planes built here hold

* every pair reachable at an interior pixel from values in [0, 255] (``interior_reachable``), one block each;
* 2-wide / 2-tall bands of half-blocks along the four image borders, whose centres sit on column 0 / W-1 and row
  0 / H-1 and so go through the border formulas of the reference (column clamp for gx, dropped columns for gy,
  row clamp for gy, dropped rows for gx: src/utils.cpp:114-186).  They carry the critical-margin pairs (the
  magnitude's square root lies within 2 float32 ulps of an integer) and the bin-boundary pairs that each border
  formula can reach;
* a strip of ramps, whose neighbours along the bin direction have equal magnitudes (NMS is a strict ">").

The width is a multiple of 8 and of 3 plus the bands: the strips of the marching kernels (496 or 248 columns) are
crossed, and block centres land on every pixel-in-lane position 0-7.  Everything here is plain numpy; the GPU tests
compare the kernels with the oracle on these planes, tests/test_sobel_planes.py checks the construction itself.
"""
from __future__ import annotations

import functools

import numpy as np

VMAX = 255
LIM = 4 * VMAX  # |gx|, |gy| <= 1020
W = 4320        # = 8 * 540 = 3 * 1440
NB = (W - 4) // 3  # interior blocks per block row (columns 2 .. 3 * NB + 1; then two filler columns, the right band)
N_PLANES = 2
RAMP_ROWS = 48
RAMP_SIZE = 24


def interior_reachable(gx, gy, vmax: int = VMAX):
    """Whether (gx, gy) is the gradient of some 3x3 block with values in [0, vmax] at an interior pixel.

    With the corners a (top left), c, g, i and the edge cells b (top), d, f, h:  gx = (c-a) + (i-g) + 2(f-d) and
    gy = (g-a) + (i-c) + 2(h-b).  Put p = i-a, q = c-g (so the corners add (p+q, p-q)), u = f-d, v = h-b, each in
    [-vmax, vmax]; s = p+q and d = p-q have the same parity and |s| + |d| <= 2 vmax.  So gx and gy have the same parity,
    and the smallest |s| (|d|) that leaves gx - s (gy - d) even and within +-2 vmax must fit into that sum."""
    gx, gy = np.abs(np.asarray(gx, np.int64)), np.abs(np.asarray(gy, np.int64))
    smin = np.maximum(gx - 2 * vmax, gx % 2)
    dmin = np.maximum(gy - 2 * vmax, gy % 2)
    return ((gx - gy) % 2 == 0) & (smin + dmin <= 2 * vmax) & (gx <= 4 * vmax) & (gy <= 4 * vmax)


def interior_blocks(gx, gy, vmax: int = VMAX) -> np.ndarray:
    """3x3 blocks (uint8, [n, 3, 3]) whose centre has gradient (gx, gy); every pair must be interior_reachable."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    assert interior_reachable(gx, gy, vmax).all()
    s = np.where(np.abs(gx) > 2 * vmax, np.sign(gx) * (np.abs(gx) - 2 * vmax), np.abs(gx) % 2)
    d = np.where(np.abs(gy) > 2 * vmax, np.sign(gy) * (np.abs(gy) - 2 * vmax), np.abs(gy) % 2)
    p, q, u, v = (s + d) // 2, (s - d) // 2, (gx - s) // 2, (gy - d) // 2
    a = np.maximum(0, -p)
    i = a + p
    g = np.maximum(0, -q)
    c = g + q
    dd = np.maximum(0, -u)
    f = dd + u
    b = np.maximum(0, -v)
    h = b + v
    e = (a + i + c + g) // 4  # the centre value does not enter its own gradient
    blk = np.stack([np.stack([a, b, c], -1), np.stack([dd, e, f], -1), np.stack([g, h, i], -1)], 1)
    assert blk.min() >= 0 and blk.max() <= vmax
    return blk.astype(np.uint8)


def left_band_blocks(gx, gy, vmax: int = VMAX):
    """Half-blocks for a pixel in column 0 (rows r-1..r+1, columns 0..1): values (a, b) / (c, d) / (e, f) give
    gx = (b-a) + 2(d-c) + (f-e) (column clamp) and gy = 2(e-a) + (f-b) (column -1 dropped).  Returns
    ([n, 3, 2] uint8, ok); rows where ok is False are zero: no half-block has that gradient."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    n = gx.size
    out = np.zeros((n, 3, 2), np.int64)
    ok = np.zeros(n, bool)
    for beta in range(-vmax, vmax + 1):  # beta = f - b, alpha = e - a
        todo = ~ok & ((gy - beta) % 2 == 0)
        alpha = (gy - beta) // 2
        todo &= np.abs(alpha) <= vmax
        # t = b - a: gx = 2t + beta - alpha + 2w with w = d - c in [-vmax, vmax]
        todo &= (gx - beta + alpha) % 2 == 0
        amin, amax = np.maximum(0, -alpha), np.minimum(vmax, vmax - alpha)
        bmin, bmax = max(0, -beta), min(vmax, vmax - beta)
        tmin, tmax = bmin - amax, bmax - amin
        half = (gx - beta + alpha) // 2
        t = np.clip(half, tmin, tmax)
        w = half - t
        todo &= np.abs(w) <= vmax
        if not todo.any():
            continue
        a = np.maximum(amin, bmin - t)
        b = a + t
        e, f = a + alpha, b + beta
        c = np.maximum(0, -w)
        d = c + w
        blk = np.stack([np.stack([a, b], -1), np.stack([c, d], -1), np.stack([e, f], -1)], 1)
        out[todo] = blk[todo]
        ok |= todo
    assert out.min() >= 0 and out.max() <= vmax
    return out.astype(np.uint8), ok


def border_blocks(kind: str, gx, gy, vmax: int = VMAX):
    """Half-blocks for a pixel on one border.  kind: "left" ([n, 3, 2], centre (1, 0)), "right" ([n, 3, 2], centre
    (1, 1)), "top" ([n, 2, 3], centre (0, 1)), "bottom" ([n, 2, 3], centre (1, 1)).  The right band is the left one
    mirrored (gx changes sign), the top band the left one transposed (the border rules swap with the axes)."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    if kind == "left":
        return left_band_blocks(gx, gy, vmax)
    if kind == "right":
        blk, ok = left_band_blocks(-gx, gy, vmax)
        return blk[:, :, ::-1], ok
    if kind == "top":
        blk, ok = left_band_blocks(gy, gx, vmax)
        return blk.transpose(0, 2, 1), ok
    if kind == "bottom":
        blk, ok = left_band_blocks(-gy, gx, vmax)
        return blk.transpose(0, 2, 1)[:, ::-1, :], ok
    raise ValueError(kind)


def _grid(lim: int = LIM):
    g = np.arange(-lim, lim + 1, dtype=np.int64)
    gx, gy = np.meshgrid(g, g)
    return gx.ravel(), gy.ravel()


def critical_pairs(lim: int = LIM):
    """Every (gx, gy) in [-lim, lim]^2 whose sqrt(n + 1/2), n = gx^2 + gy^2, lies within 2 float32 ulps of an integer:
    where v_sqrt_f32's error margin is smallest (n = k^2 - 1 and k^2, k > 1024)."""
    gx, gy = _grid(lim)
    r = np.sqrt((gx * gx + gy * gy).astype(np.float64) + 0.5)
    ulp = np.spacing(r.astype(np.float32)).astype(np.float64)
    sel = np.abs(r - np.rint(r)) <= 2 * ulp
    return gx[sel], gy[sel]


def bin_boundary_pairs(lim: int = LIM):
    """Pairs at the bin boundaries: 2|P| - (A-B) or 2|P| - (B-A) in {-1, 0, 1} (A = gx^2, B = gy^2, P = gx gy), plus
    the axes gx = 0, gy = 0 and the diagonals |gx| = |gy|."""
    gx, gy = _grid(lim)
    A, B, P2 = gx * gx, gy * gy, 2 * np.abs(gx * gy)
    sel = (np.abs(P2 - (A - B)) <= 1) | (np.abs(P2 - (B - A)) <= 1) | (gx == 0) | (gy == 0) | (np.abs(gx) == np.abs(gy))
    return gx[sel], gy[sel]


def _ramp_strip(width: int) -> np.ndarray:
    """RAMP_ROWS rows of RAMP_SIZE^2 ramp patches: slopes 1..5 along x, y, x+y and x-y, rising and falling; inside a
    patch every pixel's neighbours along its bin direction have its own magnitude."""
    yy, xx = np.mgrid[0:RAMP_SIZE, 0:RAMP_SIZE]
    kinds = []
    for slope in range(1, 6):
        for base in (xx, yy, xx + yy, xx - yy + RAMP_SIZE - 1):
            for sign in (1, -1):
                r = slope * base
                r = r if sign > 0 else r.max() - r
                kinds.append(r + (255 - r.max()) // 2)
    strip = np.zeros((RAMP_ROWS, width), np.int64)
    k = 0
    for y0 in range(0, RAMP_ROWS - RAMP_SIZE + 1, RAMP_SIZE):
        for x0 in range(0, width - RAMP_SIZE + 1, RAMP_SIZE):
            strip[y0:y0 + RAMP_SIZE, x0:x0 + RAMP_SIZE] = kinds[k % len(kinds)]
            k += 1
    assert strip.min() >= 0 and strip.max() <= 255
    return strip


@functools.lru_cache(maxsize=1)
def build():
    """The planes and where their chosen pairs sit.

    Returns a dict: ``planes`` uint8 [N_PLANES, H, W]; ``centres``: int64 [m, 5] rows (plane, row, col, gx, gy) of
    every chosen pixel; ``kind``: per centre 0 = interior, 1 = border band; ``critical``: per centre, whether the pair
    is a critical-margin pair; ``n_interior`` the number of interior-reachable pairs (each placed once)."""
    gx_all, gy_all = _grid()
    sel = interior_reachable(gx_all, gy_all)
    igx, igy = gx_all[sel], gy_all[sel]
    n_int = igx.size
    order = np.random.default_rng(20261016).permutation(n_int)  # neighbouring blocks: unrelated gradients
    igx, igy = igx[order], igy[order]
    rows_per_plane = -(-n_int // (NB * N_PLANES))  # block rows
    H = 2 + 3 * rows_per_plane + RAMP_ROWS + 2
    planes = np.zeros((N_PLANES, H, W), np.uint8)
    centres, kinds = [], []

    # interior blocks: plane-major, then block rows, then block columns
    slots = N_PLANES * rows_per_plane * NB
    pad = slots - n_int  # the last slots repeat the first pairs
    bgx, bgy = np.concatenate([igx, igx[:pad]]), np.concatenate([igy, igy[:pad]])
    blocks = interior_blocks(bgx, bgy).reshape(N_PLANES, rows_per_plane, NB, 3, 3)
    planes[:, 2:2 + 3 * rows_per_plane, 2:2 + 3 * NB] = blocks.transpose(0, 1, 3, 2, 4).reshape(
        N_PLANES, 3 * rows_per_plane, 3 * NB)
    pl, br, bc = np.meshgrid(np.arange(N_PLANES), np.arange(rows_per_plane), np.arange(NB), indexing="ij")
    centres.append(np.stack([pl.ravel(), 3 + 3 * br.ravel(), 3 + 3 * bc.ravel(), bgx, bgy], 1))
    kinds.append(np.zeros(slots, np.int64))

    # ramps below the blocks
    planes[:, 2 + 3 * rows_per_plane:2 + 3 * rows_per_plane + RAMP_ROWS, 2:W - 2] = _ramp_strip(W - 4)

    # border bands: critical pairs first, then bin-boundary pairs, each dealt to the bands whose formula reaches it
    cgx, cgy = critical_pairs()
    bgx2, bgy2 = bin_boundary_pairs()
    crit_set = set(zip(cgx.tolist(), cgy.tolist()))
    also_crit = np.array([(x, y) in crit_set for x, y in zip(bgx2.tolist(), bgy2.tolist())], bool)
    cand_gx = np.concatenate([cgx, bgx2[~also_crit]])
    cand_gy = np.concatenate([cgy, bgy2[~also_crit]])
    bands = {  # kind -> (slot centres (row, col) of one plane, slot origins (row, col) of the half-block)
        "top": [(0, 3 + 3 * j, 0, 2 + 3 * j) for j in range(NB)],
        "bottom": [(H - 1, 3 + 3 * j, H - 2, 2 + 3 * j) for j in range(NB)],
        "left": [(3 + 3 * k, 0, 2 + 3 * k, 0) for k in range(rows_per_plane)],
        "right": [(3 + 3 * k, W - 1, 2 + 3 * k, W - 2) for k in range(rows_per_plane)],
    }
    oks = {kind: border_blocks(kind, cand_gx, cand_gy) for kind in bands}
    used = {kind: 0 for kind in bands}
    cap = {kind: N_PLANES * len(s) for kind, s in bands.items()}
    band_rows = []
    for idx in range(cand_gx.size):
        # the band with the most room left among those that reach the pair (a pair is placed once)
        best = max((k for k in bands if oks[k][1][idx] and used[k] < cap[k]), key=lambda k: cap[k] - used[k],
                   default=None)
        if best is None:
            continue
        slot = used[best]
        used[best] += 1
        p, s = divmod(slot, len(bands[best]))
        cy, cx, oy, ox = bands[best][s]
        blk = oks[best][0][idx]
        planes[p, oy:oy + blk.shape[0], ox:ox + blk.shape[1]] = blk
        band_rows.append((p, cy, cx, cand_gx[idx], cand_gy[idx]))
    centres.append(np.array(band_rows, np.int64).reshape(-1, 5))
    kinds.append(np.ones(len(band_rows), np.int64))

    centres = np.concatenate(centres)
    crit = np.array([(int(x), int(y)) in crit_set for x, y in centres[:, 3:5]], bool)
    return {"planes": planes, "centres": centres, "kind": np.concatenate(kinds), "critical": crit,
            "n_interior": n_int, "band_use": dict(used), "band_capacity": cap}
