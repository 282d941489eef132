"""The launch plan of the warp and the tiled route's decision per tile (canny_hip_selftest_warp_plan) against a restatement of
DESIGN.md section 32, host-only.  The launcher takes its grid from the helper this entry reports and the kernel decides with
the function behind the tile query, so tests/test_gpu_warp.py can KNOW that a case sends a workgroup into its second trip and
that one frame holds staged and unstaged tiles."""
import numpy as np
import pytest

import warp_rule as wr
from canny_edge_amd import capi

CAP = 4096            # workgroups of the warp's launch
TILE_W, TILE_H = 64, 16
ONE = wr.ONE


def tiles(h, w):
    return -(-h // TILE_H) * -(-w // TILE_W)


@pytest.mark.parametrize("h,w", [(1, 1), (16, 64), (17, 65), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for n in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            p = capi.warp_plan(n, h, w)
            units = n * per
            what = f"n={n} {h} x {w}: {p}"
            assert (p.units, p.per_group, p.aux) == (units, 1, 0), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


def test_the_plan_refuses_what_the_warp_refuses():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (65536, 16, 64), (1, 32769, 64), (1, 16, 32769)):
        with pytest.raises(capi.CannyHipError):
            capi.warp_plan(*args)
    x = wr.record(wr.IDENTITY)
    for args in ((0, 50, 16, 64, 0, 0, 0), (50, 0, 16, 64, 0, 0, 0), (50, 50, 16, 64, 2, 0, 0), (50, 50, 16, 64, 0, 1, 0),
                 (50, 50, 16, 64, 0, 0, 1), (50, 50, 16, 64, 0, -1, 0), (50, 50, 16, 65, 0, 2, 0)):
        with pytest.raises(capi.CannyHipError):
            capi.warp_tile(x, *args)
    assert capi.warp_tile(x, 50, 100, 16, 65, 0, 1, 0).staged


def pitch(bw):
    return ((-(-bw // 4)) | 1) * 4


def footprint(coef, interp, src_h, src_w, out_h, out_w, tx, ty):
    """The bounding box of the taps of every pixel of the tile, from the rule pixel by pixel (not from the corners)."""
    x0, y0 = tx * TILE_W, ty * TILE_H
    ys, xs = np.mgrid[y0:min(y0 + TILE_H, out_h), x0:min(x0 + TILE_W, out_w)].astype(np.int64)
    a11, a12, t1, a21, a22, t2 = coef
    X, Y = a11 * xs + a12 * ys + t1, a21 * xs + a22 * ys + t2
    if interp == wr.NEAREST:
        sx, sy = (X + 32768) >> 16, (Y + 32768) >> 16
        lo, hi = (int(sx.min()), int(sy.min())), (int(sx.max()), int(sy.max()))
    else:
        ix, iy = (X + 128) >> 16, (Y + 128) >> 16
        lo, hi = (int(ix.min()), int(iy.min())), (int(ix.max()) + 1, int(iy.max()) + 1)
    return max(lo[0], 0), max(lo[1], 0), min(hi[0], src_w - 1), min(hi[1], src_h - 1)


CASES = {"identity": wr.IDENTITY, "shift": wr.shift(-6.977, -3.977), "quarter turn": wr.quarter_turn(300),
         "one degree": wr.small_turn(300, 200), "half scale": (2 * ONE, 0, 0, 0, 2 * ONE, 0),
         "scale 8": (8 * ONE, 0, 0, 0, 8 * ONE, 0), "shear": (ONE, ONE // 2, -20 * ONE, 0, ONE, 0),
         "mirror": (-ONE, 0, 299 * ONE, 0, ONE, 0), "leaving": wr.shift(270.5, 190.5), "outside": wr.shift(5000, 0)}


@pytest.mark.parametrize("interp", [wr.NEAREST, wr.BILINEAR])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_footprint_of_every_tile_bounds_its_taps_exactly(name, interp):
    """The corners' bounding box IS the pixels' bounding box (the map is affine, the tap index monotone), clipped to the source;
    the tile is staged iff the box is not empty and rows of pitch(bw) bytes fit the budget."""
    src_h, src_w, out_h, out_w = 200, 300, 200, 300
    x = wr.record(CASES[name])
    for ty in range(-(-out_h // TILE_H)):
        for tx in range(-(-out_w // TILE_W)):
            got = capi.warp_tile(x, src_h, src_w, out_h, out_w, interp, tx, ty)
            bx0, by0, bx1, by1 = footprint(CASES[name], interp, src_h, src_w, out_h, out_w, tx, ty)
            if bx1 < bx0 or by1 < by0:
                assert not got.staged and (got.x1 < got.x0 or got.y1 < got.y0), (name, tx, ty, got)
            else:
                assert (got.x0, got.y0, got.x1, got.y1) == (bx0, by0, bx1, by1), (name, tx, ty, got)
                assert got.staged == (pitch(bx1 - bx0 + 1) * (by1 - by0 + 1) <= capi.WARP_LDS_BYTES), (name, tx, ty, got)


def test_one_frame_with_staged_and_unstaged_tiles():
    """Scale 8 from a 200 x 600 source into a 16 x 67 frame: the full tile's footprint is 505 x 121 bytes, past the budget; the
    three-pixel tile beside it needs 18 x 122 and is staged.  tests/test_gpu_warp.py runs exactly this."""
    x = wr.record(CASES["scale 8"])
    for interp, (wide, narrow) in ((wr.NEAREST, ((0, 0, 504, 120), (512, 0, 528, 120))),
                                   (wr.BILINEAR, ((0, 0, 505, 121), (512, 0, 529, 121)))):
        a, b = capi.warp_tile(x, 200, 600, 16, 67, interp, 0, 0), capi.warp_tile(x, 200, 600, 16, 67, interp, 1, 0)
        assert not a.staged and tuple(a[1:]) == wide and b.staged and tuple(b[1:]) == narrow
    # an unusable record stages nothing
    assert not capi.warp_tile(wr.record(wr.IDENTITY, flags=0), 50, 50, 16, 64, 0, 0, 0).staged
    assert not capi.warp_tile(wr.record((wr.LIM_A + 1, 0, 0, 0, ONE, 0)), 50, 50, 16, 64, 0, 0, 0).staged
