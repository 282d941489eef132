"""The launch plans of the chamfer matching (canny_hip_selftest_chamfer_plan, canny_hip_selftest_chamfer_bands) against the
rows of DESIGN.md section 21, host-only: every capped launch 64 items below its cap, at it, 64 above and at three trips'
worth; the chunks the batch is walked in; and the sizes at which the tiled score kernel changes geometry -- one band of dy
or several, and the automatic choice of the route.  The launchers take their grids and the set its bands from the helpers
these entries report, so tests/test_gpu_chamfer.py can KNOW that a case sends a wave into its second trip."""
import numpy as np
import pytest

from canny_edge_amd import capi

# which -> (items per workgroup and trip, cap on the grid)
TABLE = {"cost": (256, 16384), "cells": (256, 2048)}
TILE_X, TILE_Y, LDS_ELEMS = 64, 16, 32768


def _sizes(which, units):
    """(n_frames, height, width, n_templates) of a call whose capped launch walks exactly `units` items."""
    if which == "cost":                      # pixels of the chunk; with one template of 1-pixel-high frames: one chunk
        for n in range(min(4096, units), 0, -1):
            if units % n == 0:
                return n, 1, units // n, 1
    for T in range(min(1024, units), 0, -1):  # anchors of ONE frame: T * h * w
        if units % T == 0:
            return 3, 1, units // T, T
    raise AssertionError((which, units))


@pytest.mark.parametrize("which", sorted(TABLE))
def test_the_plan_on_both_sides_of_the_cap(which):
    per_group, cap = TABLE[which]
    per_trip = per_group * cap
    for units, crossed in ((per_trip - 64, False), (per_trip, False), (per_trip + 64, True), (3 * per_trip + 64, True)):
        n, h, w, T = _sizes(which, units)
        p, chunk = capi.chamfer_plan(which, n, h, w, T, with_scores=True)
        what = f"{which} n={n} h={h} w={w} T={T}: {p}, chunk {chunk}"
        assert chunk == n, what
        assert p.units == units and p.per_group == per_group and p.aux == 0, what
        assert p.grid == min(cap, -(-units // per_group)), what
        assert p.trips == -(-units // (p.grid * per_group)) and (p.trips >= 2) == crossed, what
        assert p.trips == (1 if not crossed else 2 if units < 2 * per_trip else 4), what


def test_the_chunks_of_a_batch():
    plan = capi.chamfer_plan
    # at most 4096 frames, whatever their size
    assert plan("cells", 4096, 2, 2, 1)[1] == 4096 and plan("cells", 4097, 2, 2, 1)[1] == 4096
    assert plan("cells", 65535, 1, 1, 1, True)[1] == 4096
    # with d_scores: as many frames as keep the u16 cost plane, 2 * h * w bytes each, within 256 MiB
    assert plan("cells", 128, 2160, 3840, 8, True)[1] == (256 << 20) // (2 * 2160 * 3840) == 16
    assert plan("cells", 3, 16384, 16384, 1, True)[1] == 1          # one frame at least: 512 MiB of costs
    # without d_scores: as many frames as keep 4 * T * h * w bytes each within 256 MiB, one at least
    per_frame = 4 * 8 * 512 * 512                                   # 8 MiB
    assert plan("cells", 100, 512, 512, 8)[1] == (256 << 20) // per_frame == 32
    assert plan("cells", 100, 512, 512, 8, True)[1] == 100
    assert plan("cells", 20, 512, 512, 8)[1] == 20
    assert plan("cells", 5, 2160, 3840, 8)[1] == 1                   # a 4K frame with 8 templates: 253 MiB
    assert plan("cells", 5, 2160, 3840, 9)[1] == 1                   # ... and one frame at least beyond the budget
    assert plan("cells", 128, 2160, 3840, 1)[1] == 8
    # the cost plan is that of a full chunk
    p, chunk = plan("cost", 128, 2160, 3840, 1)
    assert chunk == 8 and p.units == 8 * 2160 * 3840 and p.grid == 16384 and p.trips == 16
    for bad in ((2, 1, 1, 1, 1), (0, 0, 1, 1, 1), (0, 1, 0, 1, 1), (0, 1, 1, 1, 0), (0, 1, 1, 1, 1025), (1, 1, 1500, 1500, 1024)):
        with pytest.raises(capi.CannyHipError):
            plan(*bad)


def _row(dxs, dys):
    return [np.array([(x, y) for y in dys for x in dxs], np.int16)]


def test_one_band_or_several():
    """A band holds as many rows of dy as keep (rows of dy + 15) * (64 + dx span) u16 within 64 KiB of LDS."""
    for dx_span in (0, 1, 63, 200, 448, 449, 510):
        cols = TILE_X + dx_span
        span = LDS_ELEMS // cols - TILE_Y + 1       # rows of dy one band takes
        assert span >= 42
        for dy_span, bands in ((0, 1), (span - 1, 1), (span, 2), (2 * span - 1, 2), (2 * span, 3)):
            if dy_span > 510:
                continue
            dys = range(-(dy_span // 2), dy_span - dy_span // 2 + 1)
            got = capi.chamfer_bands(_row((-(dx_span // 2), dx_span - dx_span // 2), dys))
            want_elems = (min(dy_span + 1, span) + TILE_Y - 1) * cols
            assert got[:3] == (bands, want_elems, want_elems), (dx_span, dy_span, got)
            assert want_elems <= LDS_ELEMS
    # rows of dy without points cost nothing: a band starts at the next dy that has a point
    got = capi.chamfer_bands(_row((-255, 255), (-255, 0, 255)))
    assert got[0] == 3 and got[1] == TILE_Y * (TILE_X + 510)
    # the launch's LDS is the largest tile of the set, the bands are per template
    two = _row((0,), (0,)) + _row((-255, 255), range(-100, 101))
    assert capi.chamfer_bands(two, 0)[:2] == (1, TILE_Y * TILE_X)
    b = capi.chamfer_bands(two, 1)
    assert b[0] == 5 and b[1] == b[2] == capi.chamfer_bands(two, 0)[2] == 57 * 574


def test_the_automatic_route():
    """Direct (1) for sets whose largest template has fewer than 8 points, tiled (2) from 8 on."""
    for k, route in ((1, 1), (7, 1), (8, 2), (9, 2), (257, 2)):
        tpl = [np.array([(i % 5, i // 5) for i in range(k)], np.int16)]
        assert capi.chamfer_bands(tpl)[3] == route, k
        assert capi.chamfer_bands([tpl[0][:1]] + tpl + [tpl[0][:2]], 1)[3] == route, k   # the largest template decides
    with pytest.raises(capi.CannyHipError):
        capi.chamfer_bands(_row((256,), (0,)))
    with pytest.raises(capi.CannyHipError):
        capi.chamfer_bands(_row((0,), (0,)), 1)
