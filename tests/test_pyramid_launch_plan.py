"""The launch plan of one pyrDown (canny_hip_selftest_pyramid_plan) against a restatement of DESIGN.md section 40, host-only.
The launchers take their grids from the helper this entry reports, so tests/test_gpu_pyramid.py can KNOW that a case sends a
workgroup into its second trip.  A pyrUp INTO planes of oh x ow has the plan of a pyrDown of planes 2 oh x 2 ow."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of a launch
TILE_W, TILE_H = 128, 32  # of the OUTPUT


def tiles(h, w):
    oh, ow = (h + 1) // 2, (w + 1) // 2
    return -(-oh // TILE_H) * -(-ow // TILE_W)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 256), (65, 257), (130, 513), (2160, 3840), (32768, 32768)])
def test_the_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.pyramid_plan(frames, h, w)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, 1), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


def test_the_tiles_of_a_frame():
    plan = capi.pyramid_plan
    # a tile is 32 x 128 outputs: 64 x 256 source pixels and, as the sizes round up, one row and one column fewer
    assert plan(1, 64, 256).units == 1 and plan(1, 63, 255).units == 1
    assert plan(1, 65, 256).units == 2 and plan(1, 64, 257).units == 2 and plan(1, 66, 258).units == 4
    assert plan(3, 65, 257).units == 12 and plan(1, 1, 1).units == 1
    assert plan(128, 2160, 3840).units == 128 * 34 * 15
    assert plan(4096, 3, 5).trips == 1 and plan(4100, 3, 5).trips == 2
    # the pyrUp of 3 x 5 planes to 6 x 10 and the pyrDown of 12 x 20 planes write planes of the same size
    assert plan(4100, 12, 20)[:4] == plan(4100, 3, 5)[:4]


def test_the_route_automatic_takes_depends_on_nothing():
    auto = capi.pyramid_plan(1, 16, 64).aux
    assert auto in (capi.PYR_ROUTE_DIRECT, capi.PYR_ROUTE_TILED)
    for n, h, w in ((77, 999, 1234), (1, 1, 1), (65535, 3, 5), (2, 32768, 4000), (128, 2160, 3840), (1, 64, 256), (1, 1, 300)):
        assert capi.pyramid_plan(n, h, w).aux == auto, (n, h, w)


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (1, -16, 64)):
        with pytest.raises(capi.CannyHipError) as ei:
            capi.pyramid_plan(*args)
        assert ei.value.status == 1, args
    for args in ((65536, 16, 64), (1, 32769, 64), (1, 16, 32769), (1, 32768, 65536)):
        with pytest.raises(capi.CannyHipError) as ei:
            capi.pyramid_plan(*args)
        assert ei.value.status == 2, args
    assert capi.load().canny_hip_selftest_pyramid_plan(1, 16, 64, None) == 1
