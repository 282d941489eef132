"""The launch plans of the temporal fusion's two capped launches (canny_hip_selftest_fuse_plan) against a restatement of
DESIGN.md section 33, host-only.  The launchers take their grids from the helper this entry reports, so
tests/test_gpu_fuse.py can KNOW that a case sends a workgroup into its second trip."""
import pytest

from canny_edge_amd import capi

CAP = 4096            # workgroups of either launch
TILE_W, TILE_H = 64, 16
MAX_REGS = 32         # the widest register instantiation of the median


def tiles(h, w):
    return -(-h // TILE_H) * -(-w // TILE_W)


@pytest.mark.parametrize("h,w", [(1, 1), (16, 64), (17, 65), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_plans_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for planes in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = planes * per
            for p in (capi.fuse_plan("mask", planes, h, w),
                      capi.fuse_plan("fuse", planes, h, w, 1, 1),                               # a window per frame
                      capi.fuse_plan("fuse", min(planes + 8, 65535), h, w, min(planes + 8, 65535) - planes + 1, 1)):   # sliding
                what = f"planes={planes} {h} x {w}: {p}"
                assert (p.units, p.per_group) == (units, 1), what
                assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
                assert (p.trips >= 2) == (units > CAP), what


def test_the_windows_of_the_plan():
    for n, group_len, step, groups in ((10, 3, 3, 3), (10, 3, 1, 8), (10, 10, 1, 1), (10, 1, 20, 1), (11, 4, 2, 4), (4098, 2, 1, 4097),
                                       (65535, 255, 255, 257)):
        assert capi.fuse_groups(n, group_len, step) == groups
        assert capi.fuse_plan("fuse", n, 16, 64, group_len, step).units == groups
        assert capi.fuse_plan(0, n, 17, 65, group_len, step).units == 4 * groups
        assert capi.fuse_plan("mask", n, 17, 65, group_len, step).units == 4 * n


def test_the_route_automatic_takes():
    for group_len in range(1, 256):
        assert capi.fuse_plan("fuse", 255, 1, 1, group_len, 1).aux == (1 if group_len <= MAX_REGS else 2), group_len
    assert capi.fuse_plan("mask", 255, 1, 1).aux == 0


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64, 1, 1), (1, 0, 64, 1, 1), (1, 16, 0, 1, 1), (65536, 16, 64, 1, 1), (1, 32769, 64, 1, 1),
                 (1, 16, 32769, 1, 1)):
        for which in ("fuse", "mask"):
            with pytest.raises(capi.CannyHipError):
                capi.fuse_plan(which, *args)
    for args in ((4, 16, 64, 0, 1), (4, 16, 64, 5, 1), (300, 16, 64, 256, 1), (4, 16, 64, 2, 0)):
        with pytest.raises(capi.CannyHipError):
            capi.fuse_plan("fuse", *args)
        capi.fuse_plan("mask", *args)                     # the mask's plan does not read the window
    with pytest.raises(capi.CannyHipError):
        capi.fuse_plan(2, 4, 16, 64)
