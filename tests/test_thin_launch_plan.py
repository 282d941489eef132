"""The launch plan of the thinning launches (canny_hip_selftest_thin_plan) against a restatement of DESIGN.md section 37,
host-only.  The launcher takes its grid from the helper this entry reports, so tests/test_gpu_thin.py can KNOW that a case
sends a workgroup into its second trip."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of the launch
TILE_WORDS, TILE_H = 8, 64


def tiles(h, w):
    return -(-h // TILE_H) * -(-(-(-w // 64)) // TILE_WORDS)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 512), (65, 513), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.thin_plan(frames, h, w)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, 1), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


def test_the_tiles_of_a_frame():
    assert capi.thin_plan(1, 64, 512).units == 1 and capi.thin_plan(1, 65, 512).units == 2
    assert capi.thin_plan(1, 64, 513).units == 2 and capi.thin_plan(3, 65, 513).units == 12
    assert capi.thin_plan(128, 2160, 3840).units == 128 * 34 * 8
    assert capi.thin_plan(4096, 3, 5).trips == 1 and capi.thin_plan(4097, 3, 5).trips == 2


def test_the_iterations_of_a_launch():
    """The fifth word: the fuse asked for, or what automatic takes (0: automatic is the stepwise route); the sizes do not
    matter."""
    auto = capi.thin_plan(1, 16, 64).aux
    assert 0 <= auto <= capi.THIN_MAX_FUSE and auto == capi.thin_plan(77, 999, 1234, 0).aux
    for fuse in range(1, capi.THIN_MAX_FUSE + 1):
        p = capi.thin_plan(3, 100, 700, fuse)
        assert p.aux == fuse and p[:4] == capi.thin_plan(3, 100, 700)[:4], "the grid does not depend on the fuse"


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (65536, 16, 64), (1, 32769, 64), (1, 16, 32769),
                 (1, 32768, 65536), (1, 16, 64, 9), (1, 16, 64, -1)):
        with pytest.raises(capi.CannyHipError):
            capi.thin_plan(*args)
    assert capi.load().canny_hip_selftest_thin_plan(1, 16, 64, 0, None) == 1
