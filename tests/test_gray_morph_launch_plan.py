"""The launch plan of one primitive step of the grey-level morphology (canny_hip_selftest_gray_morph_plan) against a
restatement of DESIGN.md section 39, host-only.  The launcher takes its grid from the helper this entry reports, so
tests/test_gpu_gray_morph.py can KNOW that a case sends a workgroup into its second trip."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of a launch
TILE_W, TILE_H = 128, 32


def tiles(h, w):
    return -(-h // TILE_H) * -(-w // TILE_W)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (32, 128), (33, 129), (65, 257), (2160, 3840), (32768, 32768)])
def test_the_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.gray_morph_plan(frames, h, w)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, 1), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


def test_the_tiles_of_a_frame():
    plan = capi.gray_morph_plan
    assert plan(1, 32, 128).units == 1 and plan(1, 33, 128).units == 2
    assert plan(1, 32, 129).units == 2 and plan(3, 33, 129).units == 12
    assert plan(128, 2160, 3840).units == 128 * 68 * 30
    assert plan(4096, 3, 5).trips == 1 and plan(4100, 3, 5).trips == 2
    for op in range(8):                                              # the plan itself does not depend on op or element
        k = 3 if op == capi.GRAY_MEDIAN else 31
        assert plan(7, 100, 300, op, k, k)[:4] == plan(7, 100, 300)[:4]


def test_the_route_automatic_takes_depends_on_op_and_element_alone():
    for op in range(8):
        sizes = ((3, 3), (5, 5)) if op == capi.GRAY_MEDIAN else ((1, 1), (3, 3), (1, 31), (31, 1), (5, 3), (15, 15), (31, 31))
        for kw, kh in sizes:
            auto = capi.gray_morph_plan(1, 16, 64, op, kw, kh).aux
            assert auto in (capi.GRAY_ROUTE_GENERAL, capi.GRAY_ROUTE_FAST), (op, kw, kh)
            for n, h, w in ((77, 999, 1234), (1, 1, 1), (65535, 3, 5), (2, 32768, 4000)):
                assert capi.gray_morph_plan(n, h, w, op, kw, kh).aux == auto, (op, kw, kh, n, h, w)
    # a single offset has no run to share
    assert capi.gray_morph_plan(1, 16, 64, capi.GRAY_ERODE, 1, 1).aux == capi.GRAY_ROUTE_GENERAL
    # erosions and dilations are one kernel with the comparison turned round: every morphology op draws the same line
    for kw, kh in ((3, 3), (7, 7), (15, 15), (31, 31)):
        assert len({capi.gray_morph_plan(1, 16, 64, op, kw, kh).aux for op in range(7)}) == 1


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (1, 16, 64, 8), (1, 16, 64, -1), (1, 16, 64, 0, 2, 3),
                 (1, 16, 64, 0, 3, 4), (1, 16, 64, 0, 33, 3), (1, 16, 64, 0, 3, 0), (1, 16, 64, capi.GRAY_MEDIAN, 7, 7),
                 (1, 16, 64, capi.GRAY_MEDIAN, 5, 3), (1, 16, 64, capi.GRAY_MEDIAN, 1, 1)):
        with pytest.raises(capi.CannyHipError) as ei:
            capi.gray_morph_plan(*args)
        assert ei.value.status == 1, args
    for args in ((65536, 16, 64), (1, 32769, 64), (1, 16, 32769), (1, 32768, 65536)):
        with pytest.raises(capi.CannyHipError) as ei:
            capi.gray_morph_plan(*args)
        assert ei.value.status == 2, args
    assert capi.load().canny_hip_selftest_gray_morph_plan(1, 16, 64, 0, 3, 3, None) == 1
