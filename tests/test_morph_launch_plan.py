"""The launch plan of one primitive step of the binary morphology (canny_hip_selftest_morph_plan) against a restatement of
DESIGN.md section 34, host-only.  The launcher takes its grid from the helper this entry reports, so tests/test_gpu_morph.py
can KNOW that a case sends a workgroup into its second trip."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of the launch
TILE_WORDS, TILE_H = 8, 64


def tiles(h, w):
    return -(-h // TILE_H) * -(-(-(-w // 64)) // TILE_WORDS)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (64, 512), (65, 513), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.morph_plan(frames, h, w)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, 1), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


def test_the_tiles_of_a_frame():
    assert capi.morph_plan(1, 64, 512).units == 1 and capi.morph_plan(1, 65, 512).units == 2
    assert capi.morph_plan(1, 64, 513).units == 2 and capi.morph_plan(3, 65, 513).units == 12
    assert capi.morph_plan(128, 2160, 3840).units == 128 * 34 * 8


def test_the_route_automatic_takes():
    """The fifth word: 1 general, 2 separable, for a full rectangle of that size (DESIGN.md section 34 draws the line)."""
    for kw in range(1, 32, 2):
        for kh in range(1, 32, 2):
            aux = capi.morph_plan(1, 16, 64, kw, kh).aux
            assert aux in (1, 2), (kw, kh)
            assert aux == capi.morph_plan(77, 999, 1234, kw, kh).aux, "the route depends on the element alone"
    assert capi.morph_plan(1, 16, 64, 1, 1).aux == 1 and capi.morph_plan(1, 16, 64, 31, 31).aux == 2


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (65536, 16, 64), (1, 32769, 64), (1, 16, 32769),
                 (1, 32768, 65536)):
        with pytest.raises(capi.CannyHipError):
            capi.morph_plan(*args)
    for kw, kh in ((0, 3), (2, 3), (3, 2), (33, 3), (3, 33), (-1, 3)):
        with pytest.raises(capi.CannyHipError):
            capi.morph_plan(1, 16, 64, kw, kh)
    assert capi.load().canny_hip_selftest_morph_plan(1, 16, 64, 3, 3, None) == 1
