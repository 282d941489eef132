"""The launch plans of the reconstruction's sweep launches (canny_hip_selftest_reconstruct_plan) against a restatement of
DESIGN.md section 38, host-only.  The launcher takes its grids from the helper this entry reports, so
tests/test_gpu_reconstruct.py can KNOW that a case sends a workgroup into its second trip."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of a launch
TILE_WORDS, TILE_H = 8, 64
BLOCK = 256               # words a workgroup of the stepwise route takes per trip


def words(h, w):
    return h * -(-w // 64)


def tiles(h, w):
    return -(-h // TILE_H) * -(-(-(-w // 64)) // TILE_WORDS)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 512), (65, 513), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_tile_plan_on_both_sides_of_the_cap(h, w):
    per = tiles(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.reconstruct_plan(frames, h, w, capi.RECON_ROUTE_TILES)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, 1), what
            assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
            assert (p.trips >= 2) == (units > CAP), what


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 512), (65, 513), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_word_plan_on_both_sides_of_the_cap(h, w):
    per = words(h, w)
    for target in (1, BLOCK * (CAP - 1), BLOCK * CAP, BLOCK * CAP + 1, 3 * BLOCK * CAP + 1):
        for frames in sorted({min(max(target // per, 1), 65535), min(-(-target // per), 65535)}):
            units = frames * per
            p = capi.reconstruct_plan(frames, h, w, capi.RECON_ROUTE_STEPWISE)
            what = f"frames={frames} {h} x {w}: {p}"
            assert (p.units, p.per_group) == (units, BLOCK), what
            assert p.grid == min(CAP, -(-units // BLOCK)) and p.trips == -(-units // (p.grid * BLOCK)), what
            assert (p.trips >= 2) == (units > CAP * BLOCK), what


def test_the_tiles_of_a_frame():
    plan = lambda *a: capi.reconstruct_plan(*a, capi.RECON_ROUTE_TILES)
    assert plan(1, 64, 512).units == 1 and plan(1, 65, 512).units == 2
    assert plan(1, 64, 513).units == 2 and plan(3, 65, 513).units == 12
    assert plan(128, 2160, 3840).units == 128 * 34 * 8
    assert plan(4096, 3, 5).trips == 1 and plan(4097, 3, 5).trips == 2


def test_the_route_automatic_takes():
    """The fifth word: the route of automatic, whatever is asked about; automatic's plan is that route's."""
    auto = capi.reconstruct_plan(1, 16, 64).aux
    assert auto in (capi.RECON_ROUTE_STEPWISE, capi.RECON_ROUTE_TILES)
    for route in (0, 1, 2):
        assert capi.reconstruct_plan(77, 999, 1234, route).aux == auto
    assert capi.reconstruct_plan(3, 100, 700, 0)[:4] == capi.reconstruct_plan(3, 100, 700, auto)[:4]


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (65536, 16, 64), (1, 32769, 64), (1, 16, 32769),
                 (1, 32768, 65536), (1, 16, 64, 3), (1, 16, 64, -1)):
        with pytest.raises(capi.CannyHipError):
            capi.reconstruct_plan(*args)
    assert capi.load().canny_hip_selftest_reconstruct_plan(1, 16, 64, 0, None) == 1
