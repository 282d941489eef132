"""The launch plans of the binarization (canny_hip_selftest_binarize_plan) against a restatement of DESIGN.md section 36,
host-only.  The launchers take their grids from the helpers this entry reports, so tests/test_gpu_binarize.py can KNOW that a
case sends a workgroup into its second trip, and where a strip and a segment end."""
import pytest

from canny_edge_amd import capi

CAP = 4096                # workgroups of every launch
CHUNK = 256               # output bytes a workgroup takes per trip (FIXED, OTSU, the straightforward route)
STRIP = 512               # useful columns of a marching strip
WAVES = 4                 # marching work items (strip, segment) a workgroup takes per trip


def chunks(h, w):
    return -(-(h * -(-w // 8)) // CHUNK)


def segment_rows(kh):
    return max(64, 2 * kh)


def items(h, w, kh):
    return -(-w // STRIP) * -(-h // segment_rows(kh))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (64, 512), (65, 513), (33, 257), (2160, 3840), (32768, 32768)])
def test_the_bytes_plan_on_both_sides_of_the_cap(h, w):
    per = chunks(h, w)
    for target in (1, CAP - 64, CAP, CAP + 64, 3 * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            for method in (capi.BIN_FIXED, capi.BIN_OTSU) if h * w <= capi.BIN_OTSU_MAX_PIXELS else (capi.BIN_FIXED,):
                p, t = capi.binarize_plan(frames, h, w, method)
                what = f"frames={frames} {h} x {w}: {p}"
                assert (p.units, p.per_group, p.aux) == (units, 1, 0), what
                assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid) == t.direct_trips, what
                assert (p.trips >= 2) == (units > CAP), what
            assert capi.binarize_plan(frames, h, w, capi.BIN_ADAPTIVE_MEAN, 3, 3)[1].direct_trips == -(-units // min(CAP, units))


@pytest.mark.parametrize("h,w,kh", [(1, 1, 3), (64, 512, 3), (65, 513, 31), (2160, 3840, 15), (2160, 3840, 255), (32768, 32768, 101)])
def test_the_marching_plan_on_both_sides_of_the_cap(h, w, kh):
    per = items(h, w, kh)
    for target in (1, WAVES * CAP - 64, WAVES * CAP, WAVES * CAP + 64, 3 * WAVES * CAP + 64):
        for frames in sorted({max(target // per, 1), min(-(-target // per), 65535)}):
            units = frames * per
            p, t = capi.binarize_plan(frames, h, w, capi.BIN_ADAPTIVE_MEAN, 3, kh)
            assert p.aux in (1, 2)
            grid = min(CAP, -(-units // WAVES))
            assert t.march_trips == -(-units // (grid * WAVES)), (frames, t)
            assert (t.march_trips >= 2) == (units > WAVES * CAP)
            if p.aux == 2:
                assert (p.units, p.per_group, p.grid, p.trips) == (units, WAVES, grid, t.march_trips)
            else:
                assert (p.units, p.per_group, p.trips) == (frames * chunks(h, w), 1, t.direct_trips)


def test_the_tiling():
    for kh in range(3, 256, 2):
        t = capi.binarize_plan(1, 64, 64, capi.BIN_ADAPTIVE_MEAN, 3, kh)[1]
        assert t.strip_cols == STRIP and STRIP % 8 == 0, "a strip starts at a multiple of 8 columns: an output byte has one writer"
        assert t.segment_rows == segment_rows(kh) and t.segment_rows >= 2 * (kh - 1), "the warm-up is at most half the rows loaded"
    for kw in range(3, 256, 2):
        t = capi.binarize_plan(1, 64, 64, capi.BIN_ADAPTIVE_MEAN, kw, 3)[1]
        assert t.staged_cols % 64 == 0 and t.staged_cols >= STRIP + kw - 1, "the strip and kw / 2 halo columns a side are staged"
    assert capi.binarize_plan(1, 64, 64, capi.BIN_ADAPTIVE_MEAN, 65, 3)[1].staged_cols == 576
    assert capi.binarize_plan(1, 64, 64, capi.BIN_ADAPTIVE_MEAN, 67, 3)[1].staged_cols == 832


def test_the_route_automatic_takes():
    """The fifth word: 1 straightforward, 2 marching, from the window alone (DESIGN.md section 36 draws the line); 0 for the
    methods that have no routes."""
    for kw in (3, 5, 15, 31, 65, 67, 101, 255):
        for kh in (3, 5, 15, 31, 101, 255):
            aux = capi.binarize_plan(1, 16, 64, capi.BIN_ADAPTIVE_MEAN, kw, kh)[0].aux
            assert aux in (1, 2), (kw, kh)
            assert aux == capi.binarize_plan(77, 999, 1234, capi.BIN_ADAPTIVE_MEAN, kw, kh)[0].aux, "the route depends on the window alone"
    assert capi.binarize_plan(1, 16, 64, capi.BIN_FIXED)[0].aux == 0 and capi.binarize_plan(1, 16, 64, capi.BIN_OTSU, 4, 0)[0].aux == 0


def test_the_plan_refuses_what_the_calls_refuse():
    for args in ((0, 16, 64), (1, 0, 64), (1, 16, 0), (-1, 16, 64), (65536, 16, 64), (1, 32769, 64), (1, 16, 32769),
                 (1, 32768, 65536)):
        with pytest.raises(capi.CannyHipError):
            capi.binarize_plan(*args)
    for kw, kh in ((1, 3), (2, 3), (3, 2), (257, 3), (3, 257), (-1, 3), (3, 1)):
        with pytest.raises(capi.CannyHipError):
            capi.binarize_plan(1, 16, 64, capi.BIN_ADAPTIVE_MEAN, kw, kh)
    for method in (-1, 3):
        with pytest.raises(capi.CannyHipError):
            capi.binarize_plan(1, 16, 64, method)
    with pytest.raises(capi.CannyHipError) as ei:
        capi.binarize_plan(1, 8193, 8192, capi.BIN_OTSU)
    assert ei.value.status == 2
    assert capi.load().canny_hip_selftest_binarize_plan(1, 16, 64, 2, 3, 3, None) == 1
