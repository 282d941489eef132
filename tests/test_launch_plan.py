"""canny_hip_selftest_launch_plan against the table of DESIGN.md section 21: for every launch whose grid is capped, the
work items, the items a workgroup takes per trip of its grid-stride loop and the cap -- checked one item below the cap
(one trip, the grid still grows with the work) and one above (the grid stays, a second trip begins).  Host-only: the
launchers take their grids from the helpers this entry reports, so tests/test_gpu_past_the_grid_cap.py can KNOW that a
case sends a wave into its second trip."""
import numpy as np
import pytest

from canny_edge_amd import capi

N_MAX = 65535  # frames a batch call takes

# kind -> (items per workgroup and trip, cap on the grid): the "one trip covers" column of section 21
TABLE = {
    "points_rows": (16, 65536),
    "scan_frames": (256, 1),
    "cc_tiles": (4, 65536),
    "cc_rows": (4, 65536),
    "cc_fixup": (256, 4096),
    "ct_rows": (4, 65536),
    "edt_rows": (4, 65536),
    "edt_columns": (4, 65536),
    "pg_records": (4, 65536),
    "pg_scan_sums": (256, 1),
    "hough_vote_strong": (256, 2048),
    "hough_vote_bits": (256, 2048),
    "hough_vote_points": (256, 2048),
    "hough_cells": (256, 4096),
    "circles_vote_strong": (1, 2048),
    "circles_vote_bits": (1, 2048),
    "circles_steps": (256, 8192),
    "to_gray": (256, 8192),
}


def _sizes(kind, units):
    """A valid call of `kind` with exactly `units` work items (n_frames, height, width, extra), or None if no call has."""
    if kind in ("points_rows", "cc_rows", "ct_rows"):           # image rows of the batch
        for n in range(min(N_MAX, units), 0, -1):
            if units % n == 0:
                return n, units // n, 8, 0
    if kind == "edt_rows":                                      # groups of 8 rows (the cap lies beyond the switch)
        return _sizes("cc_rows", units * 8)
    if kind == "cc_tiles":                                      # 64 x 64 tiles of the batch: frames one pixel wide
        for n in range(min(N_MAX, units), 0, -1):
            if units % n == 0:
                return n, 64 * (units // n), 1, 0
    if kind == "edt_columns":                                   # 64-column strips of the batch: frames one row high
        for n in range(min(N_MAX, units), 0, -1):
            if units % n == 0:
                return n, 1, 64 * (units // n), 0
    if kind == "scan_frames":
        return units, 1, 1, 0
    if kind == "hough_vote_strong":                             # words of the frame's tiles: a multiple of 64
        return (1, units, 8, 0) if units % 64 == 0 else None
    if kind == "hough_vote_bits":                               # one word per row of a narrow frame
        return 1, units, 8, 0
    if kind == "hough_vote_points":                             # as many points as pixels / 16, which sizes the grid
        return 1, units, 16, units
    if kind in ("circles_vote_strong", "circles_vote_bits"):    # chunks of 64 words
        return 1, units * 64, 8, 0
    if kind in ("cc_fixup", "pg_records", "hough_cells", "circles_steps"):
        return 1, 1, 1, units
    if kind == "pg_scan_sums":                                  # chunks of 2048 records
        return 1, 1, 1, units * 2048
    if kind == "to_gray":                                       # groups of 16 pixels
        return 1, 1, 1, units * 16
    raise AssertionError(kind)


def test_the_table_names_every_kind():
    assert set(TABLE) == set(capi.PLAN_KINDS) and len(capi.PLAN_KINDS) == 18


@pytest.mark.parametrize("kind", capi.PLAN_KINDS)
def test_the_plan_on_both_sides_of_the_cap(kind):
    per_group, cap = TABLE[kind]
    per_trip = per_group * cap
    if kind == "hough_cells":
        # uncapped the grid is sized for FOUR trips of 256 cells: the cap of 4096 workgroups is reached at 4 Mi cells
        per_trip *= 4
    for units, crossed in ((per_trip - 64, False), (per_trip, False), (per_trip + 64, True), (3 * per_trip + 64, True)):
        if units < 1:
            continue
        sizes = _sizes(kind, units)
        assert sizes is not None, (kind, units)
        n, h, w, extra = sizes
        p = capi.launch_plan(kind, n, h, w, extra)
        what = f"{kind} n={n} h={h} w={w} extra={extra}: {p}"
        assert p.units == units and p.per_group == per_group, what
        assert p.trips == -(-p.units // (p.grid * p.per_group)), what
        if kind == "hough_cells":
            assert p.grid == min(cap, -(-units // (4 * per_group))), what
            assert p.trips == (4 if not crossed else -(-units // (cap * per_group))) and p.trips >= 4, what
            assert (p.trips > 4) == crossed, what
        else:
            assert p.grid == min(cap, -(-units // per_group)), what
            assert (p.trips >= 2) == crossed and (p.grid == cap or not crossed), what
        assert p.aux == (8 if kind == "edt_rows" else 0), what


def test_one_item_above_the_cap_is_a_second_trip():
    """The smallest crossings: exactly one item more than a trip covers."""
    for kind, sizes in (("cc_fixup", (1, 1, 1, 4096 * 256 + 1)), ("pg_records", (1, 1, 1, 65536 * 4 + 1)),
                        ("circles_steps", (1, 1, 1, 8192 * 256 + 1)), ("to_gray", (1, 1, 1, 8192 * 256 * 16 + 16)),
                        ("scan_frames", (257, 1, 1, 0)), ("hough_vote_bits", (1, 2048 * 256 + 1, 8, 0)),
                        ("circles_vote_bits", (1, 2048 * 64 + 1, 8, 0)), ("pg_scan_sums", (1, 1, 1, 256 * 2048 + 1))):
        p = capi.launch_plan(kind, *sizes)
        assert p.trips == 2 and p.units == TABLE[kind][0] * TABLE[kind][1] + 1, (kind, p)
        below = list(sizes)
        if kind == "scan_frames":
            below[0] -= 1
        elif kind in ("hough_vote_bits", "circles_vote_bits"):
            below[1] -= 1
        else:
            below[3] -= 16 if kind == "to_gray" else 1
        assert capi.launch_plan(kind, *below).trips == 1, kind


def test_to_gray_counts_whole_groups_of_16_pixels():
    assert capi.launch_plan("to_gray", extra=15) == (0, 256, 1, 0, 0)
    assert capi.launch_plan("to_gray", extra=16 * 257 + 15)[:3] == (257, 256, 2)


def test_the_strong_plane_counts_the_rows_that_pad_its_last_tile():
    bits = capi.launch_plan("hough_vote_bits", 1, 65, 130)
    strong = capi.launch_plan("hough_vote_strong", 1, 65, 130)
    assert bits.units == 65 * 3 and strong.units == 2 * 3 * 64 and bits.grid == strong.grid == 2
    assert capi.launch_plan("circles_vote_bits", 1, 65, 130).units == 4      # ceil(195 / 64)
    assert capi.launch_plan("circles_vote_strong", 1, 65, 130).units == 6


def test_the_point_list_vote_walks_the_points_on_a_grid_sized_by_the_pixels():
    for points in (0, 1, 528, 529, 100000):
        p = capi.launch_plan("hough_vote_points", 1, 65, 130, points)
        assert p.units == points and p.grid == -(-(65 * 130 // 16) // 256) == 3 and p.per_group == 256
        assert p.trips == -(-points // (3 * 256))
    big = capi.launch_plan("hough_vote_points", 1, 1100003, 8, 3000000)
    assert big.grid == 2048 and big.trips == 6


def test_the_rows_per_wave_switch_of_the_edt_row_pass():
    """One row per wave below 65 536 rows of the batch, eight from there on."""
    for n, h in ((1, 65535), (255, 257), (N_MAX, 1)):
        p = capi.launch_plan("edt_rows", n, h, 8)
        assert p.aux == 1 and p.units == n * h and p.grid == -(-n * h // 4) and p.trips == 1, p
    for n, h in ((1, 65536), (256, 256), (2, 32768), (N_MAX, 2)):
        p = capi.launch_plan("edt_rows", n, h, 8)
        assert p.aux == 8 and p.units == -(-n * h // 8) and p.grid == min(65536, -(-p.units // 4)), p
    p = capi.launch_plan("edt_rows", 1, 65537, 8)
    assert p.units == 8193 and p.aux == 8                                   # the last wave takes one row
    # with one row per wave the cap is out of reach; with eight it lies at 2 Mi rows
    assert capi.launch_plan("edt_rows", N_MAX, 32, 8).trips == 1
    assert capi.launch_plan("edt_rows", 63560, 33, 8).trips == 2


def test_the_width_counts_only_where_the_unit_is_a_tile_or_a_strip():
    for w in (1, 64, 65, 4096):
        assert capi.launch_plan("cc_rows", 9, 100, w).units == 900
        assert capi.launch_plan("cc_tiles", 9, 100, w).units == 9 * 2 * -(-w // 64)
        assert capi.launch_plan("edt_columns", 9, 100, w).units == 9 * -(-w // 64)


def test_invalid_requests_are_refused():
    for args in ((-1, 1, 1, 1, 1), (18, 1, 1, 1, 1), (1000, 1, 1, 1, 1),
                 ("cc_rows", 0, 8, 8, 0), ("cc_rows", N_MAX + 1, 8, 8, 0), ("cc_rows", 1, 0, 8, 0), ("cc_tiles", 1, 8, 0, 0),
                 ("edt_rows", 1, 65536, 65536, 0),                       # more than 2^31 - 1 pixels in a frame
                 ("scan_frames", 0, 1, 1, 0), ("scan_frames", N_MAX + 1, 1, 1, 0),
                 ("hough_vote_points", 1, 8, 8, -1), ("cc_fixup", 1, 1, 1, 0), ("pg_records", 1, 1, 1, -5), ("to_gray", 1, 1, 1, 0), ("hough_cells", 1, 1, 1, 0)):
        with pytest.raises(capi.CannyHipError):
            capi.launch_plan(*args)
    with pytest.raises(ValueError):
        capi.launch_plan("no_such_kind")
    assert capi.load().canny_hip_selftest_launch_plan(0, 1, 1, 1, 0, None) != 0


def test_the_query_needs_no_context_and_changes_nothing():
    a = [capi.launch_plan(k, 7, 129, 130, 1000) for k in capi.PLAN_KINDS]
    b = [capi.launch_plan(k, 7, 129, 130, 1000) for k in capi.PLAN_KINDS]
    assert a == b and all(isinstance(v, int) for p in a for v in p)
    out = np.full(6, 0xEE, np.uint64)
    assert capi.load().canny_hip_selftest_launch_plan(3, 7, 129, 130, 0, out.ctypes.data) == 0
    assert out[5] == 0xEE and out[0] == 7 * 129
