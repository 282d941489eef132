"""The launch plan of the edge curves' row kernels (canny_hip_selftest_curves_plan) against its row of DESIGN.md section
21, host-only: 64 rows below the cap of the grid, at it, 64 above and at three trips' worth.  The launchers take their grid
from the helper this entry reports, so tests/test_gpu_curves.py can KNOW that a case sends a wave into its second trip."""
import pytest

from canny_edge_amd import capi

PER_GROUP, CAP = 4, 65536    # image rows per workgroup and trip, cap on the grid


def test_the_plan_on_both_sides_of_the_cap():
    per_trip = PER_GROUP * CAP
    h = 64
    for rows, crossed in ((per_trip - 64, False), (per_trip, False), (per_trip + 64, True), (3 * per_trip + 64, True)):
        n = rows // h
        assert n * h == rows and n <= 65535
        for w in (1, 9, 130):
            p = capi.curves_plan(n, h, w)
            what = f"{n} x {h} x {w}: {p}"
            assert p.units == rows and p.per_group == PER_GROUP and p.aux == 0, what
            assert p.grid == min(CAP, -(-rows // PER_GROUP)), what
            assert p.trips == -(-rows // (p.grid * PER_GROUP)) and (p.trips >= 2) == crossed, what
            assert p.trips == (1 if not crossed else 2 if rows < 2 * per_trip else 4), what


def test_small_batches_take_small_grids_and_bad_sizes_are_refused():
    assert capi.curves_plan(1, 1, 1).grid == 1 and capi.curves_plan(1, 5, 7).grid == 2
    assert capi.curves_plan(3, 270, 480) == capi.launch_plan("ct_rows", 3, 270, 480)   # the contours' row grid
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8), (1, 1 << 15, (1 << 13) + 1)):
        with pytest.raises(capi.CannyHipError):
            capi.curves_plan(*bad)
