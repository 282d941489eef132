"""The launch plans of the contour shape measures (canny_hip_selftest_shapes_plan) against the rows of DESIGN.md section
21, host-only: every capped launch 64 items below its cap, at it, 64 above and at three trips' worth.  The launchers take
their grids from the helpers this entry reports, so tests/test_gpu_shapes.py can KNOW that a case sends a wave into its
second trip."""
import pytest

from canny_edge_amd import capi

# which -> (record slots per item, items per workgroup and trip, cap on the grid)
TABLE = {"records": (1, 4, 65536), "scan_sums": (2048, 256, 1)}


@pytest.mark.parametrize("which", sorted(TABLE))
def test_the_plan_on_both_sides_of_the_cap(which):
    per_item, per_group, cap = TABLE[which]
    per_trip = per_group * cap
    for units, crossed in ((per_trip - 64, False), (per_trip, False), (per_trip + 64, True), (3 * per_trip + 64, True)):
        if units < 1:
            continue
        for capacity in sorted({units * per_item, (units - 1) * per_item + 1}):
            p = capi.shapes_plan(which, capacity)
            what = f"{which} capacity={capacity}: {p}"
            assert p.units == units and p.per_group == per_group and p.aux == 0, what
            assert p.grid == min(cap, -(-units // per_group)), what
            assert p.trips == -(-units // (p.grid * per_group)) and (p.trips >= 2) == crossed, what
            assert p.trips == (1 if not crossed else 2 if units < 2 * per_trip else 4), what


def test_the_plans_are_those_of_the_polygon_stage_and_small_capacities_take_small_grids():
    for capacity in (1, 3, 4, 5, 2048, 2049, 65536 * 4 + 4099, 256 * 2048 + 4099):
        assert capi.shapes_plan("records", capacity) == capi.launch_plan("pg_records", extra=capacity)
        assert capi.shapes_plan("scan_sums", capacity) == capi.launch_plan("pg_scan_sums", extra=capacity)
    assert capi.shapes_plan("records", 1).grid == 1 and capi.shapes_plan("records", 5).grid == 2
    assert capi.shapes_plan("scan_sums", 2049).units == 2
    for bad in (("records", 0), ("scan_sums", 0), (2, 1), (-1, 1)):
        with pytest.raises(capi.CannyHipError):
            capi.shapes_plan(*bad)
