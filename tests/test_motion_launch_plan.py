"""The launch plans of the motion estimate (canny_hip_selftest_motion_plan) against a restatement of DESIGN.md section 31,
host-only: every capped launch 64 items below its cap, at it, 64 above and at three trips' worth.  The launchers take their
grids from the helpers this entry reports, so tests/test_gpu_motion.py can KNOW that a case sends a wave into its second
trip."""
import numpy as np
import pytest

from canny_edge_amd import capi

CAP = 2048   # workgroups of every capped launch of the motion estimate
BLOCK = 256  # hypotheses of one score workgroup


def units_of(which, n_pairs, hypotheses):
    return n_pairs * -(-hypotheses // BLOCK) if which == "score" else n_pairs


@pytest.mark.parametrize("which", ["gather", "score", "refit"])
def test_the_plan_on_both_sides_of_the_cap(which):
    for hypotheses in (1, 255, 256, 257, 1024, 4095, 4096):
        blocks = -(-hypotheses // BLOCK) if which == "score" else 1
        for target, crossed in ((CAP - 64, False), (CAP, False), (CAP + 64, True), (3 * CAP + 64, True)):
            for n_pairs in sorted({target // blocks, -(-target // blocks)}):
                units = units_of(which, n_pairs, hypotheses)
                p = capi.motion_plan(which, n_pairs, hypotheses)
                what = f"{which} n_pairs={n_pairs} hypotheses={hypotheses}: {p}"
                assert (p.units, p.per_group, p.aux) == (units, 1, 0), what
                assert p.grid == min(CAP, units) and p.trips == -(-units // p.grid), what
                assert (p.trips >= 2) == (units > CAP), what
                if units == target:
                    assert (p.trips >= 2) == crossed and p.trips == (1 if not crossed else 2 if units < 2 * CAP else 4), what


def test_small_batches_take_small_grids_and_the_limits_hold():
    assert capi.motion_plan("gather", 1).grid == 1 and capi.motion_plan("refit", 127, 4096).grid == 127
    assert capi.motion_plan("score", 127, 4096) == capi.LaunchPlan(2032, 1, 2032, 1, 0)
    assert capi.motion_plan("score", 127, 1024).grid == 508 and capi.motion_plan("score", 129, 4096).trips == 2
    big = capi.motion_plan("score", capi.MATCH_MAX_PAIRS, capi.MOTION_MAX_HYPOTHESES)
    assert (big.units, big.grid, big.trips) == (1 << 24, CAP, 1 << 13)
    assert capi.MOTION_PLANS == ("gather", "score", "refit")
    L = capi.load()
    out = np.zeros(5, np.uint64)
    for args in ((0, 0, 16), (1, 1, 0), (1, 1, 4097), (1, (1 << 20) + 1, 16), (3, 1, 16), (-1, 1, 16), (2, 0, 1)):
        assert L.canny_hip_selftest_motion_plan(*args, capi._hp(out)) == 1, args
    assert L.canny_hip_selftest_motion_plan(0, 1, 16, None) == 1
    assert not out.any()
