"""GPU: every feature's profile parts sit in slots of their own.  One long-lived context with profiling on; after the
smallest call of a feature, launches are counted in that feature's parts (and those of the features it is documented
to run, and the canny stages) and nowhere else; each getter accepts its last part and refuses the one behind it.  Counts
only, no timing."""
import numpy as np
import pytest

from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

H, W = 48, 64
SIGMA, LO, HI = 1.4, 50, 150
INVALID = 1  # CANNY_HIP_ERR_INVALID
SQUARE = np.array([(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2), (1, 2), (2, 2)])   # a chamfer template: (dx, dy) offsets

# feature -> (the Context method that reads its parts, how many parts it has)
FEATURES = {
    "hough": ("hough_profile_get", 3),
    "components": ("components_profile_get", 4),
    "edt": ("edt_profile_get", 2),
    "hough_segments": ("hough_segments_profile_get", 3),
    "contours": ("contours_profile_get", 4),
    "hough_circles": ("hough_circles_profile_get", 4),
    "polygons": ("polygons_profile_get", 3),
    "edgels": ("edgels_profile_get", 2),
    "line_fits": ("line_fits_profile_get", 1),
    "circle_fits": ("circle_fits_profile_get", 1),
    "chamfer": ("chamfer_profile_get", 4),
    "shapes": ("shapes_profile_get", 3),
    "curves": ("curves_profile_get", 2),
    "corners": ("corners_profile_get", 4),
    "descriptors": ("descriptors_profile_get", 4),
    "motion": ("motion_profile_get", 3),
    "warp": ("warp_profile_get", 2),
    "fuse": ("fuse_profile", 2),
    "morph": ("morph_profile", 1),
}


def _calls(hip, frame):
    """feature -> (its smallest call, the other features that call is documented to run)"""
    batch, pair = frame[None], np.stack([frame, frame])   # the calls that need a batch, or two frames, get the one frame
    return {
        "hough": (lambda c: c.canny_hough(frame, SIGMA, LO, HI, threshold=10, lines_max=8), ()),
        "components": (lambda c: c.canny_components(frame, SIGMA, LO, HI), ()),
        "polygons": (lambda c: c.canny_polygons(frame, SIGMA, LO, HI), ("contours",)),
        "edgels": (lambda c: c.canny_edgels(frame, SIGMA, LO, HI), ()),
        "morph": (lambda c: c.canny_morph(batch, SIGMA, LO, HI, hip.MORPH_DILATE, hip.morph_element(hip.MORPH_RECT, 3), 3, 3), ()),
        "edt": (lambda c: c.canny_edt(frame, SIGMA, LO, HI), ()),
        "contours": (lambda c: c.canny_contours(frame, SIGMA, LO, HI), ()),
        "curves": (lambda c: c.canny_curves(frame, SIGMA, LO, HI), ()),
        "shapes": (lambda c: c.canny_shapes(frame, SIGMA, LO, HI), ("contours",)),
        "hough_segments": (lambda c: c.canny_hough_segments(frame, SIGMA, LO, HI, threshold=10, lines_max=8), ("hough",)),
        "corners": (lambda c: c.canny_corners(frame, SIGMA, LO, HI), ()),
        "hough_circles": (lambda c: c.canny_hough_circles(frame, SIGMA, LO, HI, 3, 12, threshold=5, support_threshold=5), ()),
        "line_fits": (lambda c: c.canny_hough_line_fits(frame, SIGMA, LO, HI, threshold=10, lines_max=8),
                      ("hough", "hough_segments")),
        "circle_fits": (lambda c: c.canny_hough_circle_fits(frame, SIGMA, LO, HI, 3, 12, threshold=5, support_threshold=5),
                        ("hough_circles",)),
        "chamfer": (lambda c: c.canny_chamfer(frame, SIGMA, LO, HI, c.chamfer_set_create([SQUARE]), 160, 80), ("edt",)),
        "descriptors": (lambda c: c.canny_corner_descriptors(frame, SIGMA, LO, HI), ("corners",)),
        "motion": (lambda c: c.canny_motion(pair, SIGMA, LO, HI), ("corners", "descriptors")),
        "warp": (lambda c: c.canny_align(pair, SIGMA, LO, HI), ("corners", "descriptors", "motion")),
        "fuse": (lambda c: c.canny_background(pair, SIGMA, LO, HI), ("corners", "descriptors", "motion", "warp")),
    }


def _read(ctx):
    """feature -> [(ms, launches) of every part]"""
    return {f: [getattr(ctx, m)(p) for p in range(n)] for f, (m, n) in FEATURES.items()}


def test_the_table_covers_every_getter(hip):
    exported = {n for n in hip.EXPORTS if n.endswith("_profile_get")} - {"canny_hip_profile_get"}
    assert {"canny_hip_%s_profile_get" % f for f in FEATURES} == exported


def test_each_feature_counts_in_its_own_parts_only(hip):
    frame = synth_frame(H, W)
    calls = _calls(hip, frame)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 0)   # all slots
        for feature, (call, runs_also) in calls.items():
            ctx.profile_reset()
            call(ctx)
            got = _read(ctx)
            print(feature, {f: [n for _, n in parts] for f, parts in got.items() if any(n for _, n in parts)},
                  "stages", [ctx.profile_get(s)[1] for s in range(10)])
            assert sum(n for _, n in got[feature]) > 0, feature
            for other, parts in got.items():
                if other != feature and other not in runs_also:
                    assert parts == [(0.0, 0)] * len(parts), (feature, other, parts)
            for ms, n in got[feature]:
                assert n >= 0 and (n > 0 or ms == 0.0), (feature, got[feature])
            assert sum(ctx.profile_get(s)[1] for s in range(10)) > 0, feature   # the canny call in front of it
        for feature, (method, n_parts) in FEATURES.items():
            getattr(ctx, method)(n_parts - 1)
            with pytest.raises(hip.CannyHipError) as ei:
                getattr(ctx, method)(n_parts)
            assert ei.value.status == INVALID, feature
        ctx.profile_reset()
        for feature, parts in _read(ctx).items():
            assert parts == [(0.0, 0)] * len(parts), feature
        assert all(ctx.profile_get(s) == (0.0, 0) for s in range(10))


def test_every_slot_behind_the_polygons_follows_bit_30(hip):
    frame = synth_frame(H, W)
    calls = _calls(hip, frame)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 1 << 30)
        ctx.profile_reset()
        for feature in ("morph", "edgels", "components"):
            calls[feature][0](ctx)
        got = _read(ctx)
        counts = {f: [n for _, n in parts] for f, parts in got.items()}
        print(counts)
        assert sum(counts["morph"]) > 0 and sum(counts["edgels"]) > 0
        assert got["components"] == [(0.0, 0)] * 4
        assert all(ctx.profile_get(s) == (0.0, 0) for s in range(10))
        for other in set(FEATURES) - {"morph", "edgels"}:
            assert not any(counts[other]), other
