"""CPU-only: every feature's profile getter (canny_hip_<feature>_profile_get) refuses a null context and null outputs,
for every part it has and the first it has not, and the table below names every such getter the library exports.  No
kernel is launched and no GPU is needed: the getters check their arguments before they touch the device."""
import ctypes as C

import pytest

from canny_edge_amd import capi

INVALID = 1  # CANNY_HIP_ERR_INVALID

# getter -> the names of its parts.  Features whose parts capi names in a tuple use it; the others (one or two parts,
# named by single constants there) list them as include/canny_hip.h does.
GETTERS = {
    "canny_hip_hough_profile_get": capi.HOUGH_PARTS,
    "canny_hip_components_profile_get": capi.CC_PARTS,
    "canny_hip_edt_profile_get": capi.EDT_PARTS,
    "canny_hip_hough_segments_profile_get": capi.SEGMENT_PARTS,
    "canny_hip_contours_profile_get": capi.CONTOUR_PARTS,
    "canny_hip_hough_circles_profile_get": capi.CIRCLE_PARTS,
    "canny_hip_polygons_profile_get": capi.POLYGON_PARTS,
    "canny_hip_edgels_profile_get": ("layout", "refine"),
    "canny_hip_line_fits_profile_get": ("fit",),
    "canny_hip_circle_fits_profile_get": ("fit",),
    "canny_hip_chamfer_profile_get": capi.CHAMFER_PARTS,
    "canny_hip_shapes_profile_get": capi.SHAPE_PARTS,
    "canny_hip_curves_profile_get": capi.CURVE_PARTS,
    "canny_hip_corners_profile_get": capi.CORNER_PARTS,
    "canny_hip_descriptors_profile_get": capi.DESC_PARTS,
    "canny_hip_motion_profile_get": capi.MOTION_PARTS,
    "canny_hip_warp_profile_get": capi.WARP_PARTS,
    "canny_hip_fuse_profile_get": capi.FUSE_PARTS,
    "canny_hip_morph_profile_get": ("steps",),
}


def test_the_table_names_every_feature_getter():
    exported = {n for n in capi.EXPORTS if n.endswith("_profile_get")} - {"canny_hip_profile_get"}
    assert set(GETTERS) == exported
    assert (capi.EDGEL_PART_LAYOUT, capi.EDGEL_PART_REFINE) == (0, 1)
    assert capi.LINE_FIT_PART_FIT == 0 and capi.CIRCLE_FIT_PART_FIT == 0


@pytest.mark.parametrize("name", sorted(GETTERS))
def test_getter_refuses_null_context_and_null_outputs(name):
    fn = getattr(capi.load(), name)
    for part in range(-1, len(GETTERS[name]) + 1):
        ms, n = C.c_double(-1.0), C.c_long(-1)
        assert fn(None, part, C.byref(ms), C.byref(n)) == INVALID, (name, part, "null context")
        assert (ms.value, n.value) == (-1.0, -1), (name, part, "outputs written")
        assert fn(None, part, None, None) == INVALID, (name, part, "null context, null outputs")
        assert fn(None, part, None, C.byref(n)) == INVALID and fn(None, part, C.byref(ms), None) == INVALID
