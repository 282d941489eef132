"""CPU-only checks of the colour -> gray contract (include/canny_hip.h, "gray_rule"): the two integer rules over every
(R,G,B) triple, the layout helper of the Python binding, and the names the header publishes.  No kernel runs here."""
import os
import re

import numpy as np
import pytest

from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "canny_hip.h")

# (wb, wg, wr, shift) of rule 0 (OpenCV cvtColor *2GRAY on CV_8U) and rule 1 (PIL convert('L'))
RULES = {0: (1868, 9617, 4899, 14), 1: (7471, 38470, 19595, 16)}


def gray(rgb, rule):
    """numpy reference: (..., 3) uint8 R,G,B -> gray uint8 = (wb B + wg G + wr R + 2^(s-1)) >> s."""
    wb, wg, wr, s = RULES[rule]
    c = np.asarray(rgb).astype(np.uint32)
    return ((wb * c[..., 2] + wg * c[..., 1] + wr * c[..., 0] + (1 << (s - 1))) >> s).astype(np.uint8)


@pytest.fixture(scope="module")
def all_triples():
    """All 2^24 (R,G,B) triples, R major, as a 4096 x 4096 RGB image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.empty((1 << 24, 3), np.uint8)
    rgb[:, 0] = v >> 16
    rgb[:, 1] = (v >> 8) & 0xFF
    rgb[:, 2] = v & 0xFF
    return rgb.reshape(4096, 4096, 3)


def test_rule1_equals_pil_on_every_triple(all_triples):
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(all_triples, "RGB").convert("L"))
    assert np.array_equal(gray(all_triples, 1), want)


def test_rule0_is_the_opencv_formula_and_the_rules_differ_on_39135_triples(all_triples):
    c = all_triples.astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    opencv = ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)  # CV_DESCALE(.., yuv_shift = 14)
    g0 = gray(all_triples, 0)
    assert np.array_equal(g0, opencv)
    assert int((g0 != gray(all_triples, 1)).sum()) == 39135


def test_rules_stay_in_24_bits_and_map_white_to_255():
    for wb, wg, wr, s in RULES.values():
        assert wb + wg + wr == 1 << s
        assert 255 * max(wb, wg, wr) < 1 << 24 and 255 * (wb + wg + wr) + (1 << (s - 1)) < 1 << 24
        assert (255 * (wb + wg + wr) + (1 << (s - 1))) >> s == 255


@pytest.mark.parametrize("shape,order,batch,want", [
    ((480, 640), "bgr", False, capi.LAYOUT_GRAY8),
    ((480, 640), "rgb", False, capi.LAYOUT_GRAY8),
    ((480, 640, 3), "bgr", False, capi.LAYOUT_BGR8),
    ((480, 640, 3), "rgb", False, capi.LAYOUT_RGB8),
    ((480, 640, 4), "bgr", False, capi.LAYOUT_BGRA8),
    ((480, 640, 4), "rgb", False, capi.LAYOUT_RGBA8),
    ((8, 480, 640), "bgr", True, capi.LAYOUT_GRAY8),
    ((8, 480, 640, 3), "bgr", True, capi.LAYOUT_BGR8),
    ((8, 480, 640, 3), "rgb", True, capi.LAYOUT_RGB8),
    ((8, 480, 640, 4), "bgr", True, capi.LAYOUT_BGRA8),
    ((8, 480, 640, 4), "rgb", True, capi.LAYOUT_RGBA8),
])
def test_layout_of(shape, order, batch, want):
    assert capi.layout_of(shape, order, batch=batch) == want
    assert capi.LAYOUT_CHANNELS[want] == (shape[-1] if len(shape) - batch == 3 else 1)


@pytest.mark.parametrize("shape,order,batch", [
    ((480, 640, 2), "bgr", False), ((480, 640, 5), "bgr", False), ((480,), "bgr", False), ((1, 2, 3, 3), "bgr", False),
    ((480, 640, 3), "BGR", False), ((480, 640, 3), "hsv", False), ((8, 480, 640, 1), "rgb", True), ((480, 640), "bgr", True),
])
def test_layout_of_rejects(shape, order, batch):
    with pytest.raises(ValueError):
        capi.layout_of(shape, order, batch=batch)


def test_header_publishes_layouts_options_and_stage():
    h = open(HEADER).read()
    for name, value, py in (("CANNY_HIP_GRAY8", 0, capi.LAYOUT_GRAY8), ("CANNY_HIP_BGR8", 1, capi.LAYOUT_BGR8),
                            ("CANNY_HIP_RGB8", 2, capi.LAYOUT_RGB8), ("CANNY_HIP_BGRA8", 3, capi.LAYOUT_BGRA8),
                            ("CANNY_HIP_RGBA8", 4, capi.LAYOUT_RGBA8), ("CANNY_HIP_STAGE_TO_GRAY", 8, capi.STAGE_TO_GRAY),
                            ("CANNY_HIP_STAGE_COUNT", 9, len(capi.STAGE_NAMES))):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", h), name
        assert py == value, name
    for opt in ('"gray_rule"', '"fuse_gray"', '"last_canny_fused_gray"'):
        assert opt in h, opt
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", h).group(1)) >= 300
    assert capi.STAGE_NAMES[capi.STAGE_TO_GRAY] == "to_gray"
