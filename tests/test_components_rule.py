"""Connected components, the part that needs no GPU: the numpy restatement of the rule (tests/components_rule.py) against
scipy.ndimage.label + find_objects, and the library's own host statement of the rule, canny_hip_components_from_bits,
against the numpy rule -- on random masks, on the oracle's edge maps and on directed masks.  Everything is integers: every
comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import components_rule as rule
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

SHAPES = [(1, 1), (1, 70), (70, 1), (2, 9), (9, 2), (64, 8), (37, 63), (40, 64), (33, 65), (50, 77), (66, 129), (130, 200)]
DENSITIES = [0.05, 0.2, 0.45, 0.6, 0.9]
MIN_AREAS = [0, 1, 2, 5, 20, 44]
GUARD = np.int32(0x5A5A5A5A)
N_GUARD = 32


def _mask(h, w, density, seed):
    return np.random.default_rng(seed).random((h, w)) < density


def _raw(bits, h, w, min_area, labels, stats, capacity):
    """The C entry point itself: (status, count)."""
    n = C.c_ulonglong(0xDEAD)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    st = capi.load().canny_hip_components_from_bits(ptr(bits), h, w, min_area, ptr(labels), ptr(stats), capacity,
                                                    C.byref(n))
    return st, n.value


def _check_lib(mask, min_area, what):
    h, w = mask.shape
    want_l, want_s = rule.components(mask, min_area)
    got_l, got_s, k = capi.components_from_bits(np.packbits(mask, axis=-1), h, w, min_area)
    assert k == want_s.shape[0], f"{what}: count"
    assert got_l.dtype == np.int32 and np.array_equal(got_l, want_l), f"{what}: labels"
    assert got_s.dtype == np.int32 and np.array_equal(got_s, want_s), f"{what}: stats"
    return want_l, want_s


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_numpy_rule_is_scipy_label(shape, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    h, w = shape
    m = _mask(h, w, density, 7 * h + w)
    labels, stats = rule.components(m, 1)
    ref, n = ndimage.label(m, structure=np.ones((3, 3)))
    assert stats.shape == (n, 6)
    assert np.array_equal(labels, ref), "numbering: ascending first pixel is scipy's order"
    for k, sl in enumerate(ndimage.find_objects(ref), start=1):
        box = (sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start)
        assert tuple(stats[k - 1, :4]) == box
        assert stats[k - 1, rule.AREA] == int((ref == k).sum())
        assert stats[k - 1, rule.FIRST] == int(np.flatnonzero(ref == k)[0])
    # the filter: dropping components and renumbering the rest in the same order
    for min_area in (2, 5):
        fl, fs = rule.components(m, min_area)
        keep = stats[:, rule.AREA] >= min_area
        assert np.array_equal(fs, stats[keep])
        renumber = np.zeros(n + 1, np.int32)
        renumber[1:][keep] = np.arange(1, int(keep.sum()) + 1)
        assert np.array_equal(fl, renumber[ref])


def test_numpy_rule_on_directed_masks_is_scipy_label():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, m in rule.directed_masks(200, 300).items():
        ref, n = ndimage.label(m, structure=np.ones((3, 3)))
        labels, stats = rule.components(m, 1)
        assert stats.shape[0] == n and np.array_equal(labels, ref), name


@pytest.mark.parametrize("min_area", MIN_AREAS + [10 ** 6])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_on_random_masks(shape, density, min_area):
    h, w = shape
    assert min_area <= 44 or min_area > h * w
    _check_lib(_mask(h, w, density, 7 * h + w), min_area, f"{shape} density={density} min_area={min_area}")


@pytest.mark.parametrize("min_area", MIN_AREAS + [480 * 640 + 1])
def test_host_function_on_the_oracles_map_of_a_synthetic_frame(min_area):
    edges = oracle.canny(synth_frame(480, 640, 1), 1.4, 50, 150) != 0
    _, all_stats = rule.components(edges, 1)
    assert all_stats.shape[0] == 419 and int(edges.sum()) == 2694 and all_stats[:, rule.AREA].max() == 43
    _, stats = _check_lib(edges, min_area, f"synth_frame min_area={min_area}")
    if min_area >= 44:
        assert stats.shape[0] == 0, "44 drops every component of this frame: the empty result"
    if min_area == 5:
        assert 0.3 < stats.shape[0] / 419 < 0.7


@pytest.mark.parametrize("thr", [(50, 150), (1, 1)], ids=lambda t: f"thr{t[0]}_{t[1]}")
@pytest.mark.parametrize("min_area", MIN_AREAS + [256 * 256 + 1])
def test_host_function_on_the_fixture_image(fixture_image, min_area, thr):
    edges = oracle.canny(np.ascontiguousarray(fixture_image), 1.4, *thr) != 0
    assert edges.any()
    _check_lib(edges, min_area, f"fixture thr={thr} min_area={min_area}")


@pytest.mark.parametrize("min_area", [1, 2, 20])
@pytest.mark.parametrize("shape", [(200, 300), (64, 8), (9, 2), (2, 9), (129, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_on_directed_masks(shape, min_area):
    h, w = shape
    for name, m in rule.directed_masks(h, w).items():
        _, stats = _check_lib(m, min_area, f"{name} {shape} min_area={min_area}")
        if min_area == 1 and h >= 9 and w >= 9:
            want = {"diagonal_pair": 1, "staircase": 1, "all_set": 1, "all_clear": 0, "spiral": 1, "serpentine": 1,
                    "combs": 2, "checkerboard": ((h + 1) // 2) * ((w + 1) // 2)}[name]
            assert stats.shape[0] == want, f"{name} {shape}"
        if name == "checkerboard":
            assert stats.shape[0] == 0 or (min_area <= 1 and np.all(stats[:, rule.AREA] == 1))


def test_serpentine_and_spiral_over_many_tiles():
    for m in (rule.serpentine(300, 400), rule.spiral(333)):
        _, stats = _check_lib(m, 1, "long path")
        assert stats.shape[0] == 1 and stats[0, rule.AREA] == int(m.sum())


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % 8], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padding_bits_are_not_pixels(shape):
    h, w = shape
    m = _mask(h, w, 0.4, 3 + w)
    bits = np.packbits(m, axis=-1)
    bits[:, -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want_l, want_s = rule.components(m, 1)
    got_l, got_s, k = capi.components_from_bits(bits, h, w, 1)
    assert k == want_s.shape[0] and np.array_equal(got_l, want_l) and np.array_equal(got_s, want_s)
    empty = np.zeros_like(bits)
    empty[:, -1] = np.uint8((1 << (8 - w % 8)) - 1)
    got_l, got_s, k = capi.components_from_bits(empty, h, w, 1)
    assert k == 0 and not got_l.any()


@pytest.mark.parametrize("min_area", [1, 3])
def test_capacity_bounds_the_records_never_the_count(min_area):
    h, w = 66, 129
    m = _mask(h, w, 0.3, 11)
    bits = np.packbits(m, axis=-1)
    want_l, want_s = rule.components(m, min_area)
    K = want_s.shape[0]
    assert K > 4
    for cap in (K, K - 1, K // 2, 1, 0, K + 7):
        stats = np.full((cap + N_GUARD) * 6, GUARD, np.int32)
        labels = np.full(h * w + N_GUARD, GUARD, np.int32)
        st, count = _raw(bits, h, w, min_area, labels, stats, cap)
        assert st == 0 and count == K, "the count is the true one, whatever fits"
        n = min(cap, K)
        assert np.array_equal(stats[:n * 6].reshape(n, 6), want_s[:n]), f"capacity={cap}: the prefix that fits is exact"
        assert np.all(stats[n * 6:] == GUARD), f"capacity={cap}: written past the records that fit"
        assert np.array_equal(labels[:h * w].reshape(h, w), want_l) and np.all(labels[h * w:] == GUARD)
        _, s, k = capi.components_from_bits(bits, h, w, min_area, capacity=cap)
        assert k == K and np.array_equal(s, want_s[:n])
    # counts only: no stats, no labels
    st, count = _raw(bits, h, w, min_area, None, None, 0)
    assert st == 0 and count == K
    # labels without stats
    labels = np.full(h * w + N_GUARD, GUARD, np.int32)
    st, count = _raw(bits, h, w, min_area, labels, None, 0)
    assert st == 0 and count == K and np.array_equal(labels[:h * w].reshape(h, w), want_l)
    assert np.all(labels[h * w:] == GUARD)


def test_invalid_arguments():
    bits, labels, stats = np.zeros(8, np.uint8), np.zeros(64, np.int32), np.zeros(6 * 64, np.int32)
    assert _raw(None, 8, 8, 1, labels, stats, 64)[0] == 1          # CANNY_HIP_ERR_INVALID
    assert _raw(bits, 0, 8, 1, labels, stats, 64)[0] == 1
    assert _raw(bits, 8, 0, 1, labels, stats, 64)[0] == 1
    assert _raw(bits, 8, 8, 1, labels, None, 4)[0] == 1             # a capacity without a buffer
    assert capi.load().canny_hip_components_from_bits(bits.ctypes.data_as(C.c_void_p), 8, 8, 1, None, None, 0, None) == 1


def test_header_publishes_the_record_layout():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "canny_hip.h")).read()
    assert re.search(r"#define CANNY_HIP_CC_STATS 6\b", header)
    for k, name in enumerate(("LEFT", "TOP", "WIDTH", "HEIGHT", "AREA", "FIRST")):
        assert re.search(rf"\bCANNY_HIP_CC_STAT_{name}\s*=\s*{k}\b", header), name
    assert (capi.CC_LEFT, capi.CC_TOP, capi.CC_WIDTH, capi.CC_HEIGHT, capi.CC_AREA, capi.CC_FIRST) == tuple(range(6))
    assert re.search(r"\bCANNY_HIP_STAGE_COUNT\s*=\s*9\b", header) and re.search(r"\bCANNY_HIP_STAGE_END\s*=\s*10\b", header)
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 700
