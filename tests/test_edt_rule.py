"""CPU-only: the distance-transform rule (tests/edt_rule.py) against its literal definition and against scipy, and the
library's host-only canny_hip_edt_from_bits against the rule.  Squared distances are integers and the float plane is a
correctly rounded root, so every comparison is exact; dist2, dist and nearest are asserted separately."""
import numpy as np
import pytest
from scipy import ndimage

import edt_rule as rule
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

SHAPES = [(1, 1), (1, 9), (9, 1), (3, 7), (5, 8), (7, 9), (64, 64), (65, 130), (130, 64), (257, 203), (37, 1001)]
DENSITIES = [0.0, 0.02, 0.1, 0.5, 0.9, 1.0]


def _random_mask(rng, h, w, density):
    return rng.random((h, w)) < density if density < 1.0 else np.ones((h, w), bool)


def _check_library(mask, what, pad_ones=False):
    h, w = mask.shape
    bits = np.packbits(mask, axis=-1)
    if pad_ones and w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want_d2, want_d, want_nn = rule.transform(mask)
    d2, d, nn = capi.edt_from_bits(bits, h, w)
    assert d2.dtype == np.int32 and np.array_equal(d2, want_d2), f"{what}: dist2 differs"
    assert d.dtype == np.float32 and d.tobytes() == want_d.tobytes(), f"{what}: dist differs"
    assert nn.dtype == np.int32 and np.array_equal(nn, want_nn), f"{what}: nearest differs"


def test_separable_equals_the_definition():
    rng = np.random.default_rng(2024)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 17), (17, 1), (2, 2), (40, 60), (33, 64), (23, 23)]
    shapes += [tuple(int(v) for v in rng.integers(1, 41, 2)) for _ in range(40)]
    for h, w in shapes:
        for density in DENSITIES:
            mask = _random_mask(rng, h, w, density)
            d2, nn = rule.separable(mask, band=7)
            want_d2, want_nn = rule.brute(mask, pairs_per_chunk=5000)
            assert np.array_equal(d2, want_d2), f"dist2 {(h, w)} density={density}"
            assert np.array_equal(nn, want_nn), f"nearest {(h, w)} density={density}"
    for h, w in ((9, 12), (12, 9), (21, 21)):
        for name, mask in rule.directed_masks_large(h, w).items():
            d2, nn = rule.separable(mask)
            want_d2, want_nn = rule.brute(mask)
            assert np.array_equal(d2, want_d2) and np.array_equal(nn, want_nn), f"{name} {(h, w)}"


def test_the_definition_on_known_answers():
    m = np.zeros((3, 5), bool)
    m[1, 1] = m[1, 3] = True
    d2, nn = rule.brute(m)
    assert d2.tolist() == [[2, 1, 2, 1, 2], [1, 0, 1, 0, 1], [2, 1, 2, 1, 2]]
    assert nn.tolist() == [[6, 6, 6, 8, 8], [6, 6, 6, 8, 8], [6, 6, 6, 8, 8]]        # column 2: the smaller index
    m = np.zeros((5, 3), bool)
    m[0, 1] = m[4, 1] = True
    assert rule.brute(m)[1][2].tolist() == [1, 1, 1]                                  # row 2: equally far, the upper pixel
    d2, nn = rule.brute(np.zeros((2, 3), bool))
    assert np.all(d2 == rule.NONE) and np.all(nn == -1)
    assert np.all(np.isposinf(rule.dist_of(d2))) and rule.dist_of(d2).dtype == np.float32


def _check_scipy(mask, d2, d, what):
    e, ind = ndimage.distance_transform_edt(~mask, return_indices=True)
    assert np.array_equal(np.rint(e * e).astype(np.int64), d2), f"{what}: dist2 differs from scipy"
    assert e.astype(np.float32).tobytes() == d.tobytes(), f"{what}: dist differs from scipy"
    return ind


def test_the_rule_against_scipy():
    rng = np.random.default_rng(7)
    for h, w in [(1, 1), (5, 8), (40, 60), (64, 64), (130, 203), (300, 400)]:
        for density in (0.001, 0.02, 0.1, 0.5, 0.9, 1.0):
            mask = _random_mask(rng, h, w, density)
            if not mask.any():
                mask[h // 2, w // 2] = True
            d2, d, nn = rule.transform(mask)
            ind = _check_scipy(mask, d2, d, f"{(h, w)} density={density}")
            # scipy names SOME nearest pixel: it must lie at the distance, it need not be the rule's
            r, c = np.indices(mask.shape)
            assert np.array_equal((r - ind[0]) ** 2 + (c - ind[1]) ** 2, d2) and mask[ind[0], ind[1]].all()
            assert np.array_equal((r - nn // w) ** 2 + (c - nn % w) ** 2, d2) and mask[nn // w, nn % w].all()


def test_library_and_scipy_on_a_4k_oracle_map():
    mask = oracle.canny(synth_frame(2160, 3840, 1), 1.4, 50, 150) != 0
    assert int(mask.sum()) == 62325
    d2, d, nn = capi.edt_from_bits(np.packbits(mask, axis=-1), 2160, 3840)
    _check_scipy(mask, d2, d, "4K")
    assert abs(float(d.max()) - 292.1) < 0.05
    r, c = np.indices(mask.shape)
    assert np.array_equal((r - nn // 3840) ** 2 + (c - nn % 3840) ** 2, d2) and mask[nn // 3840, nn % 3840].all()


def test_library_nearest_on_a_large_oracle_map():
    mask = oracle.canny(synth_frame(540, 960, 3), 1.4, 50, 150) != 0
    assert mask.any()
    _check_library(mask, "540x960 oracle map")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edt_from_bits_on_random_masks(shape):
    h, w = shape
    rng = np.random.default_rng(31 * h + w)
    for density in (0.002, 0.02, 0.1, 0.5, 0.9):
        _check_library(_random_mask(rng, h, w, density), f"{shape} density={density}")
        _check_library(_random_mask(rng, h, w, density), f"{shape} density={density}, dirty padding", pad_ones=True)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edt_from_bits_on_directed_masks(shape):
    h, w = shape
    for name, mask in rule.directed_masks_large(h, w).items():
        _check_library(mask, f"{name} {shape}")
        _check_library(mask, f"{name} {shape}, dirty padding", pad_ones=True)


@pytest.mark.parametrize("shape", [s for s in SHAPES if min(s) >= 2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_edt_from_bits_on_oracle_maps(shape):
    """The detector needs two rows and two columns; the one-row and one-column shapes are covered by the other masks."""
    h, w = shape
    for seed, (sigma, lo, hi) in enumerate([(1.4, 50, 150), (1.0, 1, 2), (0.6, 20, 60)]):
        mask = oracle.canny(synth_frame(h, w, 40 + seed), sigma, lo, hi) != 0
        _check_library(mask, f"oracle map {shape} sigma={sigma} thr=({lo},{hi})", pad_ones=True)


def test_the_tie_rule_by_hand():
    m = np.zeros((11, 9), bool)
    m[1, 4] = m[9, 4] = True                      # row 5 is equally far from both: the upper pixel, index 1 * 9 + 4
    d2, d, nn = capi.edt_from_bits(np.packbits(m, axis=-1), 11, 9)
    assert np.all(nn[5] == 13) and np.all(nn[:5] == 13) and np.all(nn[6:] == 9 * 9 + 4)
    assert d2[5].tolist() == [16 + (c - 4) ** 2 for c in range(9)]
    m = np.zeros((3, 9), bool)
    m[1, 2] = m[1, 6] = True                      # column 4 is equally far from both: the left pixel
    d2, d, nn = capi.edt_from_bits(np.packbits(m, axis=-1), 3, 9)
    assert np.all(nn[:, :5] == 11) and np.all(nn[:, 5:] == 15)
    assert d.dtype == np.float32 and d[0, 4] == np.float32(np.sqrt(5.0))


def test_every_combination_of_null_outputs():
    rng = np.random.default_rng(3)
    for mask in (rng.random((37, 53)) < 0.05, np.zeros((6, 10), bool)):
        h, w = mask.shape
        bits = np.packbits(mask, axis=-1)
        want = rule.transform(mask)
        for k in range(1, 8):
            flags = [bool(k & 1), bool(k & 2), bool(k & 4)]
            got = capi.edt_from_bits(bits, h, w, *flags)
            for name, asked, g, wnt in zip(("dist2", "dist", "nearest"), flags, got, want):
                assert (g is not None) == asked
                if asked:
                    assert g.tobytes() == wnt.tobytes(), f"{name} with outputs {flags}"
        with pytest.raises(capi.CannyHipError) as ei:
            capi.edt_from_bits(bits, h, w, False, False, False)
        assert ei.value.status == 1                # CANNY_HIP_ERR_INVALID


def test_sizes_out_of_range_give_the_documented_statuses():
    one = np.zeros(8, np.uint8)
    for h, w in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(capi.CannyHipError) as ei:
            capi.edt_from_bits(one, h, w)
        assert ei.value.status == 1, (h, w)        # CANNY_HIP_ERR_INVALID
    # height * width >= 2^31, and height^2 + width^2 >= 2^31 with a frame that would otherwise be fine: rejected before
    # anything is read or written (the buffers here are far too small for a call that went ahead)
    for h, w in ((65536, 32768), (46341, 1), (1, 46341), (32768, 32768), (40000, 30000)):
        assert h * w >= 2 ** 31 or h * h + w * w >= 2 ** 31
        out = np.full(4, 77, np.int32)
        st = capi.load().canny_hip_edt_from_bits(one.ctypes.data, h, w, out.ctypes.data, None, None)
        assert st == 2, (h, w)                     # CANNY_HIP_ERR_UNSUPPORTED
        assert np.all(out == 77)
    assert capi.load().canny_hip_edt_from_bits(None, 4, 4, one.ctypes.data, None, None) == 1


def test_version_and_constants():
    assert capi.load().canny_hip_version() >= 800
    assert capi.EDT_NONE == rule.NONE == 0x7FFFFFFF and capi.EDT_PARTS == ("rows", "columns")
