"""Edge point lists, the host-only part: canny_hip_points_from_bits turns one packed bit map (rows MSB-first, padded to
bytes -- numpy.packbits(mask, axis=-1), the layout of canny_hip_canny_batch_bits) into the ascending pixel indices
r * width + c of its set pixels, which is np.flatnonzero(mask) and the reference's own index convention
(src/utils.cpp:360-427: pixel (r,c) at r*width+c).  No GPU is needed and no kernel is launched."""
import ctypes as C

import numpy as np
import pytest

from canny_edge_amd import capi

SHAPES = [(1, 1), (2, 9), (9, 2), (37, 53), (64, 8), (120, 1001), (270, 480)]
DENSITIES = [0.0, 0.03, 0.5, 1.0]
GUARD = 0xA5A5A5A5


def _mask(h, w, density, seed):
    rng = np.random.default_rng(seed)
    return rng.random((h, w)) < density  # density 0.0 -> all clear, 1.0 -> all set


def _raw(bits, h, w, points, capacity):
    """The C entry point itself: (status, count)."""
    n = C.c_ulonglong(0xDEAD)
    st = capi.load().canny_hip_points_from_bits(
        bits.ctypes.data_as(C.c_void_p) if bits is not None else None, h, w,
        points.ctypes.data_as(C.c_void_p) if points is not None else None, capacity, C.byref(n))
    return st, n.value


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_points_equal_flatnonzero(shape, density):
    h, w = shape
    m = _mask(h, w, density, 1000 * h + w)
    got = capi.points_from_bits(np.packbits(m, axis=-1), h, w)
    assert got.dtype == np.uint32
    assert np.array_equal(got, np.flatnonzero(m))
    assert got.size == int(m.sum())


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % 8])
def test_padding_bits_are_not_pixels(shape):
    h, w = shape
    m = _mask(h, w, 0.3, 77 + w)
    bits = np.packbits(m, axis=-1)
    bits[:, -1] |= np.uint8((1 << (8 - w % 8)) - 1)  # every padding bit of every row set
    assert np.array_equal(capi.points_from_bits(bits, h, w), np.flatnonzero(m))
    # and padding alone is an empty list
    empty = np.zeros_like(bits)
    empty[:, -1] = np.uint8((1 << (8 - w % 8)) - 1)
    assert capi.points_from_bits(empty, h, w).size == 0


@pytest.mark.parametrize("shape", [(37, 53), (120, 1001)])
def test_capacity_below_the_count_gives_the_exact_prefix(shape):
    h, w = shape
    m = _mask(h, w, 0.5, 5 + h)
    bits = np.packbits(m, axis=-1)
    want = np.flatnonzero(m).astype(np.uint32)
    for cap in (want.size - 1, want.size // 2, 1, 0):
        buf = np.full(cap + 64, GUARD, np.uint32)
        st, count = _raw(bits, h, w, buf, cap)
        assert st == 0
        assert count == want.size, "the count is the true one, whatever fits"
        assert np.array_equal(buf[:cap], want[:cap])
        assert np.all(buf[cap:] == GUARD), "nothing is written at or past points + capacity"
        pts, n = capi.points_from_bits(bits, h, w, capacity=cap)
        assert n == want.size and np.array_equal(pts, want[:cap])
    # room to spare: the words after the list stay untouched too
    buf = np.full(want.size + 64, GUARD, np.uint32)
    st, count = _raw(bits, h, w, buf, want.size + 64)
    assert st == 0 and count == want.size
    assert np.array_equal(buf[:want.size], want) and np.all(buf[want.size:] == GUARD)


def test_counts_only_call():
    m = _mask(64, 70, 0.1, 9)
    st, count = _raw(np.packbits(m, axis=-1), 64, 70, None, 0)
    assert st == 0 and count == int(m.sum())


def test_invalid_arguments():
    bits = np.zeros(8, np.uint8)
    pts = np.zeros(64, np.uint32)
    assert _raw(None, 8, 8, pts, 64)[0] == 1          # CANNY_HIP_ERR_INVALID
    assert _raw(bits, 0, 8, pts, 64)[0] == 1
    assert _raw(bits, 8, 0, pts, 64)[0] == 1
    assert _raw(bits, -1, 8, pts, 64)[0] == 1
    assert _raw(bits, 8, 8, None, 4)[0] == 1           # a capacity without a buffer
    assert capi.load().canny_hip_points_from_bits(bits.ctypes.data_as(C.c_void_p), 8, 8, None, 0, None) == 1


@pytest.mark.parametrize("shape", SHAPES)
def test_points_to_rc_round_trips(shape):
    h, w = shape
    m = _mask(h, w, 0.2, 31 * h + w)
    pts = capi.points_from_bits(np.packbits(m, axis=-1), h, w)
    rows, cols = capi.points_to_rc(pts, w)
    r, c = np.nonzero(m)
    assert np.array_equal(rows, r) and np.array_equal(cols, c)
    assert np.array_equal(rows * w + cols, pts)
    back = np.zeros((h, w), bool)
    back[rows, cols] = True
    assert np.array_equal(back, m)


def test_header_publishes_the_compact_stage():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "canny_hip.h")).read()
    assert re.search(r"\bCANNY_HIP_STAGE_COMPACT\s*=\s*9\b", header)
    assert re.search(r"\bCANNY_HIP_STAGE_END\s*=\s*10\b", header)
    assert capi.STAGE_COMPACT == 9
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 500
