"""CPU-only checks of the contour rule: tests/contours_rule.py against properties that do not use
a border follower's state at all, and the library's host function canny_hip_contours_from_bits against the rule.  No
kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import components_rule as cr
import contours_rule as rule
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.int32(0x5A5A5A5A)
GUARD64 = np.uint64(0xEEEEEEEEEEEEEEEE)
N_GUARD = 32
SHAPES = [(37, 53), (9, 2), (2, 9), (64, 8), (120, 1001)]
MIN_AREAS = [1, 5, 20]


def _mask(h, w, density, seed):
    return np.random.default_rng(seed).random((h, w)) < density


def _outline_blobs(h, w, seed):
    """Thin outlines of random blobs: the boundary pixels of a union of discs."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    solid = np.zeros((h, w), bool)
    for _ in range(6):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 10)
        solid |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    p = np.pad(solid, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return solid & ~inner


# ---- properties that do not depend on the follower ------------------------------------------------------------------
def _exterior_border(component):
    """Pixels of `component` (bool, one component alone) with a 4-neighbour in the exterior background: the component
    padded by one pixel, the 4-connected region of unset cells that contains the pad."""
    p = np.pad(component, 1)
    ext = np.zeros_like(p)
    ext[0, :] = ext[-1, :] = ext[:, 0] = ext[:, -1] = True
    while True:
        grown = ext.copy()
        grown[1:, :] |= ext[:-1, :]
        grown[:-1, :] |= ext[1:, :]
        grown[:, 1:] |= ext[:, :-1]
        grown[:, :-1] |= ext[:, 1:]
        grown &= ~p
        if np.array_equal(grown, ext):
            break
        ext = grown
    near = ext[:-2, 1:-1] | ext[2:, 1:-1] | ext[1:-1, :-2] | ext[1:-1, 2:]
    return component & near


def _moore_clockwise(mask, first):
    """Moore-neighbour tracing, clockwise, from (p0, backtrack W); stops when the move p0 -> p1 is about to recur.
    Returns [p0, p1, ...] without the closing p0."""
    h, w = mask.shape
    ring = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]   # clockwise from W

    def is_set(y, x):
        return 0 <= y < h and 0 <= x < w and mask[y, x]

    p0 = (first // w, first % w)
    cur, back = p0, 0        # back: ring position of the backtrack cell relative to cur
    seq, p1 = [p0], None
    while True:
        for i in range(1, 9):
            k = (back + i) % 8
            ny, nx = cur[0] + ring[k][0], cur[1] + ring[k][1]
            if is_set(ny, nx):
                break
        else:
            return [first]
        prev_k = (k - 1) % 8                                  # the last unset cell examined: the next backtrack
        by, bx = cur[0] + ring[prev_k][0], cur[1] + ring[prev_k][1]
        nxt = (ny, nx)
        if cur == p0:
            if p1 is None:
                p1 = nxt
            elif nxt == p1:
                break
        seq.append(nxt)
        back = ring.index((by - ny, bx - nx))
        cur = nxt
    assert seq[-1] == p0
    return [y * w + x for y, x in seq[:-1]]


def _check_properties(mask, what):
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    labels, stats = cr.components(mask, 1)
    got_stats, chains = rule.contours(mask, 1)
    assert np.array_equal(got_stats, stats)
    for k, (rec, ch) in enumerate(zip(stats, chains), 1):
        tag = f"{what}: component {k}"
        assert ch[0] == rec[cr.FIRST] and ch.size <= 8 * rec[cr.AREA], tag
        y, x = ch // w, ch % w
        if ch.size > 1:
            dy, dx = np.abs(np.roll(y, -1) - y), np.abs(np.roll(x, -1) - x)
            assert np.all(np.maximum(dy, dx) == 1), f"{tag}: consecutive pixels are distinct 8-neighbours, cyclically"
        else:
            assert rec[cr.AREA] == 1, tag
        comp = labels == k
        border = np.flatnonzero(_exterior_border(comp))
        assert np.array_equal(np.unique(ch), border), f"{tag}: the chain as a set is the exterior border"
        moore = _moore_clockwise(comp, int(rec[cr.FIRST]))
        assert ch.tolist() == moore[:1] + moore[:0:-1], f"{tag}: the reverse of the clockwise Moore trace"
    return stats, chains


@pytest.mark.parametrize("density", [0.05, 0.2, 0.4, 0.6, 0.9])
def test_properties_on_random_maps(density):
    for seed in range(3):
        _check_properties(_mask(37, 53, density, 100 * seed + int(density * 100)), f"density={density} seed={seed}")


@pytest.mark.parametrize("shape", [(64, 72), (9, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_properties_on_directed_masks(shape):
    h, w = shape
    for name, m in cr.directed_masks(h, w).items():
        stats, chains = _check_properties(m, f"{name} {shape}")
        if shape == (64, 72) and name == "all_set":
            assert len(chains) == 1 and chains[0].size == 2 * (64 + 72) - 4
        if shape == (64, 72) and name == "checkerboard":
            assert len(chains) == 1152 and all(c.size == 1 for c in chains)


def test_properties_on_thin_outlines():
    for seed in range(4):
        _check_properties(_outline_blobs(48, 60, seed), f"outlines seed={seed}")


def test_the_serpentine_is_walked_out_and_back():
    m = cr.serpentine(256, 256)
    stats, chains = rule.contours(m, 1)
    assert int(m.sum()) == 32896 and len(chains) == 1 and chains[0].size == 65535
    assert np.array_equal(np.unique(chains[0]), np.flatnonzero(m))


# ---- the host function against the rule --------------------------------------------------------------------------------
def _raw(bits, h, w, min_area, stats, cap, chain, points, pcap, count=True, point_count=True):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    k, n = C.c_ulonglong(77), C.c_ulonglong(77)
    st = capi.load().canny_hip_contours_from_bits(ptr(bits), h, w, min_area, ptr(stats), cap,
                                                  C.byref(k) if count else None, ptr(chain), ptr(points), pcap,
                                                  C.byref(n) if point_count else None)
    return st, k.value, n.value


def _check_lib(mask, min_area, what, bits=None):
    h, w = mask.shape
    want = rule.csr(mask[None], min_area)
    bits = np.packbits(mask, axis=-1) if bits is None else bits
    stats, chain, points, k, n = capi.contours_from_bits(bits, h, w, min_area)
    assert k == want[0].shape[0] and n == want[3].size, f"{what}: the counts"
    assert np.array_equal(stats, want[0]), f"{what}: stats differ"
    assert chain.dtype == np.uint64 and np.array_equal(chain, want[2]), f"{what}: chain_offsets differ"
    assert points.dtype == np.int32 and np.array_equal(points, want[3]), f"{what}: points differ"
    return want


@pytest.mark.parametrize("min_area", MIN_AREAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_matches_the_rule(shape, min_area):
    h, w = shape
    for density in (0.05, 0.4, 0.9):
        m = _mask(h, w, density, 7 * h + w + int(density * 100))
        _check_lib(m, min_area, f"{shape} density={density} min_area={min_area}")
        if w % 8:   # padding bits set: they are not pixels
            bits = np.packbits(m, axis=-1)
            bits[:, -1] |= np.uint8((1 << (8 - w % 8)) - 1)
            _check_lib(m, min_area, f"{shape} density={density} min_area={min_area}, padding set", bits=bits)


@pytest.mark.parametrize("shape", [(64, 72), (9, 2), (2, 9), (130, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_on_directed_masks(shape):
    h, w = shape
    for name, m in cr.directed_masks(h, w).items():
        for min_area in (1, 2):
            _check_lib(m, min_area, f"{name} {shape} min_area={min_area}")


def test_host_function_on_the_long_serpentine():
    want = _check_lib(cr.serpentine(256, 256), 1, "serpentine")
    assert want[3].size == 65535


@pytest.mark.parametrize("min_area", [1, 3])
def test_capacities_bound_the_writes_never_the_counts(min_area):
    h, w = 66, 129
    m = _mask(h, w, 0.3, 11)
    bits = np.packbits(m, axis=-1)
    want_s, _, want_c, want_p, _ = rule.csr(m[None], min_area)
    K, P = want_s.shape[0], want_p.size
    assert K > 4 and P > K
    long_chain = int(np.argmax(np.diff(want_c)))
    mid = int(want_c[long_chain]) + int(want_c[long_chain + 1] - want_c[long_chain]) // 2   # lands inside a chain
    assert want_c[long_chain] < mid < want_c[long_chain + 1]
    for cap in (K, K - 1, 1, 0, K + 7):
        for pcap in (P, mid, 1, 0, P + 9):
            stats = np.full((cap + N_GUARD) * 6, GUARD, np.int32)
            chain = np.full(cap + 1 + N_GUARD, GUARD64, np.uint64)
            points = np.full(pcap + N_GUARD, GUARD, np.int32)
            st, k, n = _raw(bits, h, w, min_area, stats, cap, chain, points, pcap)
            what = f"capacity={cap} point_capacity={pcap}"
            assert st == 0 and k == K and n == P, f"{what}: the counts are the true ones"
            fit = min(cap, K)
            assert np.array_equal(stats[:fit * 6].reshape(fit, 6), want_s[:fit]) and np.all(stats[fit * 6:] == GUARD), what
            assert np.array_equal(chain[:fit + 1], want_c[:fit + 1]), f"{what}: chain_offsets"
            assert np.all(chain[fit + 1:] == GUARD64), f"{what}: written past the chain offsets that exist"
            pfit = min(pcap, int(want_c[fit]))
            assert np.array_equal(points[:pfit], want_p[:pfit]), f"{what}: the prefix that fits is exact"
            assert np.all(points[pfit:] == GUARD), f"{what}: written past the points that fit"
            s, c, p, k, n = capi.contours_from_bits(bits, h, w, min_area, capacity=cap, point_capacity=pcap)
            assert (k, n) == (K, P) and np.array_equal(s, want_s[:fit]) and np.array_equal(c, want_c[:fit + 1])
            assert np.array_equal(p, want_p[:pfit])
    # counts only
    st, k, n = _raw(bits, h, w, min_area, None, 0, None, None, 0)
    assert st == 0 and k == K and n == P
    # stats may be NULL at any capacity
    chain = np.full(K + 1, GUARD64, np.uint64)
    points = np.full(P + N_GUARD, GUARD, np.int32)
    st, k, n = _raw(bits, h, w, min_area, None, K, chain, points, P)
    assert st == 0 and np.array_equal(chain, want_c) and np.array_equal(points[:P], want_p)
    assert np.all(points[P:] == GUARD)


def test_invalid_arguments():
    bits = np.zeros(8, np.uint8)
    stats, chain, points = np.zeros(6 * 64, np.int32), np.zeros(65, np.uint64), np.zeros(64, np.int32)
    assert _raw(bits, 8, 8, 1, stats, 64, chain, points, 64)[0] == 0
    assert _raw(None, 8, 8, 1, stats, 64, chain, points, 64)[0] == 1          # CANNY_HIP_ERR_INVALID
    assert _raw(bits, 0, 8, 1, stats, 64, chain, points, 64)[0] == 1
    assert _raw(bits, 8, 0, 1, stats, 64, chain, points, 64)[0] == 1
    assert _raw(bits, 8, 8, 1, stats, 64, None, points, 64)[0] == 1           # a capacity without chain_offsets
    assert _raw(bits, 8, 8, 1, stats, 64, chain, None, 64)[0] == 1            # a point_capacity without points
    assert _raw(bits, 8, 8, 1, stats, 64, chain, points, 64, count=False)[0] == 1
    assert _raw(bits, 8, 8, 1, stats, 64, chain, points, 64, point_count=False)[0] == 1
    # the frame size these calls support: 2^28 pixels
    assert _raw(bits, 1 << 14, (1 << 14) + 1, 1, None, 0, None, None, 0)[0] == 2   # CANNY_HIP_ERR_UNSUPPORTED


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1000
    assert capi.load().canny_hip_version() >= 1000
    assert re.search(r"CANNY_HIP_STAGE_COUNT = 9,", header) and re.search(r"CANNY_HIP_STAGE_END = 10\b", header)
    for k, name in enumerate(("LABEL", "COUNT", "WRITE", "STATS")):
        assert re.search(rf"\bCANNY_HIP_CONTOUR_PART_{name}\s*=\s*{k}\b", header), name
    assert len(capi.CONTOUR_PARTS) == 4
    names = ("canny_hip_dev_canny_contours", "canny_hip_dev_contours_bits", "canny_hip_canny_contours",
             "canny_hip_contours_from_bits", "canny_hip_contours_profile_get")
    for name in names:
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(capi.load(), name)
    for method in ("canny_contours", "dev_canny_contours", "dev_contours_bits", "contours_profile_get"):
        assert callable(getattr(capi.Context, method))
    assert "contour chains (cv::findContours)" not in header
