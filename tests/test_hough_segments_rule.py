"""canny_hip_hough_segments_from_bits -- the host-only walk of the Hough segment rule (include/canny_hip.h, DESIGN.md
section 16) -- against the numpy restatement of the rule (tests/hough_segments_rule.py), which looks at the full plane for
every line.  The numpy side is fed with the library's own vote tables; every comparison is exact equality on whole arrays,
and every output buffer is sentinel-filled with a guard behind it.  No GPU is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bits_inputs as bi
import hough_rule as hr
import hough_segments_rule as sr
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.int32(-0x5A5A5A5B)
N_GUARD = 64
LINES = 12


def _lines_of(mask, rho, theta, lo, hi, lines_max=LINES, threshold=0):
    """(bases of the strongest peaks of the mask, accumulator, numrho, tables)"""
    h, w = mask.shape
    numangle, numrho = capi.hough_geometry(h, w, rho, theta, lo, hi)
    tabs = capi.hough_tables(rho, theta, lo, numangle)
    acc = hr.accumulate(np.flatnonzero(mask), w, numrho, *tabs)
    return hr.peaks(acc, threshold)[0][:lines_max], acc, numrho, tabs


def _lib(mask, bases, rho, theta, lo, hi, min_length, max_gap, exclusive, cap):
    """The library's records in a guarded, sentinel-filled buffer: (rows written, true count)."""
    h, w = mask.shape
    buf = np.full(cap * 6 + N_GUARD, SENT, np.int32)
    got, count = capi.hough_segments_from_bits(np.packbits(mask, axis=-1), h, w, bases, rho, theta, lo, hi, min_length,
                                               max_gap, exclusive, segments_max=cap, out=buf)
    k = min(cap, count)
    assert got.shape == (k, 6)
    assert (buf[k * 6:] == SENT).all(), "slots past the count (or the guard) were written"
    return got.copy(), count


def _check(mask, bases, numrho, tabs, rho, theta, lo, hi, min_length, max_gap, exclusive, what):
    want = sr.segments(mask, bases, numrho, *tabs, min_length, max_gap, exclusive)
    got, count = _lib(mask, bases, rho, theta, lo, hi, min_length, max_gap, exclusive, max(len(want), 1) + 3)
    assert count == len(want), f"{what}: count {count} != {len(want)}"
    assert np.array_equal(got, want), f"{what}: records differ"
    return want


@pytest.mark.parametrize("rho", sr.RHOS)
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_walk_equals_the_rule(shape, rho):
    h, w = shape
    seen = 0
    for kind, mask in sr.mask_kinds(h, w, seed=h * 31 + w).items():
        for theta, lo, hi in sr.ANGLES:
            bases, _, numrho, tabs = _lines_of(mask, rho, theta, lo, hi)
            for min_length, max_gap in sr.parameter_sets(h, w):
                for exclusive in (0, 1):
                    what = f"{shape} {kind} rho={rho} theta={theta:.4f} [{lo:.2f},{hi:.2f}] {min_length}/{max_gap}/{exclusive}"
                    seen += len(_check(mask, bases, numrho, tabs, rho, theta, lo, hi, min_length, max_gap, exclusive, what))
    assert seen > 0


def test_pattern_features_at_the_chunk_borders():
    """One drawn row per pattern variant, the line through it alone: the segments are what the pattern says, worked out
    here in plain Python -- a gap of max_gap is bridged, max_gap + 1 splits, tb - ta = min_length is kept, one less is
    dropped, across positions 63 / 64 and 1023 / 1024."""
    h, w, y = 5, 1100, 2
    for variant in range(4):
        row = sr.pattern(w, variant)
        on = np.flatnonzero(row)
        runs, a = [], on[0]
        for p, q in zip(on, list(on[1:]) + [None]):
            if q is None or q - p - 1 > sr.MAX_GAP:
                if p - a >= sr.MIN_LENGTH:
                    runs.append((a, y, p, y, 0, int(row[a:p + 1].sum())))
                a = q
        border = 63 if variant < 2 else 1023
        bridged = [r for r in runs if r[0] < border < r[2]]
        assert len(bridged) == (1 if variant in (0, 2) else 0)
        other = 1023 if variant < 2 else 63
        assert len([r for r in runs if r[0] <= other < r[2]]) == (1 if variant in (0, 2) else 0)
        for mask in (np.zeros((h, w), bool), np.zeros((w, h), bool)):
            if mask.shape[0] == h:
                mask[y, :] = row
                want = np.array(runs, np.int32)
            else:
                mask[:, y] = row
                want = np.array(runs, np.int32)[:, [1, 0, 3, 2, 4, 5]]
            bases, acc, numrho, tabs = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi, lines_max=1)
            assert acc.ravel()[bases[0]] == row.sum()
            for exclusive in (0, 1):
                got, count = _lib(mask, bases, 1.0, np.pi / 180, 0.0, np.pi, sr.MIN_LENGTH, sr.MAX_GAP, exclusive, 64)
                assert count == len(want) and np.array_equal(got, want), (variant, mask.shape, exclusive)
                assert np.array_equal(sr.segments(mask, bases, numrho, *tabs, sr.MIN_LENGTH, sr.MAX_GAP, exclusive), want)


@pytest.mark.parametrize("shape,rho", [((97, 161), 1.0), ((64, 200), 2.5), ((120, 75), 0.5), ((40, 1100), 1.0)],
                         ids=lambda v: str(v))
def test_one_run_per_line_carries_the_cells_votes(shape, rho):
    """exclusive = 0, min_length = 0, max_gap = L: one segment per line with at least one vote, support = accum[base]."""
    h, w = shape
    mask = sr.drawn(h, w) | (np.random.default_rng(h + w).random(shape) < 0.01)
    bases, acc, numrho, tabs = _lines_of(mask, rho, np.pi / 180, 0.0, np.pi, lines_max=40)
    assert len(bases) == 40
    got, count = _lib(mask, bases, rho, np.pi / 180, 0.0, np.pi, 0, max(h, w), 0, 64)
    assert count == 40 and np.array_equal(got[:, 4], np.arange(40))
    assert np.array_equal(got[:, 5], acc.ravel()[bases])
    assert mask[got[:, 1], got[:, 0]].all() and mask[got[:, 3], got[:, 2]].all(), "an end point is not a set pixel"
    # a cell without votes gives nothing
    empty = np.flatnonzero(acc[1:-1, 1:-1].ravel() == 0)[:1]
    n, r = empty[0] // numrho, empty[0] % numrho
    none, zero = _lib(mask, np.array([(n + 1) * (numrho + 2) + r + 1], np.uint32), rho, np.pi / 180, 0.0, np.pi, 0, max(h, w),
                      0, 4)
    assert zero == 0 and len(none) == 0


def test_exclusive_mode_claims_pixels_once():
    h, w = 41, 61
    mask = np.zeros((h, w), bool)
    mask[20, :] = True   # the longer line claims the crossing pixel ...
    mask[:, 30] = True   # ... and splits the shorter one there
    bases, acc, numrho, tabs = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi, lines_max=2, threshold=30)
    assert list(acc.ravel()[bases]) == [61, 41]
    plain = sr.segments(mask, bases, numrho, *tabs, 0, 0, 0)
    excl = sr.segments(mask, bases, numrho, *tabs, 0, 0, 1)
    assert plain.tolist() == [[0, 20, 60, 20, 0, 61], [30, 0, 30, 40, 1, 41]]
    assert excl.tolist() == [[0, 20, 60, 20, 0, 61], [30, 0, 30, 19, 1, 20], [30, 21, 30, 40, 1, 20]]  # the rule alone
    for exclusive, want in ((0, plain), (1, excl)):
        got, count = _lib(mask, bases, 1.0, np.pi / 180, 0.0, np.pi, 0, 0, exclusive, 8)
        assert count == len(want) and np.array_equal(got, want)
    # a denser map, many lines: no pixel is counted twice
    mask = sr.drawn(97, 161) | (np.random.default_rng(9).random((97, 161)) < 0.05)
    bases, _, numrho, tabs = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi, lines_max=300)
    got, count = _lib(mask, bases, 1.0, np.pi / 180, 0.0, np.pi, 0, 2, 1, 4096)
    assert count == len(got) > 100 and got[:, 5].sum() <= mask.sum()
    assert np.array_equal(got, sr.segments(mask, bases, numrho, *tabs, 0, 2, 1))
    twice, _ = _lib(mask, bases, 1.0, np.pi / 180, 0.0, np.pi, 0, 2, 0, 4096)
    assert twice[:, 5].sum() > mask.sum()  # ... which the non-exclusive result does


@pytest.mark.parametrize("shape", bi.SHAPES[:4], ids=bi.SHAPE_IDS[:4])
def test_dirty_pad_bits_give_what_clean_ones_give(shape):
    """The padding bits of a row are ignored, whatever they hold: the shapes and masks of tests/test_gpu_bits_inputs.py
    (a line that ends on column w - 1, a vertical line on it), the pad bits all set and random.  The control first: the
    rule with the pad columns counted as pixels gives other records, so a walk that trusted a pad bit would show."""
    n, h, w = shape
    rb = bi.row_bytes(w)
    masks = bi.line_masks(n, h, w)
    for f, mask in enumerate(masks):
        bases, _, numrho, tabs = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi, lines_max=16, threshold=2 * h // 3 if w >= 9 else 1)
        assert len(bases) >= 1
        for exclusive in (0, 1):
            want = sr.segments(mask, bases, numrho, *tabs, 3, 1, exclusive)
            assert len(want) >= 1
            for pad in bi.PADS[1:]:
                bits = bi.packed(mask, pad, seed=h + f)
                assert bits.shape == (h, rb) and np.array_equal(bi.widened(bits)[:, :w], mask)
                wide = sr.segments(bi.widened(bits), bases, numrho, *tabs, 3, 1, exclusive)
                assert wide.shape != want.shape or not np.array_equal(wide, want), "the case cannot see a trusted pad bit"
                buf = np.full((len(want) + 3) * 6 + N_GUARD, SENT, np.int32)
                got, count = capi.hough_segments_from_bits(bits, h, w, bases, 1.0, np.pi / 180, 0.0, np.pi, 3, 1, exclusive,
                                                           segments_max=len(want) + 3, out=buf)
                what = f"{shape} frame {f} exclusive {exclusive} pad bits {pad}"
                assert count == len(want) and np.array_equal(got, want), what
                assert (buf[len(want) * 6:] == SENT).all(), what + ": slots past the count (or the guard) were written"


def test_bad_and_duplicate_bases_and_a_short_capacity():
    mask = sr.drawn(97, 161)
    good, _, numrho, tabs = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi, lines_max=3)
    numangle, stride = len(tabs[0]), numrho + 2
    bad = [0, stride - 1, stride, 2 * stride - 1, (numangle + 1) * stride + 5, (numangle + 2) * stride, 0xFFFFFFFF,
           0x80000000]  # border column / row cells and far beyond the accumulator
    bases = np.array([good[0], bad[0], good[1], good[0], *bad[1:], good[2], good[0]], np.uint32)
    for exclusive in (0, 1):
        want = _check(mask, bases, numrho, tabs, 1.0, np.pi / 180, 0.0, np.pi, 0, 1, exclusive, f"bad bases {exclusive}")
        assert set(want[:, 4].tolist()) <= {0, 2, 3, 11, 12} and 0 in want[:, 4]
        if exclusive == 0:  # duplicates are lines of their own
            assert np.array_equal(want[want[:, 4] == 0][:, [0, 1, 2, 3, 5]], want[want[:, 4] == 3][:, [0, 1, 2, 3, 5]])
        else:               # ... that find nothing left of what the first one kept
            assert not (want[:, 4] == 3).any() and not (want[:, 4] == 12).any()
        for cap in (1, len(want) - 1):
            got, count = _lib(mask, bases, 1.0, np.pi / 180, 0.0, np.pi, 0, 1, exclusive, cap)
            assert count == len(want) > cap and np.array_equal(got, want[:cap])
    none, zero = _lib(mask, np.empty(0, np.uint32), 1.0, np.pi / 180, 0.0, np.pi, 0, 0, 0, 4)
    assert zero == 0


def test_statuses_and_nothing_written():
    L = capi.load()
    mask = sr.drawn(20, 30)
    bits = np.packbits(mask, axis=-1)
    bases = _lines_of(mask, 1.0, np.pi / 180, 0.0, np.pi)[0]
    out = np.full(6 * 8 + N_GUARD, SENT, np.int32)
    count = C.c_int(-77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(bits=ptr(bits), h=20, w=30, rho=1.0, theta=np.pi / 180, lo=0.0, hi=np.pi, bases=ptr(bases), n=len(bases),
              ml=0, mg=0, ex=0, seg=ptr(out), cap=8, count=C.byref(count))

    def call(**kw):
        a = dict(ok, **kw)
        return L.canny_hip_hough_segments_from_bits(a["bits"], a["h"], a["w"], a["rho"], a["theta"], a["lo"], a["hi"],
                                                    a["bases"], a["n"], a["ml"], a["mg"], a["ex"], a["seg"], a["cap"],
                                                    a["count"])

    invalid = [dict(ml=-1), dict(mg=-1), dict(ex=2), dict(ex=-1), dict(cap=0), dict(cap=-5), dict(bits=None),
               dict(bases=None), dict(seg=None), dict(count=None), dict(n=-1), dict(h=0), dict(w=0),
               dict(rho=0.0), dict(rho=float("nan")), dict(theta=0.0), dict(theta=float("inf")), dict(lo=-0.1),
               dict(lo=1.0, hi=1.0), dict(hi=3.2)]
    for kw in invalid:
        assert call(**kw) == 1, kw  # CANNY_HIP_ERR_INVALID
        assert (out == SENT).all() and count.value == -77, kw
    unsupported = [dict(cap=(2 ** 31 + 5) // 6), dict(cap=2 ** 31 - 1)]  # 1 frame * segments_max * 6 >= 2^31
    for kw in unsupported:
        assert call(**kw) == 2, kw  # CANNY_HIP_ERR_UNSUPPORTED
        assert (out == SENT).all() and count.value == -77, kw
    assert call(cap=(2 ** 31 - 1) // 6 - 50, seg=ptr(out), n=0) == 0 and count.value == 0  # just below the limit
    assert call() == 0 and count.value > 0


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 900
    assert capi.load().canny_hip_version() >= 900
    assert re.search(r"#define CANNY_HIP_SEGMENT_INTS 6\b", header) and capi.SEGMENT_INTS == 6
    assert re.search(r"CANNY_HIP_STAGE_COUNT = 9,", header) and re.search(r"CANNY_HIP_STAGE_END = 10\b", header)
    names = ("canny_hip_hough_segments_from_bits", "canny_hip_dev_hough_segments_bits",
             "canny_hip_dev_canny_hough_segments", "canny_hip_canny_hough_segments",
             "canny_hip_hough_segments_profile_get")
    for name in names:
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(capi.load(), name)
    for method in ("dev_hough_segments_bits", "dev_canny_hough_segments", "canny_hough_segments",
                   "hough_segments_profile_get"):
        assert callable(getattr(capi.Context, method))
    assert callable(capi.hough_segments_from_bits)
