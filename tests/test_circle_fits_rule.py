"""CPU-only checks of the circle-fit rule (include/canny_hip.h): the host function
canny_hip_circle_fits_from_plane against tests/circle_fits_rule.py word for word on empty, full, random and drawn masks,
the invariants of every record, the designed degenerate, trim-failed and invalid records, the statuses, the finishing
arithmetic of the host restatement against Python ints and against the exact rational solution, the accuracy of the
fitted centre on blurred disks, the -k grammar of the command line, and the host function under the host compiler's
sanitizers in a stand-alone program.  No GPU is needed."""
import itertools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import circle_fits_rule as cf
import oracle
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.int32(-0x5A5A5A5B)


def host(E, P, recs, band, trim_q8, options):
    """The host function's records; the buffer is exact-size inside the binding, so a guard goes around a second call."""
    return capi.circle_fits_from_plane(np.packbits(E, axis=-1), P, recs, band, trim_q8, options)


def check_invariants(recs, fit, band, trim_q8, options, untrimmed=None):
    """What every record keeps, from the words alone."""
    recs, fit = np.asarray(recs, np.int64).reshape(-1, 6), np.asarray(fit, np.int64).reshape(-1, 8)
    flags = fit[:, 4] & 0xFFFFFFFF
    assert not (flags & ~(cf.MAXD_MASK | cf.TRIM_FAILED | cf.DEGENERATE | cf.INVALID)).any()
    inv, deg, failed = (flags & cf.INVALID) != 0, (flags & cf.DEGENERATE) != 0, (flags & cf.TRIM_FAILED) != 0
    assert (flags[inv] == cf.INVALID).all() and not fit[inv][:, [0, 1, 2, 3, 5, 6, 7]].any()
    assert (flags[deg] == cf.DEGENERATE).all() and not fit[deg][:, 5:8].any()
    assert np.array_equal(fit[deg][:, 0:3], recs[deg][:, 0:3] * [32768, 32768, 65536]), "DEGENERATE: the Hough circle"
    assert (fit[:, 3] >= 0).all() and (fit[~deg & ~inv, 3] >= 3).all()
    if band == 0 and options == 0 and trim_q8 == 0:
        ok = ~inv
        assert np.array_equal(fit[ok, 3], recs[ok, 4]), "band = 0, options = 0, trim = 0: n == support"
    if trim_q8 == 0:
        assert not failed.any()
    good = ~deg & ~inv
    sdd = (fit[:, 6] & 0xFFFFFFFF) | (fit[:, 7] & 0xFFFFFFFF) << 32
    maxd = flags & cf.MAXD_MASK
    assert (maxd[good] ** 2 <= sdd[good]).all() and (sdd[good] <= fit[good, 3] * maxd[good] ** 2).all()
    assert ((fit[:, 5] & 0xFFFF) != 0)[good].all() and not (fit[:, 5] >> 16).any(), "sectors != 0 iff a fit with n > 0"
    assert (np.abs(fit[good, 0] - 32768 * recs[good, 0]) <= 65536 * (band + 2)).all()
    assert (np.abs(fit[good, 1] - 32768 * recs[good, 1]) <= 65536 * (band + 2)).all()
    if trim_q8 > 0:
        trimmed = good & ~failed
        if untrimmed is not None:
            first = np.asarray(untrimmed, np.int64).reshape(-1, 8)
            # The kept pixels have |d_q8| <= trim_q8 against the FIRST fit; maxd is taken against the SECOND (step 8: the
            # final fit), so maxd <= trim_q8 holds only up to how far the refit moved the circle: a point's distance
            # changes by at most the centre's move, the residual by that plus the radius's change, plus one unit for the
            # two roundings to 1/256 px.  (On a 3 x 5 frame the plain maxd <= trim_q8 does fail: 136 against 128.)
            move = np.hypot(fit[:, 0] - first[:, 0], fit[:, 1] - first[:, 1]) + np.abs(fit[:, 2] - first[:, 2])
            assert (maxd[trimmed] <= trim_q8 + np.ceil(move[trimmed] / 256.0) + 1).all()
            assert (fit[:, 3] <= first[:, 3]).all(), "n does not grow under the trim"
            same = failed | deg | inv
            assert np.array_equal(fit[same][:, [0, 1, 2, 3, 5, 6, 7]], first[same][:, [0, 1, 2, 3, 5, 6, 7]])


# ---- host function == rule ------------------------------------------------------------------------------------------------
SHAPES = [(3, 5), (97, 161), (40, 300), (300, 40)]
COMBOS = list(itertools.product(range(5), (0, 64, 128), range(4)))  # band, trim_q8, options: 60


def records_for(E, P, cell_shift, rng):
    """Hough records of the rule (low thresholds) plus caller-made ones all over and around the frame."""
    h, w = E.shape
    hi = max(1, min(45, min(h, w)))
    rec = cf.hough_records(E, P, 1 if h < 10 else 3, hi, cell_shift, 2, 3, 4, 5)
    made = np.zeros((5, 6), np.int32)
    made[:, 0], made[:, 1] = rng.integers(0, 2 * w, 5), rng.integers(0, 2 * h, 5)
    made[:, 2] = rng.integers(1, max(2, min(h, w) // 2 + 2), 5)
    made[0, :3] = (0, 0, 3)
    made[1, :3] = (2 * w - 1, 2 * h - 1, min(h, w))
    # the made records' support word: what the bin rule counts, so that the n == support invariant covers them too
    for r in made:
        r[4] = len(cf.band_pixels(E, r, 0))
    return np.concatenate([rec[:4], made]).astype(np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_equals_the_rule(shape):
    h, w = shape
    rng = np.random.default_rng(h * 7 + w)
    planes = [rng.integers(0, 256, shape).astype(np.uint8), rng.integers(-32768, 32768, shape).astype(np.int16)]
    # a third plane with structure, so that refined edgels and gated gradients occur on the drawn masks
    planes.append(cf.disk_plane(h, w, w / 2.0 + 0.25, h / 2.0 - 0.25, max(min(h, w) * 0.4, 1.0)))
    turn = itertools.cycle(COMBOS)
    seen, used = 0, set()
    for kind, E in cf.mask_kinds(h, w, 5).items():
        for P in planes:
            for cell_shift in range(3):
                recs = records_for(E, P, cell_shift, rng)
                for _ in range(2 if kind in ("all", "random") and h > 10 else 4):
                    band, trim_q8, options = next(turn)
                    want = cf.fits_of(E, P, recs, band, trim_q8, options)
                    got = host(E, P, recs, band, trim_q8, options)
                    assert got.dtype == np.int32 and got.shape == (len(recs), 8)
                    bad = np.flatnonzero((got != want).any(axis=1))
                    assert bad.size == 0, (f"{kind} shift {cell_shift} band {band} trim {trim_q8} options {options}: "
                                           f"{bad.size} differ, first {recs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}")
                    first = host(E, P, recs, band, 0, options) if trim_q8 else None
                    check_invariants(recs, got, band, trim_q8, options, first)
                    plain = host(E, P, recs, 0, 0, 0)
                    check_invariants(recs, plain, 0, 0, 0)
                    used.add((band, trim_q8, options))
                    seen += int(((got[:, 4].view(np.uint32) & (cf.DEGENERATE | cf.INVALID)) == 0).sum())
    assert len(used) == len(COMBOS), "every (band, trim, options) combination ran on this shape"
    assert seen > 0 or shape == (3, 5)


# ---- designed records ------------------------------------------------------------------------------------------------------
def test_designed_records():
    h, w = 48, 64
    flat = np.full((h, w), 77, np.uint8)  # no gradient: every edgel is its pixel's centre, unrefined
    rec = np.array([[40, 40, 10, 0, 0, 0]], np.int32)  # centre (20, 20), radius 10
    both = lambda E, P, r, *a: (host(E, P, r, *a), cf.fits_of(E, P, r, *a))
    # n = 0, 1, 2 and three collinear pixels (x = 30: d = 400 + (2y - 40)^2, bin 10 for y = 19, 20, 21)
    for pixels, n in (([], 0), ([(30, 20)], 1), ([(30, 20), (10, 20)], 2), ([(30, 19), (30, 20), (30, 21)], 3)):
        E = np.zeros((h, w), bool)
        for x, y in pixels:
            E[y, x] = True
        got, want = both(E, flat, rec, 0, 0, 0)
        assert np.array_equal(got, want)
        assert got[0].tolist() == [32768 * 40, 32768 * 40, 65536 * 10, n, cf.DEGENERATE, 0, 0, 0]
    # coincident edgels: pixels (29, 20) and (30, 20) refine to the same point (29.5, 20) on a step between them; with a
    # third pixel there are two distinct points: collinear, determinant 0
    E = np.zeros((h, w), bool)
    E[20, 29] = E[20, 30] = E[20, 10] = True
    step = np.zeros((h, w), np.uint8)
    step[:, 30:] = 200
    e = capi.edgels_from_plane(step, [20 * w + 29, 20 * w + 30])
    assert tuple(e[0, :2]) == tuple(e[1, :2]) == (256 * 29 + 128, 256 * 20)
    got, want = both(E, step, rec, 1, 0, 0)
    assert np.array_equal(got, want) and got[0, 3] == 3 and got[0, 4] == cf.DEGENERATE
    # a flat plane with GATE: no gradient, no pixel; without it the ring fits
    E = cf.ring(h, w, 20.0, 20.0, 10.0)
    for options in range(4):
        got, want = both(E, flat, rec, 1, 0, options)
        assert np.array_equal(got, want)
        assert (got[0, 3] == 0 and got[0, 4] == cf.DEGENERATE) == (options != 0)
    free = capi.circle_fits_unpack(host(E, flat, rec, 1, 0, 0))
    assert abs(free["centre"][0, 0] - 20.0) < 0.05 and abs(free["centre"][0, 1] - 20.0) < 0.05
    assert abs(free["radius"][0] - 10.0) < 0.25 and free["sector_count"][0] == 16 and free["rms"][0] < 0.4
    # a fit that runs out of band + 2: an arc of a circle of radius 60 about (20, -40) passes through the record's band
    E = cf.ring(h, w, 20.0, -40.0, 60.0, 60, 120)
    far = np.array([[40, 20, 10, 0, 0, 0]], np.int32)  # centre (20, 10), radius 10: the arc at y ~ 20 lies in its band
    uv = cf.used_pixels(E, flat, far[0], 2, 0)
    assert len(uv) >= 8
    m = cf.moments_of(uv, 10)
    A, B, C, P, Q = cf.centred(*m)
    exact_b = Fraction(A * Q - B * P, A * C - B * B)
    assert abs(exact_b) / 2 > 256 * (2 + 2), "the exact centre lies more than band + 2 pixels away"
    got, want = both(E, flat, far, 2, 0, 0)
    assert np.array_equal(got, want)
    assert got[0].tolist() == [32768 * 40, 32768 * 20, 65536 * 10, len(uv), cf.DEGENERATE, 0, 0, 0]
    # radius - band < 1: lo is 1, the centre pixel's own bin (d < 1) stays out
    E = np.ones((h, w), bool)
    small = np.array([[40, 40, 2, 0, 0, 0], [41, 41, 1, 0, 0, 0]], np.int32)
    P = np.random.default_rng(3).integers(0, 256, (h, w)).astype(np.uint8)
    for band in (2, 4):
        got, want = both(E, P, small, band, 0, 0)
        assert np.array_equal(got, want)
        assert got[0, 3] == len(cf.band_pixels(E, small[0], band)) == sum(
            1 <= (2 * x - 40) ** 2 + (2 * y - 40) ** 2 < (2 * (2 + band) + 1) ** 2 for x in range(w) for y in range(h))
    # TRIM_FAILED: pixel centres lie up to half a pixel off any circle; a trim of 1/256 px keeps too few of them
    E = cf.ring(h, w, 20.3, 20.1, 10.2)
    first = host(E, flat, rec, 1, 0, 0)
    got, want = both(E, flat, rec, 1, 1, 0)
    assert np.array_equal(got, want)
    assert got[0, 4].view(np.uint32) & cf.TRIM_FAILED and not got[0, 4].view(np.uint32) & cf.DEGENERATE
    assert np.array_equal(got[0, [0, 1, 2, 3, 5, 6, 7]], first[0, [0, 1, 2, 3, 5, 6, 7]])
    assert got[0, 4] == first[0, 4] | cf.TRIM_FAILED
    # ... and a trim that works: fewer pixels, every residual inside it against the first fit
    got, want = both(E, flat, rec, 1, 64, 0)
    assert np.array_equal(got, want) and 3 <= got[0, 3] < first[0, 3] and not got[0, 4] & cf.TRIM_FAILED


def test_invalid_records_and_statuses():
    h, w = 30, 48
    E = cf.ring(h, w, 24.0, 15.0, 9.0)
    P = np.random.default_rng(4).integers(0, 256, (h, w)).astype(np.uint8)
    ok_rec = [48, 30, 9, 1, 2, 3]
    recs = np.array([ok_rec, [48, 30, 0, 0, 0, 0], [48, 30, 1025, 0, 0, 0], [-1, 30, 9, 0, 0, 0], [2 * w, 30, 9, 0, 0, 0],
                     [48, -1, 9, 0, 0, 0], [48, 2 * h, 9, 0, 0, 0], [48, 30, -5, 0, 0, 0], [2 ** 31 - 1, 30, 9, 0, 0, 0],
                     [48, -2 ** 31, 9, 0, 0, 0], [2 * w - 1, 2 * h - 1, 1024, 0, 0, 0], [0, 0, 1, 0, 0, 0]], np.int64).astype(np.int32)
    for band, trim_q8, options in ((0, 0, 0), (4, 64, 3), (1, 0, 2)):
        got = host(E, P, recs, band, trim_q8, options)
        assert np.array_equal(got, cf.fits_of(E, P, recs, band, trim_q8, options))
        assert (got[1:10, 4].view(np.uint32) == cf.INVALID).all() and not got[1:10][:, [0, 1, 2, 3, 5, 6, 7]].any()
        assert not (got[[0, 10, 11], 4].view(np.uint32) & cf.INVALID).any()
    # statuses: nothing is written
    L, hp = capi.load(), capi._hp
    bits = np.packbits(E, axis=-1)
    out = np.full(8 * len(recs) + 16, SENT, np.int32)
    ok = [hp(bits), hp(P), 1, h, w, hp(recs), len(recs), 1, 0, 0, hp(out)]
    assert L.canny_hip_circle_fits_from_plane(*ok) == 0
    assert (out[8 * len(recs):] == SENT).all() and np.array_equal(out[:8 * len(recs)].reshape(-1, 8), host(E, P, recs, 1, 0, 0))
    for at, value, status in ((0, None, 1), (1, None, 1), (3, 1, 1), (4, 1, 1), (5, None, 1), (6, -1, 1), (7, -1, 1),
                              (7, 5, 2), (8, -1, 1), (9, 4, 1), (9, -1, 1), (10, None, 1), (3, 16385, 2), (4, 16385, 2)):
        a = list(ok)
        a[at] = value
        out[:] = SENT
        assert L.canny_hip_circle_fits_from_plane(*a) == status, (at, value)
        assert (out == SENT).all(), (at, value)
    assert L.canny_hip_circle_fits_from_plane(*ok[:7], 4, 1 << 30, 3, ok[10]) == 0  # the limits themselves are supported
    assert capi.circle_fits_from_plane(bits, P, np.zeros((0, 6), np.int32)).shape == (0, 8)
    assert capi.circle_fits_queue_capacity() >= 256


# ---- the finishing arithmetic ----------------------------------------------------------------------------------------------
def error_bound(m):
    """The header's bound on |move - 128 * exact| for both coordinates, as Fractions, or None where the rule is degenerate
    or the exact system is singular."""
    A, B, C, P, Q = cf.centred(*m[:9])
    s, a, b, c, det = cf.shifted(*m[:9])
    if m[0] < 3 or det <= 0 or A * C - B * B == 0:
        return None
    xa, xb = Fraction(P * C - Q * B, A * C - B * B), Fraction(A * Q - B * P, A * C - B * B)
    extra = (abs(xa) + abs(xb)) * 128 if s else 0
    return (xa, xb, Fraction(1, 2) + extra * Fraction(c + abs(b), det), Fraction(1, 2) + extra * Fraction(a + abs(b), det))


def test_finishing_arithmetic_against_python_ints_and_fractions():
    designed = cf.designed_moments()
    want = cf.finish_words(designed)
    got = capi.circle_fits_finish(cf.pack_moments(designed))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} sets differ, first {designed[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    # the designed sets are what they claim to be
    shifts = [cf.shifted(*m[:9])[0] for m in designed]
    assert min(shifts) == 0 and max(shifts) >= 39, "shifts of 0 and of the maximum the limits allow"
    assert max(abs(m[7]) for m in designed) >= 1 << 63, "Suz past 64 bits"
    assert max(m[0] for m in designed) >= (1 << 17) - 4
    dets = {cf.shifted(*m[:9])[4] for m in designed if m[0] >= 3}
    assert {0, 3, -3, -4} <= dets and any(d > 1 << 58 for d in dets), "the determinant is a multiple of n: 0, +n, -n"
    res = [cf.finish(*m) for m in designed]
    assert any(r[0] < 0 for r in res) and any(r[1] < 0 for r in res) and sum(r[2] for r in res) >= 10
    at_limit = [(m, r) for m, r in zip(designed, res) if m[0] == 3 and m[4] == 128 << 10]
    assert sorted({abs(r[0]) for _, r in at_limit if not r[2]}) == [65536 * (b + 2) for b in range(5)]
    assert sum(1 for _, r in at_limit if r[2]) == 10, "one unit beyond the limit is degenerate, either sign"
    halves = [r for m, r in zip(designed, res) if m[0] == 4 and m[4] == 256]
    assert [r[0] for r in halves] == [1, -1, 2, -2, 51, -51] and [r[1] for r in halves] == [-1, 1, -2, 2, -51, 51]
    # the centre against the exact rational solution, within the bound the header states
    checked = 0
    for m, r in zip(designed, res):
        eb = error_bound(m)
        if eb is None or r[2]:
            continue
        assert abs(r[0] - 128 * eb[0]) <= eb[2] and abs(r[1] - 128 * eb[1]) <= eb[3], m
        checked += 1
    assert checked >= 20
    # random point sets: the int64 restatement the GPU test uses == Python ints == the host function
    rnd = cf.random_moments(np.random.default_rng(23), 30000)
    sets = [tuple(x) for x in rnd.tolist()]
    want = cf.finish_np(rnd)
    assert np.array_equal(want, cf.finish_words(sets))
    assert np.array_equal(capi.circle_fits_finish(cf.pack_moments(sets)), want)
    assert (want[:, 3] == 0).mean() > 0.9
    for m, r in zip(sets[:3000], want[:3000].tolist()):
        eb = error_bound(m)
        if eb is not None and not r[3]:
            assert abs(r[0] - 128 * eb[0]) <= eb[2] and abs(r[1] - 128 * eb[1]) <= eb[3], m
    with pytest.raises(capi.CannyHipError):
        capi.circle_fits_finish(np.zeros((0, 12), np.int64))


def test_error_bound_on_shifted_systems():
    """Real point sets whose matrices need a shift: band pixels of large rings and short arcs on a random plane (so the
    edgels are scattered), the move compared with the exact solution of the unshifted system."""
    rng = np.random.default_rng(8)
    h, w = 300, 300
    P = rng.integers(0, 256, (h, w)).astype(np.uint8)
    checked = 0
    for r, a0, a1 in ((120, 0, 360), (120, 10, 60), (90, 100, 130), (140, 0, 25), (30, 0, 360)):
        E = cf.ring(h, w, 150.3, 149.8, r, a0, a1)
        uv = cf.used_pixels(E, P, (300, 300, r), 2, 0)
        m = cf.moments_of(uv, r) + (2,)
        s = cf.shifted(*m[:9])[0]
        mx, my, deg = cf.finish(*m)
        eb = error_bound(m)
        assert s > 0 and eb is not None
        if not deg:
            assert abs(mx - 128 * eb[0]) <= eb[2] and abs(my - 128 * eb[1]) <= eb[3]
            assert eb[2] < 1 and eb[3] < 1, "on real sets the shift costs less than half a unit of 1/65536 px"
            checked += 1
    assert checked >= 3


# ---- accuracy on blurred disks -----------------------------------------------------------------------------------------------
DISKS = [(6.4, 64.25, 48.4, 0), (8.3, 64.25, 48.4, 0), (12.6, 64.25, 48.4, 0), (12.6, 64.0, 48.15, 0),
         (20.3, 64.25, 48.4, 0), (20.3, 64.75, 48.9, 1), (30.7, 63.6, 47.9, 1), (30.7, 63.6, 47.9, 0),
         (40.2, 64.1, 48.3, 0), (20.3, 10.2, 48.4, 0), (25.5, 64.4, 2.3, 0)]  # R; cx, cy; cell_shift
TRIMS = (0, 64)
WORST_MEASURED = 0.0526  # px, the largest distance of a fitted centre from the true one over the cases (all reach n >= 16),
CAP = 1.5 * WORST_MEASURED  # measured with tests/circle_fits_rule.py (0.0525: R 20.3 clipped by the left border, trim 0; section 25)
ACCURACY = {}


def accuracy_case(disk, trim_q8):
    """(n, fitted centre error, Hough centre error, fitted radius - R, rms) of the case's first record, or None."""
    if (disk, trim_q8) in ACCURACY:
        return ACCURACY[(disk, trim_q8)]
    R, cx, cy, cell_shift = disk
    frame = cf.disk_plane(96, 128, cx, cy, R)
    E, P = oracle.canny(frame, 1.0, 50, 150) != 0, oracle.gaussian(frame, 1.0)
    recs = cf.hough_records(E, P, 5, 45, cell_shift, 20, 15, 10, 16)
    out = None
    if len(recs):
        want = cf.fits_of(E, P, recs[:1], 1, trim_q8, cf.REFINED_ONLY)
        got = host(E, P, recs[:1], 1, trim_q8, cf.REFINED_ONLY)
        assert np.array_equal(got, want)
        u = capi.circle_fits_unpack(got)
        if not (u["degenerate"][0] or u["invalid"][0]):
            out = (int(u["n"][0]), math.hypot(u["centre"][0, 0] - cx, u["centre"][0, 1] - cy),
                   math.hypot(recs[0, 0] / 2.0 - cx, recs[0, 1] / 2.0 - cy), float(u["radius"][0]) - R, float(u["rms"][0]))
    ACCURACY[(disk, trim_q8)] = out
    return out


@pytest.mark.parametrize("trim_q8", TRIMS)
@pytest.mark.parametrize("disk", DISKS, ids=lambda d: f"R{d[0]}-{d[1]}-{d[2]}-s{d[3]}")
def test_fitted_centre_lies_closer_to_the_truth_than_the_hough_centre(disk, trim_q8):
    """96 x 128 planes round(40 + 180 Phi((R - |p - c|) / 1.0)), sigma 1.0, thresholds 50 / 150, radii 5..45, circle
    threshold 20, support threshold 15, min_dist 10; band 1, REFINED_ONLY, trim 0 and 64; the first record of each case.
    For every case with n >= 16 the fitted centre lies less than half as far from the true centre as the Hough centre
    does, and below 1.5 x the worst value measured with the Python rule; |r - R| < 0.5 px."""
    r = accuracy_case(disk, trim_q8)
    if r is None:
        print(f"disk {disk} trim {trim_q8}: no fit")
        return
    n, fit, hough, dr, rms = r
    print(f"disk R {disk[0]:5.1f} at ({disk[1]}, {disk[2]}) shift {disk[3]} trim {trim_q8:3d}: n {n:3d} fit {fit:.4f} "
          f"hough {hough:.4f} ratio {fit / max(hough, 1e-9):.3f} r - R {dr:+.4f} rms {rms:.4f}")
    if n >= 16:
        assert fit < hough / 2
        assert fit < CAP
        assert abs(dr) < 0.5


def test_most_accuracy_cases_reach_sixteen_pixels():
    cases = [accuracy_case(d, t) for d in DISKS for t in TRIMS]
    reach = sum(1 for r in cases if r is not None and r[0] >= 16)
    assert 4 * reach >= 3 * len(cases), f"only {reach} of {len(cases)} cases have a fit with n >= 16"
    worst = max(r[1] for r in cases if r is not None and r[0] >= 16)
    assert worst <= WORST_MEASURED + 1e-4, f"the worst fitted centre is {worst:.4f} px: WORST_MEASURED is stale"


def test_dark_disks_give_the_same_maps_and_fits():
    R, cx, cy, cell_shift = DISKS[4]
    bright = cf.disk_plane(96, 128, cx, cy, R)
    dark = cf.disk_plane(96, 128, cx, cy, R, dark=220, step=-180)
    out = []
    for frame in (bright, dark):
        E, P = oracle.canny(frame, 1.0, 50, 150) != 0, oracle.gaussian(frame, 1.0)
        recs = cf.hough_records(E, P, 5, 45, cell_shift, 20, 15, 10, 16)
        out.append((E, recs, host(E, P, recs, 1, 0, cf.REFINED_ONLY)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


# ---- header, bindings, command line ------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1500
    assert capi.load().canny_hip_version() >= 1500
    for word in ("CANNY_HIP_CIRCLE_FIT_INTS 8", "CANNY_HIP_CIRCLE_FIT_GATE", "CANNY_HIP_CIRCLE_FIT_REFINED_ONLY",
                 "CANNY_HIP_CIRCLE_FIT_TRIM_FAILED 0x08000000u", "CANNY_HIP_CIRCLE_FIT_DEGENERATE 0x10000000u",
                 "CANNY_HIP_CIRCLE_FIT_INVALID 0x80000000u", "CANNY_HIP_CIRCLE_FIT_MAX_BAND 4",
                 "CANNY_HIP_CIRCLE_FIT_MAX_AXIS 16384", "CANNY_HIP_CIRCLE_FIT_PART_FIT", "halves away from zero",
                 "n == support", "restoring division", "2^18.01", "2^64.6", "det'", "belongs to the sector that STARTS"):
        assert word in header, word
    assert "circle refits" not in header, "the line fits' follow-up list no longer names it"
    for name in ("canny_hip_circle_fits_from_plane", "canny_hip_dev_circle_fits_bits", "canny_hip_dev_canny_hough_circle_fits",
                 "canny_hip_canny_hough_circle_fits", "canny_hip_dev_circle_fits_arith", "canny_hip_circle_fits_finish",
                 "canny_hip_circle_fits_profile_get", "canny_hip_circle_fits_queue_capacity"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert len(capi.PLAN_KINDS) == 18  # the fit kernel's grid has no cap, so there is no new launch plan
    assert (capi.CIRCLE_FIT_INTS, capi.CIRCLE_FIT_GATE, capi.CIRCLE_FIT_REFINED_ONLY) == (cf.FIT_INTS, cf.GATE, cf.REFINED_ONLY)
    assert (capi.CIRCLE_FIT_MAXD_MASK, capi.CIRCLE_FIT_TRIM_FAILED, capi.CIRCLE_FIT_DEGENERATE, capi.CIRCLE_FIT_INVALID) == (
        cf.MAXD_MASK, cf.TRIM_FAILED, cf.DEGENERATE, cf.INVALID)
    assert (capi.CIRCLE_FIT_MAX_BAND, capi.CIRCLE_FIT_MOMENT_WORDS) == (cf.MAX_BAND, cf.MOMENT_WORDS)


def test_unpack_helper():
    fit = np.array([[65536 * 3 + 32768, 65536 * 2, 65536 * 10 + 16384, 4, 64, 0xFFFF, 4 * 64 * 64, 0],
                    [0, 0, 0, 0, -(1 << 31), 0, 0, 0], [65536, 65536, 65536 * 5, 2, 1 << 28, 0, 0, 0],
                    [65536, 65536, 65536 * 5, 9, (1 << 27) | 128, 0x0111, 9 * 128 * 128, 0]], np.int64).astype(np.int32)
    u = capi.circle_fits_unpack(fit)
    assert np.array_equal(u["centre"][0], [3.5, 2.0]) and u["radius"][0] == 10.25 and u["n"][0] == 4
    assert u["rms"][0] == 0.25 and u["maxd"][0] == 0.25 and list(u["sector_count"]) == [16, 0, 0, 3]
    assert list(u["invalid"]) == [False, True, False, False] and list(u["degenerate"]) == [False, False, True, False]
    assert list(u["trim_failed"]) == [False, False, False, True] and u["rms"][3] == 0.5
    mine = cf.unpack(fit)
    assert np.array_equal(mine[0], u["centre"][:, 0]) and np.array_equal(mine[2], u["radius"])
    assert np.array_equal(mine[5], u["rms"]) and np.array_equal(mine[6], u["sector_count"])


def test_cli_k_grammar(tmp_path):
    """-k takes band,trim_q8[,options] and needs -r: without it, or with a band outside 0..4, a negative trim, options
    outside 0..3 or anything that is not whole integers, it is a usage error (exit 2) before any device is touched; with
    fewer than three positionals the usage text names it; nothing is written."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    run = lambda *a: subprocess.run([exe, *a, "-o", str(tmp_path)], capture_output=True, text=True, timeout=60)
    r = run("1.0", "50", "150", "-k", "1,0")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -k needs the circles of -r")
    r = run("1.0", "50", "150", "-l", "1,1,20", "-k", "1,0,2")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -k needs the circles of -r")
    for bad in ("1", "5,0", "-1,0", "1,-1", "1,0,4", "1,0,-1", "x", "1,x", "1,0,2,3", "", " 1,0", "1, 0", "1,0 ", "1,,0", "1,0,"):
        r = run("1.0", "50", "150", "-r", "5,45,20,15", "-k", bad)
        assert r.returncode == 2 and r.stderr.startswith("ERROR: -k expects band,trim_q8[,options]"), bad
    r = run("1.0", "50", "-r", "5,45,20,15", "-k", "1,64,2")
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-k band,trim_q8[,options]" in r.stderr
    assert "canny_circle_fits.txt" in r.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_circle_fits_host.cpp has its own main and is compiled together with csrc/canny_circle_fits_host.cpp
    and csrc/canny_edgels_host.cpp alone: nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_circle_fits_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_circle_fits_host.cpp"),
                           os.path.join(csrc, "canny_circle_fits_host.cpp"), os.path.join(csrc, "canny_edgels_host.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed frames ok" in r.stdout, r.stdout + r.stderr
