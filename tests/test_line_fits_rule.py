"""CPU-only checks of the line-fit rule (include/canny_hip.h): the host function
canny_hip_line_fits_from_plane against tests/line_fits_rule.py word for word on the drawn masks of the segment tests, the
degenerate and the invalid records, the invariants of every record, the finishing arithmetic of the host restatement
against Python ints, the accuracy of the fitted end points on blurred straight edges, the -f grammar of the command line,
and the host function under the host compiler's sanitizers in a stand-alone program.  No GPU is needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hough_rule as hr
import hough_segments_rule as sr
import line_fits_rule as lr
import oracle
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA = float(np.pi / 180)


def tables(h, w, rho, theta=THETA, min_theta=0.0, max_theta=float(np.pi)):
    na, nr = capi.hough_geometry(h, w, rho, theta, min_theta, max_theta)
    return (nr, *capi.hough_tables(rho, theta, min_theta, na))


def check_invariants(seg, fit, exclusive, options):
    """What every record keeps, from the words alone."""
    fit = np.asarray(fit, np.int64)
    flags = fit[:, 9] & 0xFFFFFFFF
    assert not (flags & ~(lr.MAXD_MASK | lr.DEGENERATE | lr.INVALID)).any()
    assert not (flags & lr.INVALID).any()
    deg = (flags & lr.DEGENERATE) != 0
    assert (fit[:, 8] >= 0).all() and (fit[~deg, 8] >= 2).all()
    if not exclusive and not options:
        assert np.array_equal(fit[:, 8], seg[:, 5]), "exclusive = 0, options = 0: n == support"
    elif not options:
        assert (fit[:, 8] >= seg[:, 5]).all()
    d = fit[deg]
    assert np.array_equal(d[:, 0:4], 65536 * seg[deg][:, 0:4]) and not d[:, [6, 7, 10, 11]].any()
    assert (flags[deg] == lr.DEGENERATE).all()
    empty = fit[:, 8] == 0
    assert np.array_equal(fit[empty][:, 4:6], 65536 * seg[empty][:, 0:2])
    g = fit[~deg]
    for r, s in zip(g.tolist(), seg[~deg].tolist()):
        dx, dy = r[6], r[7]
        assert abs(dx * dx + dy * dy - (1 << 60)) <= 1 << 32, "dx^2 + dy^2 is not within 2^-28 of 2^60"
        assert dx * (s[2] - s[0]) + dy * (s[3] - s[1]) >= 0, "the direction does not follow the record's order"
        # the end points at pmin <= 0 <= pmax from the centroid (pmin, pmax in 1/65536 px; the centroid rounds to 1/2 unit,
        # and each end point's two coordinates round by 1/2 unit each)
        p0 = ((r[0] - r[4]) * dx + (r[1] - r[5]) * dy) / float(1 << 30)
        p1 = ((r[2] - r[4]) * dx + (r[3] - r[5]) * dy) / float(1 << 30)
        assert p0 <= 2.0 and p1 >= -2.0 and p0 <= p1 + 2.0
        sdd = (r[10] & 0xFFFFFFFF) | (r[11] & 0xFFFFFFFF) << 32
        maxd = r[9] & lr.MAXD_MASK
        assert maxd * maxd <= sdd <= r[8] * maxd * maxd


def lines_of(mask, nr, tc, ts, rho, theta, threshold, lines_max, min_theta=0.0):
    acc = hr.accumulate(np.flatnonzero(mask.reshape(-1)), mask.shape[1], nr, tc, ts)
    return hr.lines(acc, threshold, lines_max, rho, theta, min_theta)[2]


# ---- host function == rule on the masks and parameter sets of the segment tests ------------------------------------------
CASES = [((3, 5), ("empty", "all", "random", "drawn"), 1.0, sr.ANGLES[0], 2),
         ((97, 161), ("empty", "all", "random", "drawn"), 1.0, sr.ANGLES[0], 25),
         ((97, 161), ("drawn",), 2.5, sr.ANGLES[1], 25),
         ((97, 161), ("drawn", "random"), 0.5, sr.ANGLES[2], 20),
         ((40, 1100), ("drawn",), 1.0, sr.ANGLES[0], 30),
         ((1100, 40), ("drawn",), 2.5, sr.ANGLES[0], 30)]


@pytest.mark.parametrize("shape,kinds,rho,angles,threshold", CASES,
                         ids=[f"{c[0][0]}x{c[0][1]}-rho{c[2]}-{i}" for i, c in enumerate(CASES)])
def test_host_function_equals_the_rule_on_the_segment_tests_masks(shape, kinds, rho, angles, threshold):
    h, w = shape
    theta, lo, hi = angles
    nr, tc, ts = tables(h, w, rho, theta, lo, hi)
    rng = np.random.default_rng(h * 7 + w)
    planes = [rng.integers(0, 256, shape).astype(np.uint8), rng.integers(-32768, 32768, shape).astype(np.int16)]
    masks = sr.mask_kinds(h, w, 3)
    seen = 0
    for kind in kinds:
        m = masks[kind]
        bits = np.packbits(m, axis=-1)
        bases = lines_of(m, nr, tc, ts, rho, theta, threshold, 6, lo)
        for min_length, max_gap in sr.parameter_sets(h, w):
            for exclusive in (0, 1):
                seg = sr.segments(m, bases, nr, tc, ts, min_length, max_gap, exclusive)
                got_seg, count = capi.hough_segments_from_bits(bits, h, w, bases, rho, theta, lo, hi, min_length, max_gap,
                                                               exclusive)
                assert count == len(seg) and np.array_equal(got_seg, seg)
                seg = seg[:40]  # the plain-Python rule on a prefix of the long lists of min_length = 0
                for P in planes:
                    for options in range(4):
                        want = lr.line_fits(m, P, bases, nr, tc, ts, seg, options)
                        got = capi.line_fits_from_plane(bits, P, bases, seg, rho, theta, lo, hi, options)
                        assert got.dtype == np.int32 and got.shape == (len(seg), 12)
                        bad = np.flatnonzero((got != want).any(axis=1))
                        assert bad.size == 0, (f"{kind} {min_length},{max_gap} exclusive {exclusive} options {options}: "
                                               f"{bad.size} differ, first {seg[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}")
                        check_invariants(seg, got, exclusive, options)
                        seen += len(seg)
    assert seen > 0 or shape == (3, 5)


def test_degenerate_records():
    h, w = 30, 48
    nr, tc, ts = tables(h, w, 1.0)
    m = np.zeros((h, w), bool)
    m[12, 4:44] = True
    bits = np.packbits(m, axis=-1)
    bases = lines_of(m, nr, tc, ts, 1.0, THETA, 30, 1)
    assert len(bases) == 1
    rng = np.random.default_rng(2)
    P = rng.integers(0, 256, (h, w)).astype(np.uint8)
    # single-pixel segments: min_length = 0 on a dotted line, n = 1
    dots = np.zeros((h, w), bool)
    dots[12, 4:44:4] = True
    seg = sr.segments(dots, bases, nr, tc, ts, 0, 0, 0)
    assert len(seg) == 10 and (seg[:, 5] == 1).all()
    got = capi.line_fits_from_plane(np.packbits(dots, axis=-1), P, bases, seg)
    assert np.array_equal(got, lr.line_fits(dots, P, bases, nr, tc, ts, seg, 0))
    assert (got[:, 8] == 1).all() and (got[:, 9].view(np.uint32) == lr.DEGENERATE).all()
    e = capi.edgels_from_plane(P, seg[:, 1] * w + seg[:, 0])
    assert np.array_equal(got[:, 4:6], 256 * e[:, 0:2]), "n = 1: the centroid is the edgel"
    check_invariants(seg, got, 0, 0)
    # a segment whose every pixel the gate removes: gradients ALONG the segment (a plane that varies with x only)
    seg = sr.segments(m, bases, nr, tc, ts, 5, 0, 0)
    ramp = np.tile((5 * np.arange(w)).astype(np.uint8), (h, 1))
    got = capi.line_fits_from_plane(bits, ramp, bases, seg, options=lr.GATE)
    assert np.array_equal(got, lr.line_fits(m, ramp, bases, nr, tc, ts, seg, lr.GATE))
    assert got[0, 8] == 0 and got[0, 9].view(np.uint32) == lr.DEGENERATE and tuple(got[0, 4:6]) == (65536 * 4, 65536 * 12)
    assert capi.line_fits_from_plane(bits, ramp, bases, seg)[0, 8] == 40
    # a flat plane with the gate: no gradient at all; without it every edgel is a pixel centre and the fit is the row
    flat = np.full((h, w), 77, np.int16)
    for options in range(4):
        got = capi.line_fits_from_plane(bits, flat, bases, seg, options=options)
        assert np.array_equal(got, lr.line_fits(m, flat, bases, nr, tc, ts, seg, options))
        assert (got[0, 8] == 40) == (options == 0)
    free = capi.line_fits_unpack(capi.line_fits_from_plane(bits, flat, bases, seg))
    assert np.array_equal(free["p0"], [[4.0, 12.0]]) and np.array_equal(free["p1"], [[43.0, 12.0]])
    assert np.array_equal(free["direction"], [[1.0, 0.0]]) and free["rms"][0] == 0 and free["maxd"][0] == 0
    # two coincident edgels: pixels (10, 12) and (11, 12) whose refined positions meet halfway (t = +128 and t = -128)
    two = np.zeros((h, w), bool)
    two[12, 10:12] = True
    tie = np.zeros((h, w), np.uint8)
    tie[:, 11:] = 200
    e = capi.edgels_from_plane(tie, [12 * w + 10, 12 * w + 11])
    assert tuple(e[0, :2]) == tuple(e[1, :2]) == (256 * 10 + 128, 256 * 12)
    rec = np.array([[10, 12, 11, 12, 0, 2]], np.int32)
    got = capi.line_fits_from_plane(np.packbits(two, axis=-1), tie, bases, rec)
    assert np.array_equal(got, lr.line_fits(two, tie, bases, nr, tc, ts, rec, 0))
    assert got[0, 8] == 2 and got[0, 9].view(np.uint32) == lr.DEGENERATE and tuple(got[0, 4:6]) == (65536 * 10 + 32768, 65536 * 12)


def test_invalid_records_and_statuses():
    h, w = 30, 48
    nr, tc, ts = tables(h, w, 1.0)
    m = np.zeros((h, w), bool)
    m[12, 4:44] = True
    m[3:27, 20] = True
    bits = np.packbits(m, axis=-1)
    cell = lambda n, x, y: (n + 1) * (nr + 2) + int(sr.vote_plane(h, w, tc[n], ts[n], nr)[y, x]) + 1
    bases = np.array([cell(90, 4, 12), cell(0, 20, 3)], np.uint32)  # the horizontal line, the vertical line
    P = np.random.default_rng(4).integers(0, 256, (h, w)).astype(np.uint8)
    not_cells = np.concatenate([bases, [0, nr + 1, 2 * (nr + 2) - 1, 181 * (nr + 2) + 5, 2 ** 32 - 1]]).astype(np.uint32)
    hz, vt = [4, 12, 43, 12], [20, 3, 20, 26]
    k_h = 0
    seg = np.array([hz + [k_h, 41], vt + [1 - k_h, 25],                                   # valid
                    hz + [len(not_cells), 0], hz + [-1, 0], hz + [2 ** 31 - 1, 0],        # k outside the list
                    *[hz + [2 + i, 0] for i in range(5)],                                  # bases that are no cells
                    [4, 12, w, 12, k_h, 0], [4, h, 43, 12, k_h, 0], [-1, 12, 43, 12, k_h, 0], [4, 12, 43, -1, k_h, 0],
                    [43, 12, 4, 12, k_h, 0], [20, 26, 20, 3, 1 - k_h, 0]], np.int64).astype(np.int32)  # outside; ta > tb
    want = lr.line_fits(m, P, not_cells, nr, tc, ts, seg, 0)
    got = capi.line_fits_from_plane(bits, P, not_cells, seg)
    assert np.array_equal(got, want)
    assert (got[2:, 9].view(np.uint32) == lr.INVALID).all() and not got[2:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11]].any()
    assert not (got[:2, 9].view(np.uint32) & (lr.INVALID | lr.DEGENERATE)).any()
    # x0 == x1 on the x-major line is valid (ta == tb), whatever the order of y
    one = np.array([[30, 20, 30, 2, k_h, 0]], np.int32)
    assert np.array_equal(capi.line_fits_from_plane(bits, P, bases, one), lr.line_fits(m, P, bases, nr, tc, ts, one, 0))
    # statuses
    L, hp = capi.load(), capi._hp
    out = np.zeros(12, np.int32)
    ok = [hp(bits), hp(P), 1, h, w, 1.0, len(tc), nr, hp(tc), hp(ts), hp(bases), len(bases), hp(seg), 1, 0, hp(out)]
    assert L.canny_hip_line_fits_from_plane(*ok) == 0
    for at, value, status in ((0, None, 1), (1, None, 1), (3, 1, 1), (4, 1, 1), (8, None, 1), (10, None, 1), (12, None, 1),
                              (14, 4, 1), (14, -1, 1), (15, None, 1), (5, 8.5, 2), (3, 16385, 2), (4, 16385, 2), (5, 0.0, 1)):
        a = list(ok)
        a[at] = value
        assert L.canny_hip_line_fits_from_plane(*a) == status, (at, value)
    assert L.canny_hip_line_fits_from_plane(*ok[:5], 8.0, *ok[6:]) == 0  # the limits themselves are supported
    assert capi.line_fits_from_plane(bits, P, [], np.zeros((0, 6), np.int32)).shape == (0, 12)


# ---- the finishing arithmetic ----------------------------------------------------------------------------------------------
def test_finishing_arithmetic_against_python_ints():
    designed = lr.designed_moments()
    sets = np.array(designed, dtype=object).astype(np.int64)
    want = np.array([lr.finish_words(m) for m in designed], np.int64).astype(np.int32)
    got = capi.line_fits_finish(sets)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} sets differ, first {designed[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    # the designed sets are what they claim to be
    big = (1 << 22) + 128
    assert max(m[3] for m in designed) == (1 << 18) * big * big < 1 << 63
    steps = [(m, lr.finish(*m)) for m in designed]
    assert sum(1 for _, f in steps if f[4]) >= 5 and any(f[2] < 0 for _, f in steps) and any(f[3] < 0 for _, f in steps)
    roots = set()
    for m in designed:
        n, su, sv, suu, suv, svv = m[:6]
        A, B, C = n * suu - su * su, n * suv - su * sv, n * svv - sv * sv
        if max(A, C, abs(B)) < 1 << 28:  # s = 0
            v = (A - C) ** 2 + 4 * B * B
            r = math.isqrt(v)
            roots |= {("square", r * r == v), ("below", (r + 1) ** 2 - 1 == v), ("above", r * r + 1 == v and r > 1),
                      ("negative D, E = 0", A < C and B == 0), ("negative E", B < 0), ("large", v > 1 << 57)}
    assert {k for k, hit in roots if hit} == {"square", "below", "above", "negative D, E = 0", "negative E", "large"}
    # random point sets: the int64 restatement the GPU test uses == Python ints == the host function
    rnd = lr.random_moments(np.random.default_rng(23), 30000)
    want = lr.finish_np(rnd)
    assert np.array_equal(want, np.array([lr.finish_words(m) for m in rnd.tolist()], np.int64).astype(np.int32))
    assert np.array_equal(capi.line_fits_finish(rnd), want)
    assert (want[:, 5] == 0).mean() > 0.99
    with pytest.raises(capi.CannyHipError):
        capi.line_fits_finish(np.zeros((0, 8), np.int64))


# ---- accuracy on blurred straight edges ----------------------------------------------------------------------------------
# The true line is x cos(a) + y sin(a) = d with d = an integer + phase: the phase is the line's offset from the rho grid, so
# for an on-grid angle the Hough cell's own line is min(phase, 1 - phase) away.  0.25 and 0.4 are a quarter of a cell and
# nearly the worst case of half a cell; a phase near 0 would make the cell's line exact and the comparison meaningless.
ON_GRID = [0.0, 90.0, 30.0, 60.0, 120.0, 150.0, 7.0, 173.0]
OFF_GRID = [a + 0.3 for a in (0.0, 7.0, 30.0, 60.0, 90.0, 120.0, 150.0, 172.0)]
PHASES = (0.25, 0.4)
WORST_MEASURED = 0.1882  # px, the largest distance of a fitted end point from the true line over the cases with n >= 16,
CAP = 1.5 * WORST_MEASURED  # measured with tests/line_fits_rule.py (60.0 degrees, phase 0.4); DESIGN.md section 24 has the table
ACCURACY = {}


def accuracy_case(angle, phase):
    """(n, fit, cell, pixel, angular error in degrees) of the case's segment with the largest n, or None: the largest
    distance from the true line of the two fitted end points, of the Hough cell's own line at the same two places (the
    end points projected onto it), and of the record's whole-pixel end points."""
    if (angle, phase) in ACCURACY:
        return ACCURACY[(angle, phase)]
    H, W = 96, 128
    nr, tc, ts = tables(H, W, 1.0)
    t = math.radians(angle)
    ct, st = math.cos(t), math.sin(t)
    dist = round(W / 2 * ct + H / 2 * st) + phase
    frame = lr.soft(lr.halfplane(H, W, angle, dist))
    E, P = oracle.canny(frame, 1.0, 50, 150) != 0, oracle.gaussian(frame, 1.0)
    bases, _, seg, want = lr.pipeline(E, P, nr, tc, ts, 1.0, THETA, 15, 8, 10, 3, 0, 0)
    out = None
    if len(seg):
        got = capi.line_fits_from_plane(np.packbits(E, axis=-1), P, bases, seg)
        assert np.array_equal(got, want)
        u = capi.line_fits_unpack(got)
        j = int(np.argmax(u["n"]))
        line_rho, line_theta = (float(v) for v in hr.line_of(bases[seg[j, 4]], nr, 1.0, THETA))
        cc, cs = math.cos(line_theta), math.sin(line_theta)
        off = lambda p: abs(p[0] * ct + p[1] * st - dist)
        ends = (u["p0"][j], u["p1"][j])
        on_cell = [(p[0] - (p[0] * cc + p[1] * cs - line_rho) * cc, p[1] - (p[0] * cc + p[1] * cs - line_rho) * cs) for p in ends]
        a = math.degrees(math.atan2(u["direction"][j][1], u["direction"][j][0])) - (angle + 90.0)
        out = (int(u["n"][j]), max(off(p) for p in ends), max(off(p) for p in on_cell),
               max(off(seg[j, 0:2]), off(seg[j, 2:4])), abs((a + 90.0) % 180.0 - 90.0))
    ACCURACY[(angle, phase)] = out
    return out


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("angle", ON_GRID + OFF_GRID)
def test_fitted_end_points_lie_closer_to_the_edge_than_the_cells_line(angle, phase):
    """96 x 128 planes round(40 + 180 Phi(d / 1.0)), sigma 1.0, thresholds 50 / 150, rho 1, theta 1 degree, Hough threshold
    15, min_length 10, max_gap 3.  For every case whose fit has n >= 16 the fitted end points lie less than half as far
    from the true line as the Hough cell's own line does at the same places, and below 1.5 x the worst value measured with
    the Python rule (0.1882 px -> 0.2823 px).  Measured: the ratio cell / fit lies between 2.2 and 273, the fit between
    0.0012 and 0.188 px, the angular error between 0.0000 and 0.35 degrees."""
    r = accuracy_case(angle, phase)
    if r is None:
        print(f"angle {angle} phase {phase}: no segment")
        return
    n, fit, cell, pixel, ang = r
    print(f"angle {angle:6.1f} phase {phase}: n {n:3d} fit {fit:.4f} cell {cell:.4f} pixel ends {pixel:.4f} "
          f"ratio {cell / max(fit, 1e-9):.1f} angular error {ang:.4f} deg")
    if n >= 16:
        assert fit < cell / 2
        assert fit < CAP


def test_most_accuracy_cases_reach_sixteen_pixels():
    cases = [accuracy_case(a, p) for a in ON_GRID + OFF_GRID for p in PHASES]
    reach = sum(1 for r in cases if r is not None and r[0] >= 16)
    assert 4 * reach >= 3 * len(cases), f"only {reach} of {len(cases)} cases have a fit with n >= 16"


# ---- header, bindings, command line ------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1400
    assert capi.load().canny_hip_version() >= 1400
    for word in ("CANNY_HIP_LINE_FIT_INTS 12", "CANNY_HIP_LINE_FIT_GATE", "CANNY_HIP_LINE_FIT_REFINED_ONLY",
                 "CANNY_HIP_LINE_FIT_DEGENERATE", "CANNY_HIP_LINE_FIT_INVALID", "CANNY_HIP_LINE_FIT_PART_FIT", "2^37",
                 "halves away from zero", "n == support", "n may exceed", "2^22.01", "Sdd < ", "16384"):
        assert word in header, word
    for name in ("canny_hip_line_fits_from_plane", "canny_hip_dev_line_fits_bits", "canny_hip_dev_canny_hough_line_fits",
                 "canny_hip_canny_hough_line_fits", "canny_hip_dev_line_fits_arith", "canny_hip_line_fits_profile_get",
                 "canny_hip_line_fits_finish"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert len(capi.PLAN_KINDS) == 18  # the fit kernel's grid has no cap, so there is no new launch plan
    assert (capi.LINE_FIT_INTS, capi.LINE_FIT_GATE, capi.LINE_FIT_REFINED_ONLY) == (lr.FIT_INTS, lr.GATE, lr.REFINED_ONLY)
    assert (capi.LINE_FIT_MAXD_MASK, capi.LINE_FIT_DEGENERATE, capi.LINE_FIT_INVALID) == (lr.MAXD_MASK, lr.DEGENERATE, lr.INVALID)


def test_unpack_helper():
    fit = np.array([[65536, 2 * 65536, 3 * 65536 + 32768, 2 * 65536, 2 * 65536, 2 * 65536, 1 << 30, 0, 4, 64, 4 * 64 * 64, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0, -(1 << 31), 0, 0], [0, 0, 65536, 0, 0, 0, 0, 0, 1, 1 << 28, 0, 0]], np.int64)
    u = capi.line_fits_unpack(fit.astype(np.int32))
    assert np.array_equal(u["p0"][0], [1.0, 2.0]) and np.array_equal(u["p1"][0], [3.5, 2.0])
    assert np.array_equal(u["direction"][0], [1.0, 0.0]) and u["n"][0] == 4 and u["rms"][0] == 0.25 and u["maxd"][0] == 0.25
    assert list(u["invalid"]) == [False, True, False] and list(u["degenerate"]) == [False, False, True]
    mine = lr.unpack(fit.astype(np.int32))
    assert all(np.array_equal(u[k], mine[k]) for k in u)


def test_cli_f_grammar(tmp_path):
    """-f takes the options and needs -l and -g: without them, or with anything but 0..3, it is a usage error (exit 2)
    before any device is touched; with fewer than three positionals the usage text names it; nothing is written."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    run = lambda *a: subprocess.run([exe, *a, "-o", str(tmp_path)], capture_output=True, text=True, timeout=60)
    r = run("1.0", "50", "150", "-f", "1")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -f needs the segments of -l")
    r = run("1.0", "50", "150", "-l", "1,1,20", "-f", "1")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -f needs the segments of -l")
    for bad in ("4", "-1", "x", "1,2", "", " 1", "1 "):
        r = run("1.0", "50", "150", "-l", "1,1,20", "-g", "5,2", "-f", bad)
        assert r.returncode == 2 and r.stderr.startswith("ERROR: -f expects options"), bad
    r = run("1.0", "50", "-l", "1,1,20", "-g", "5,2", "-f", "3")
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-f options" in r.stderr
    assert "canny_line_fits.txt" in r.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_line_fits_host.cpp has its own main and is compiled together with csrc/canny_line_fits_host.cpp and
    csrc/canny_edgels_host.cpp alone: nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_line_fits_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_line_fits_host.cpp"),
                           os.path.join(csrc, "canny_line_fits_host.cpp"), os.path.join(csrc, "canny_edgels_host.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed frames ok" in r.stdout, r.stdout + r.stderr
