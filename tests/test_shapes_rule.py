"""CPU-only checks of the shape rule: tests/shapes_rule.py against closed forms, an independent
exact integration and properties that need no hull algorithm at all; the library's host function
canny_hip_shapes_from_chains against the rule word for word; the grammar of the CLI's -u flag.  No kernel is launched."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import components_rule as cr
import contours_rule
import polygons_rule
import shapes_rule as rule
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.int32(0x5A5A5A5A)
GUARD64 = np.uint64(0xEEEEEEEEEEEEEEEE)
GUARDM = np.int64(0x5A5A5A5A5A5A5A5A)
N_GUARD = 32
W = rule.WORDS


def _chains_of(mask, min_area=1):
    """(chain_offsets u64, points int32, list of chains) of a mask, by the contour rule."""
    _, chains = contours_rule.contours(mask, min_area)
    co = np.zeros(len(chains) + 1, np.uint64)
    co[1:] = np.cumsum([c.size for c in chains], dtype=np.uint64)
    pts = np.concatenate(chains).astype(np.int32) if chains else np.zeros(0, np.int32)
    return co, pts, chains


def _rectangle(h, w, y0, x0, rh, rw):
    m = np.zeros((h, w), bool)
    m[y0:y0 + rh, x0:x0 + rw] = True
    return m


def _l_block(h, w):
    m = np.zeros((h, w), bool)
    m[3:20, 4:10] = True
    m[14:20, 4:25] = True
    return m


def disk(size, radius):
    y, x = np.mgrid[:size, :size]
    c = size // 2
    return (x - c) ** 2 + (y - c) ** 2 <= radius * radius


def _shapes():
    line = np.zeros((9, 60), bool)
    line[4, 5:42] = True                       # 37 pixels
    dot = np.zeros((5, 5), bool)
    dot[2, 3] = True
    out = {"rectangle": _rectangle(40, 60, 5, 7, 25, 40), "line": line, "dot": dot, "l_block": _l_block(30, 40),
           "serpentine": cr.serpentine(12, 17), "spiral": cr.spiral(15), "staircase": cr.staircase(20, 20),
           "disk20": disk(48, 20), "disk40": disk(96, 40), "disk120": disk(248, 120)}
    for density in (0.05, 0.3, 0.45, 0.9):
        out[f"random{density}"] = np.random.default_rng(int(density * 100)).random((37, 53)) < density
    return out


SHAPES = _shapes()


def _xy(chain, w):
    return [int(p) % w for p in chain], [int(p) // w for p in chain]


# ---- moments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rh,rw", [(25, 40), (2, 2), (3, 17), (30, 5)])
def test_moments_of_a_filled_rectangle_are_the_closed_forms(rh, rw):
    mask = _rectangle(40, 60, 5, 7, rh, rw)
    _, _, chains = _chains_of(mask)
    hull, m = rule.shape(chains[0], 60)
    a, b = rw - 1, rh - 1                       # the polygon through the pixel centres, its corner at the anchor
    assert m[rule.ANCHOR] == 5 * 60 + 7 and m[rule.POINTS] == 2 * (rh + rw) - 4
    sign = 1 if m[rule.AREA2] > 0 else -1
    assert m[rule.AREA2] == sign * 2 * a * b
    assert (m[rule.M10_6], m[rule.M01_6]) == (sign * 3 * a * a * b, sign * 3 * a * b * b)
    assert (m[rule.M20_12], m[rule.M02_12]) == (sign * 4 * a ** 3 * b, sign * 4 * a * b ** 3)
    assert m[rule.M11_24] == sign * 6 * a * a * b * b
    assert m[rule.HULL_VERTICES] == 4 and m[rule.HULL_AREA2] == 2 * a * b
    assert hull == [5 * 60 + 7, 5 * 60 + 7 + a, (5 + b) * 60 + 7 + a, (5 + b) * 60 + 7]
    # the rectangle is its own box: any of its edges, so the first
    assert m[rule.RECT_EDGE:] == [0, 0, a * a, a * b, a * a]


@pytest.mark.parametrize("s", [2, 3, 12, 31])
def test_moments_of_a_filled_right_triangle_are_the_closed_forms(s):
    mask = np.tri(s, s, dtype=bool)             # row y holds x = 0 .. y: the hypotenuse is walked in diagonal steps
    _, _, chains = _chains_of(mask)
    hull, m = rule.shape(chains[0], s)
    L = s - 1                                   # 0 <= x <= y <= L
    sign = 1 if m[rule.AREA2] > 0 else -1
    assert m[rule.ANCHOR] == 0 and m[rule.AREA2] == sign * L * L
    assert (m[rule.M10_6], m[rule.M01_6]) == (sign * L ** 3, sign * 2 * L ** 3)
    assert (m[rule.M20_12], m[rule.M02_12], m[rule.M11_24]) == (sign * L ** 4, sign * 3 * L ** 4, sign * 3 * L ** 4)
    assert hull == [0, L * s + L, L * s] and m[rule.HULL_AREA2] == L * L


def _poly_mul(p, q):
    out = [Fraction(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _trapezoid_moments(u, v):
    """M_pq = sum over the edges of the integral of u^p v^q over the trapezoid between the edge and the u axis, exactly."""
    out = {}
    n = len(u)
    for p, q in ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)):
        total = Fraction(0)
        for i in range(n):
            u0, v0, du, dv = u[i], v[i], u[(i + 1) % n] - u[i], v[(i + 1) % n] - v[i]
            poly = [Fraction(1)]
            for _ in range(p):
                poly = _poly_mul(poly, [Fraction(u0), Fraction(du)])
            for _ in range(q + 1):
                poly = _poly_mul(poly, [Fraction(v0), Fraction(dv)])
            total += du * sum(c / (k + 1) for k, c in enumerate(poly)) / (q + 1)
        out[p, q] = total
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_moments_equal_an_exact_integration_under_every_edge(name):
    mask = SHAPES[name]
    w = mask.shape[1]
    for chain in _chains_of(mask)[2]:
        xs, ys = _xy(chain, w)
        got = rule.moments(xs, ys)
        M = _trapezoid_moments([x - xs[0] for x in xs], [y - ys[0] for y in ys])
        # the shoelace sum is minus twice the sum of the trapezoids
        want = [-2 * M[0, 0], -6 * M[1, 0], -6 * M[0, 1], -12 * M[2, 0], -24 * M[1, 1], -12 * M[0, 2]]
        assert got[:6] == want, name
        assert got[6:] == [sum(x - xs[0] for x in xs), sum(y - ys[0] for y in ys), sum((x - xs[0]) ** 2 for x in xs),
                           sum((x - xs[0]) * (y - ys[0]) for x, y in zip(xs, ys)), sum((y - ys[0]) ** 2 for y in ys)]
        assert abs(got[0]) == polygons_rule.polygon(chain, w, 0, 0)[1][2], "|area2| is the polygon rule's at eps = 0"


def _central(m):
    """Central second moments of the region (times the area) and of the points (times n), as fractions."""
    a = Fraction(m[rule.AREA2], 2)
    m10, m01 = Fraction(m[rule.M10_6], 6), Fraction(m[rule.M01_6], 6)
    m20, m11, m02 = Fraction(m[rule.M20_12], 12), Fraction(m[rule.M11_24], 24), Fraction(m[rule.M02_12], 12)
    n = m[rule.POINTS]
    region = None if a == 0 else (abs(a), (m20 - m10 * m10 / a) * (1 if a > 0 else -1),
                                  (m11 - m10 * m01 / a) * (1 if a > 0 else -1), (m02 - m01 * m01 / a) * (1 if a > 0 else -1))
    s10, s01, s20, s11, s02 = m[rule.S10:rule.S02 + 1]
    return region, (n, s20 - Fraction(s10 * s10, n), s11 - Fraction(s10 * s01, n), s02 - Fraction(s01 * s01, n))


@pytest.mark.parametrize("name", ["rectangle", "l_block", "spiral", "disk20", "line", "staircase"])
def test_central_moments_do_not_depend_on_the_position_or_the_anchor(name):
    mask = SHAPES[name]
    h, w = mask.shape
    chain = max(_chains_of(mask)[2], key=len)
    m0 = rule.shape(chain, w)[1]
    big = np.zeros((h + 30, w + 50), bool)
    big[13:13 + h, 29:29 + w] = mask
    moved = max(_chains_of(big)[2], key=len)
    m1 = rule.shape(moved, w + 50)[1]
    assert m1[rule.ANCHOR] != m0[rule.ANCHOR] and m1[:2] == m0[:2] and m1[3:] == m0[3:], "a shift moves the anchor alone"
    assert _central(m0) == _central(m1)
    for shift in (1, len(chain) // 3, len(chain) - 1):
        rolled = np.roll(chain, -shift)
        m2 = rule.shape(rolled, w)[1]
        assert _central(m2) == _central(m0), f"{name}: anchored at position {shift}"
        assert m2[rule.HULL_VERTICES] == m0[rule.HULL_VERTICES] and m2[rule.HULL_AREA2:] == m0[rule.HULL_AREA2:]


def test_the_sums_wrap_and_read_back_as_signed():
    assert rule.wrap((1 << 63)) == -(1 << 63) and rule.wrap(-1) == -1 and rule.wrap((1 << 64) + 5) == 5
    # the border of the largest frame: the largest second moment an outer border has still fits
    xs, ys = [0, 32766, 32766, 0], [0, 0, 32766, 32766]
    big = rule.moments(xs * 1, ys * 1)
    assert big[3] == 4 * 32766 ** 4 and big[3] < 1 << 63


# ---- hull ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_hull_is_strictly_convex_holds_every_point_and_starts_at_the_left(name):
    mask = SHAPES[name]
    w = mask.shape[1]
    for chain in _chains_of(mask)[2]:
        hull, m = rule.shape(chain, w)
        xs, ys = _xy(chain, w)
        hx, hy = _xy(hull, w)
        v = len(hull)
        assert v == m[rule.HULL_VERTICES] >= 1 and len(set(hull)) == v
        assert set(hull) <= {int(p) for p in chain}, "every hull vertex is a chain point"
        assert (hx[0], hy[0]) == min(zip(xs, ys)), "the start is the smallest x, then the smallest y"
        if v >= 3:
            for k in range(v):
                ax, ay, bx, by, cx, cy = hx[k], hy[k], hx[(k + 1) % v], hy[(k + 1) % v], hx[(k + 2) % v], hy[(k + 2) % v]
                assert (bx - ax) * (cy - by) - (by - ay) * (cx - bx) > 0, "every turn is strictly positive"
        for k in range(v if v >= 2 else 0):
            ax, ay, dx, dy = hx[k], hy[k], hx[(k + 1) % v] - hx[k], hy[(k + 1) % v] - hy[k]
            assert all(dx * (y - ay) - dy * (x - ax) >= 0 for x, y in zip(xs, ys)), "every point lies on or inside"
        if v == 2:   # a segment: every point lies ON it, between its ends
            assert all(min(hx) <= x <= max(hx) and min(hy) <= y <= max(hy) for x, y in zip(xs, ys))
        if v == 1:
            assert set(zip(xs, ys)) == {(hx[0], hy[0])}
        assert m[rule.HULL_AREA2] == sum(hx[k] * hy[(k + 1) % v] - hx[(k + 1) % v] * hy[k] for k in range(v)) >= 0
        assert m[rule.HULL_AREA2] >= abs(m[rule.AREA2])


def test_a_large_disk_has_more_hull_vertices_than_a_wave_has_lanes():
    """The hull of a digital disk of radius r has about 3.5 r^(2/3) vertices: 20 at r = 20 and 44 at r = 40, so the case
    that sends the emit kernel's lanes over the edges a second time is the disk of radius 120."""
    counts = {name: rule.shape(_chains_of(SHAPES[name])[2][0], SHAPES[name].shape[1])[1][rule.HULL_VERTICES]
              for name in ("disk20", "disk40", "disk120")}
    assert counts == {"disk20": 20, "disk40": 44, "disk120": 84}


# ---- rectangle ---------------------------------------------------------------------------------------------------------
def _box(hx, hy, ax, ay, dx, dy):
    """The area of the bounding box of the hull along the direction (dx, dy), exactly."""
    along = [(x - ax) * dx + (y - ay) * dy for x, y in zip(hx, hy)]
    across = [dx * (y - ay) - dy * (x - ax) for x, y in zip(hx, hy)]
    return Fraction((max(along) - min(along)) * (max(across) - min(across)), dx * dx + dy * dy)


@pytest.mark.parametrize("name", list(SHAPES))
def test_no_direction_through_two_hull_vertices_gives_a_smaller_box(name):
    mask = SHAPES[name]
    w = mask.shape[1]
    for chain in _chains_of(mask)[2]:
        hull, m = rule.shape(chain, w)
        hx, hy = _xy(hull, w)
        v = len(hull)
        k, lo, hi, across, len2 = m[rule.RECT_EDGE:]
        if v == 1:
            assert (k, lo, hi, across, len2) == (0, 0, 0, 0, 0)
            continue
        dx, dy = hx[(k + 1) % v] - hx[k], hy[(k + 1) % v] - hy[k]
        assert len2 == dx * dx + dy * dy > 0 and 0 <= k < v
        stored = Fraction((hi - lo) * across, len2)
        assert stored == _box(hx, hy, hx[k], hy[k], dx, dy), "the stored words are the box along the stored edge"
        if v == 2:
            assert (k, lo, hi, across) == (0, 0, len2, 0)
        edges = [_box(hx, hy, hx[e], hy[e], hx[(e + 1) % v] - hx[e], hy[(e + 1) % v] - hy[e]) for e in range(v)]
        assert k == edges.index(min(edges)), "the stored edge is the smallest minimiser"
        for i in range(v):
            for j in range(v):
                if i != j:
                    assert _box(hx, hy, hx[i], hy[i], hx[j] - hx[i], hy[j] - hy[i]) >= stored, (name, i, j)
        # every hull vertex lies in the rectangle the words describe
        for x, y in zip(hx, hy):
            assert lo <= (x - hx[k]) * dx + (y - hy[k]) * dy <= hi and 0 <= dx * (y - hy[k]) - dy * (x - hx[k]) <= across


def test_python_rectangle_helper_gives_the_corners():
    mask = _rectangle(40, 60, 5, 7, 25, 40)
    co, pts, _ = _chains_of(mask)
    hoff, hull, meas = capi.shapes_from_chains(co, pts, 60, 40)
    corners, (length, breadth), angle = capi.shape_rectangle(meas[0], hull, 60)
    assert np.allclose(corners, [[7, 5], [46, 5], [46, 29], [7, 29]]) and (length, breadth, angle) == (39.0, 24.0, 0.0)


# ---- the library's host function against the rule -----------------------------------------------------------------------
def _call(co, pts, pcap, w, h, hcap, want_measures=True):
    """canny_hip_shapes_from_chains on guarded buffers -> (hull_offsets, hull, measures), all with their guards."""
    L = capi.load()
    k = co.size - 1
    hoff = np.full(k + 1 + N_GUARD, GUARD64, np.uint64)
    hull = np.full(hcap + N_GUARD, GUARD, np.int32)
    meas = np.full((k + N_GUARD) * W, GUARDM, np.int64)
    st = L.canny_hip_shapes_from_chains(capi._hp(co), capi._hp(pts) if pts.size else None, k, pcap, w, h, capi._hp(hoff),
                                        capi._hp(hull), hcap, capi._hp(meas) if want_measures else None)
    assert st == 0
    return hoff, hull, meas


def _check(co, pts, pcap, w, h, hcap, what):
    k = co.size - 1
    w_hoff, w_hull, w_meas = rule.csr(co, pts, pcap, w)
    results = []
    for want_measures in (True, False):
        hoff, hull, meas = _call(co, pts, pcap, w, h, hcap, want_measures)
        assert np.array_equal(hoff[:k + 1], w_hoff), f"{what}: hull_offsets"
        assert np.all(hoff[k + 1:] == GUARD64), f"{what}: written past the hull offsets"
        fit = min(hcap, w_hull.size)
        assert np.array_equal(hull[:fit], w_hull[:fit]), f"{what}: hull"
        assert np.all(hull[fit:] == GUARD), f"{what}: written past the hull vertices that fit"
        if want_measures:
            assert np.array_equal(meas[:W * k].reshape(k, W), w_meas), f"{what}: measures"
            assert np.all(meas[W * k:] == GUARDM), f"{what}: written past the measures"
        else:
            assert np.all(meas == GUARDM)
        results.append((hoff.tobytes(), hull.tobytes()))
    assert results[0] == results[1], f"{what}: the outputs depend on whether measures was given"
    return w_hoff, w_hull, w_meas


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_function_equals_the_rule(name):
    mask = SHAPES[name]
    h, w = mask.shape
    co, pts, _ = _chains_of(mask)
    w_hoff, _, _ = _check(co, pts, pts.size, w, h, pts.size, name)
    total = int(w_hoff[-1])
    _check(co, pts, pts.size, w, h, total, f"{name}, exact-size hull")
    _check(co, pts, pts.size, w, h, 0, f"{name}, hull_capacity 0")
    if total > 2:
        _check(co, pts, pts.size, w, h, total // 2, f"{name}, hull cut")
    j = int(np.argmax(np.diff(co)))
    mid = int(co[j]) + max(1, int(co[j + 1] - co[j]) // 2)
    if mid < pts.size:
        _, _, w_meas = _check(co, pts, mid, w, h, pts.size, f"{name}, points cut at {mid}")
        assert tuple(w_meas[-1]) == (-1,) + (0,) * (W - 1), "the last chain is cut"
    _check(co, pts, 0, w, h, 8, f"{name}, point_capacity 0")


@pytest.mark.parametrize("density", [0.05, 0.2, 0.45, 0.7, 0.9])
def test_host_function_on_random_maps(density):
    for seed, min_area in ((1, 1), (2, 5)):
        mask = np.random.default_rng(seed * 1000 + int(density * 100)).random((37, 53)) < density
        co, pts, chains = _chains_of(mask, min_area)
        if min_area > 1 and not chains:
            continue                       # a sparse map has no component of five pixels
        assert chains
        _check(co, pts, pts.size, 53, 37, pts.size, f"density {density}")
        _check(co, pts, pts.size, 53, 37, max(1, int(co.size) // 2), f"density {density}, hull cut")


def test_python_wrapper_and_argument_errors():
    mask = SHAPES["random0.45"]
    h, w = mask.shape
    co, pts, _ = _chains_of(mask)
    want = rule.csr(co, pts, pts.size, w)
    hoff, hull, meas = capi.shapes_from_chains(co, pts, w, h)
    assert np.array_equal(hoff, want[0]) and np.array_equal(hull, want[1]) and np.array_equal(meas, want[2])
    assert hull.dtype == np.int32 and meas.dtype == np.int64 and meas.shape[1] == capi.SHAPE_WORDS == len(capi.SHAPE_MEASURES)
    hoff, hull, meas = capi.shapes_from_chains(co, pts, w, h, hull_capacity=5, want_measures=False)
    assert meas is None and np.array_equal(hoff, want[0]) and np.array_equal(hull, want[1][:5])
    L = capi.load()
    hoff = np.full(co.size, GUARD64, np.uint64)
    hull = np.full(8, GUARD, np.int32)
    args = lambda **kw: [kw.get("co", capi._hp(co)), kw.get("pts", capi._hp(pts)), co.size - 1, pts.size,
                         kw.get("w", w), kw.get("h", h), kw.get("hoff", capi._hp(hoff)), kw.get("hull", capi._hp(hull)), 8,
                         None]
    for kw, status in ((dict(co=None), 1), (dict(pts=None), 1), (dict(hoff=None), 1), (dict(hull=None), 1),
                       (dict(w=32768), 2), (dict(h=32768), 2), (dict(w=0), 1), (dict(h=0), 1), (dict(h=-3), 1)):
        assert L.canny_hip_shapes_from_chains(*args(**kw)) == status, kw
        assert np.all(hoff == GUARD64) and np.all(hull == GUARD), f"{kw}: a rejected call writes nothing"
    assert L.canny_hip_shapes_from_chains(*args(h=32767)) == 0
    out = np.zeros(5, np.uint64)
    assert L.canny_hip_selftest_shapes_plan(0, 0, capi._hp(out)) == 1 and L.canny_hip_selftest_shapes_plan(2, 1, capi._hp(out)) == 1
    assert L.canny_hip_selftest_shapes_plan(0, 1, None) == 1


def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1700
    assert capi.load().canny_hip_version() >= 1700
    for word in ("cv::moments", "cv::convexHull", "cv::minAreaRect", "CANNY_HIP_SHAPE_WORDS 20", "WRAPPING",
                 "CANNY_HIP_SHAPE_PART_MEASURE", "CANNY_HIP_SHAPE_PART_SCAN", "CANNY_HIP_SHAPE_PART_EMIT", "hole borders",
                 "convexity defects", "ellipse fits", "minimum enclosing circle", "Hu invariants",
                 "canny_hip_selftest_shapes_plan"):
        assert word in header, word
    names = re.search(r"enum canny_hip_shape_measure \{(.*?)\};", header, re.S).group(1)
    got = [n.lower() for n in re.findall(r"CANNY_HIP_SHAPE_(\w+) = \d+", names)]
    assert got == list(capi.SHAPE_MEASURES)


# ---- the CLI's grammar ------------------------------------------------------------------------------------------------
def test_cli_u_needs_t(tmp_path):
    """-u without -t is a usage error like -y without -t: a message and exit status 2, before any frame is read or any
    device is touched."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    run = lambda flags: subprocess.run([exe, "1.0", "50", "150", "-o", str(tmp_path)] + flags, capture_output=True,
                                       text=True, timeout=60)
    r = run(["-u"])
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -u needs the contours of -t")
    r = run(["-u", "-m", "3"])
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -u needs")
    r = run(["-t", "-u", "-y"])
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-u" in r.stderr and "canny_shapes.txt" in r.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_shapes_host.cpp has its own main and is compiled together with csrc/canny_shapes_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_shapes_host"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_shapes_host.cpp"),
                           os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_shapes_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed chains ok" in r.stdout, r.stdout + r.stderr
