"""CPU-only checks of the polygon rule: tests/polygons_rule.py against properties that need no
simplifier at all, the library's host function canny_hip_polygons_from_chains against the rule byte for byte, and the
grammar of the CLI's -y flag.  No kernel is launched here."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_rule as cr
import contours_rule
import polygons_rule as rule
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.int32(0x5A5A5A5A)
GUARD64 = np.uint64(0xEEEEEEEEEEEEEEEE)
GUARDM = np.int64(0x5A5A5A5A5A5A5A5A)
N_GUARD = 32
TOLERANCES = [(0, 0), (256, 0), (512, 0), (0, 1311), (384, 655), (1 << 24, 0)]


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


def _shapes():
    line = np.zeros((9, 60), bool)
    line[4, 5:42] = True                       # 37 pixels
    dot = np.zeros((5, 5), bool)
    dot[2, 3] = True
    out = {"rectangle": _rectangle(40, 60, 5, 7, 25, 40), "line": line, "dot": dot, "l_block": _l_block(30, 40),
           "serpentine": cr.serpentine(12, 17), "spiral": cr.spiral(15), "staircase": cr.staircase(20, 20)}
    for density in (0.05, 0.3, 0.45, 0.9):
        out[f"random{density}"] = np.random.default_rng(int(density * 100)).random((37, 53)) < density
    return out


SHAPES = _shapes()


# ---- properties that do not depend on how the vertices were found -------------------------------------------------------
@pytest.mark.parametrize("tol", TOLERANCES, ids=lambda t: f"eps{t[0]}_ratio{t[1]}")
@pytest.mark.parametrize("name", list(SHAPES))
def test_vertices_are_an_ordered_subsequence_and_every_point_lies_within_the_tolerance(name, tol):
    mask = SHAPES[name]
    w = mask.shape[1]
    _, _, chains = _chains_of(mask)
    assert chains
    for chain in chains:
        pos, (v, length, area2, convex) = rule.polygon(chain, w, *tol)
        n = chain.size
        assert pos[0] == 0 and pos == sorted(set(pos)) and all(0 <= i < n for i in pos) and v == len(pos)
        xs, ys = [int(p) % w for p in chain], [int(p) // w for p in chain]
        assert length == rule.length_q8(xs, ys)
        eps = rule.tolerance(tol[0], tol[1], length)
        if n == 1:
            assert pos == [0] and length == 0
            continue
        assert v >= 2
        for a, b in zip(pos, pos[1:] + [n]):
            ax, ay, bx, by = xs[a], ys[a], xs[b % n], ys[b % n]
            assert (ax, ay) != (bx, by)
            base2 = (bx - ax) ** 2 + (by - ay) ** 2
            for i in range(a + 1, b):
                c = (bx - ax) * (ys[i] - ay) - (by - ay) * (xs[i] - ax)
                assert c * c * 65536 <= eps * eps * base2, f"{name}: point {i} is farther than eps from edge ({a}, {b})"
                if eps == 0:
                    assert c == 0, "eps = 0 removes only collinear points"
        if tol[0] >= 1 << 24:
            d2 = [(x - xs[0]) ** 2 + (y - ys[0]) ** 2 for x, y in zip(xs, ys)]
            assert pos == [0, d2.index(max(d2))], "eps = 2^24 leaves the two anchors"


def test_the_tolerance_is_capped():
    assert rule.tolerance(1 << 30, 0, 0) == 1 << 24 and rule.tolerance(0, 65535, 1 << 40) == 1 << 24
    assert rule.tolerance(384, 655, 33280) == 384 + ((655 * 33280) >> 16)
    co, pts, chains = _chains_of(SHAPES["rectangle"])
    assert rule.polygon(chains[0], 60, 1 << 30, 0)[0] == rule.polygon(chains[0], 60, 1 << 24, 0)[0]
    assert len(rule.polygon(chains[0], 60, 1 << 30, 0)[0]) == 2


@pytest.mark.parametrize("tol", [(0, 0), (256, 0), (512, 0), (0, 1311), (100, 1311)])
def test_a_filled_rectangle_gives_its_four_corners(tol):
    h, w, y0, x0, rh, rw = 40, 60, 5, 7, 25, 40
    _, _, chains = _chains_of(_rectangle(h, w, y0, x0, rh, rw))
    assert len(chains) == 1 and chains[0].size == 2 * (rh + rw) - 4
    pos, (v, length, area2, convex) = rule.polygon(chains[0], w, *tol)
    corners = {y0 * w + x0, y0 * w + x0 + rw - 1, (y0 + rh - 1) * w + x0, (y0 + rh - 1) * w + x0 + rw - 1}
    assert {int(chains[0][i]) for i in pos} == corners and v == 4
    assert convex == 1 and area2 == 2 * (rw - 1) * (rh - 1) and length == 256 * (2 * (rh + rw) - 4)


def test_a_line_a_pixel_and_an_l():
    line = SHAPES["line"]
    _, _, chains = _chains_of(line)
    assert chains[0].size == 2 * 37 - 2        # walked out and back
    pos, m = rule.polygon(chains[0], line.shape[1], 0, 0)
    assert [int(chains[0][i]) for i in pos] == [4 * 60 + 5, 4 * 60 + 41] and tuple(m) == (2, 256 * 72, 0, 0)
    _, _, chains = _chains_of(SHAPES["dot"])
    pos, m = rule.polygon(chains[0], 5, 256, 1311)
    assert pos == [0] and tuple(m) == (1, 0, 0, 0)
    _, _, chains = _chains_of(SHAPES["l_block"])
    pos, m = rule.polygon(chains[0], 40, 256, 0)
    assert m[0] == 6 and m[3] == 0, "an L-shaped block has six corners and is not convex"


def test_the_l_blocks_area_is_the_shoelace_of_its_corners():
    _, _, chains = _chains_of(SHAPES["l_block"])
    pos, m = rule.polygon(chains[0], 40, 0, 0)
    # the polygon through pixel centres.  The pixel (9, 14) in the concave corner has all four 4-neighbours set, so it is
    # no border pixel: the 8-connected border steps from (9, 13) diagonally to (10, 14) and both are vertices at eps = 0
    corners = [(4, 3), (9, 3), (9, 13), (10, 14), (24, 14), (24, 19), (4, 19)]
    assert sorted((int(chains[0][i]) % 40, int(chains[0][i]) // 40) for i in pos) == sorted(corners)
    shoelace = abs(sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(corners, corners[1:] + corners[:1])))
    assert m[2] == shoelace and m[3] == 0


def test_a_staircase_comes_down_to_its_turning_points():
    m = cr.staircase(20, 20)
    _, _, chains = _chains_of(m)
    for chain in chains:
        pos, (v, length, area2, convex) = rule.polygon(chain, 20, 0, 0)
        if chain.size > 2:
            assert v == 2 and area2 == 0 and convex == 0 and length == 362 * chain.size


# ---- the library's host function against the rule -----------------------------------------------------------------------
def _call(co, pts, pcap, w, h, tol, vcap, want_measures=True):
    """canny_hip_polygons_from_chains on guarded buffers -> (vertex_offsets, vertices, measures), all with their guards."""
    L = capi.load()
    k = co.size - 1
    voff = np.full(k + 1 + N_GUARD, GUARD64, np.uint64)
    verts = np.full(vcap + N_GUARD, GUARD, np.int32)
    meas = np.full((k + N_GUARD) * 4, GUARDM, np.int64)
    st = L.canny_hip_polygons_from_chains(capi._hp(co), capi._hp(pts) if pts.size else None, k, pcap, w, h, tol[0], tol[1],
                                          capi._hp(voff), capi._hp(verts), vcap, capi._hp(meas) if want_measures else None)
    assert st == 0
    return voff, verts, meas


def _check(co, pts, pcap, w, h, tol, vcap, what):
    k = co.size - 1
    w_voff, w_verts, w_meas = rule.csr(co, pts, pcap, w, *tol)
    results = []
    for want_measures in (True, False):
        voff, verts, meas = _call(co, pts, pcap, w, h, tol, vcap, want_measures)
        assert np.array_equal(voff[:k + 1], w_voff), f"{what}: vertex_offsets"
        assert np.all(voff[k + 1:] == GUARD64), f"{what}: written past the vertex offsets"
        fit = min(vcap, w_verts.size)
        assert np.array_equal(verts[:fit], w_verts[:fit]), f"{what}: vertices"
        assert np.all(verts[fit:] == GUARD), f"{what}: written past the vertices that fit"
        if want_measures:
            assert np.array_equal(meas[:4 * k].reshape(k, 4), w_meas), f"{what}: measures"
            assert np.all(meas[4 * k:] == GUARDM), f"{what}: written past the measures"
        else:
            assert np.all(meas == GUARDM)
        results.append((voff.tobytes(), verts.tobytes()))
    assert results[0] == results[1], f"{what}: the outputs depend on whether measures was given"
    return w_voff, w_verts, w_meas


@pytest.mark.parametrize("tol", TOLERANCES, ids=lambda t: f"eps{t[0]}_ratio{t[1]}")
@pytest.mark.parametrize("name", list(SHAPES))
def test_host_function_equals_the_rule(name, tol):
    mask = SHAPES[name]
    h, w = mask.shape
    co, pts, _ = _chains_of(mask)
    w_voff, w_verts, _ = _check(co, pts, pts.size, w, h, tol, pts.size, name)
    total = int(w_voff[-1])
    _check(co, pts, pts.size, w, h, tol, total, f"{name}, exact-size vertices")
    _check(co, pts, pts.size, w, h, tol, 0, f"{name}, vertex_capacity 0")
    if total > 2:
        _check(co, pts, pts.size, w, h, tol, total // 2, f"{name}, vertices cut")


@pytest.mark.parametrize("density", [0.05, 0.2, 0.45, 0.7, 0.9])
def test_host_function_on_random_maps_with_cut_chains(density):
    for seed, min_area in ((1, 1), (2, 5)):
        mask = np.random.default_rng(seed * 1000 + int(density * 100)).random((37, 53)) < density
        co, pts, chains = _chains_of(mask, min_area)
        if min_area > 1 and not chains:
            continue                       # a sparse map has no component of five pixels
        assert chains
        h, w = mask.shape
        for tol in ((0, 0), (256, 0), (0, 1311), (384, 655)):
            _check(co, pts, pts.size, w, h, tol, pts.size, f"density {density}")
            j = int(np.argmax(np.diff(co)))
            mid = int(co[j]) + max(1, int(co[j + 1] - co[j]) // 2)
            w_voff, _, w_meas = _check(co, pts, min(mid, pts.size - 1), w, h, tol, pts.size, f"density {density}, cut at {mid}")
            assert w_meas[-1, 0] == -1 and tuple(w_meas[-1]) == (-1, 0, 0, 0), "the last chain is cut"
            assert w_voff[-1] == w_voff[-2]
            _check(co, pts, 0, w, h, tol, 8, f"density {density}, point_capacity 0")


def test_python_wrapper_and_argument_errors():
    mask = SHAPES["random0.45"]
    h, w = mask.shape
    co, pts, _ = _chains_of(mask)
    want = rule.csr(co, pts, pts.size, w, 256, 1311)
    voff, verts, meas = capi.polygons_from_chains(co, pts, w, h, 256, 1311)
    assert np.array_equal(voff, want[0]) and np.array_equal(verts, want[1]) and np.array_equal(meas, want[2])
    assert verts.dtype == np.int32 and meas.dtype == np.int64
    voff, verts, meas = capi.polygons_from_chains(co, pts, w, h, 256, 1311, vertex_capacity=5, want_measures=False)
    assert meas is None and np.array_equal(voff, want[0]) and np.array_equal(verts, want[1][:5])
    assert capi.polygon_tolerance(1.5, 0.02) == (384, 1311)
    L = capi.load()
    voff = np.full(co.size, GUARD64, np.uint64)
    verts = np.full(8, GUARD, np.int32)
    args = lambda **kw: [kw.get("co", capi._hp(co)), kw.get("pts", capi._hp(pts)), co.size - 1, pts.size,
                         kw.get("w", w), kw.get("h", h), 0, kw.get("ratio", 0), kw.get("voff", capi._hp(voff)),
                         kw.get("verts", capi._hp(verts)), 8, None]
    for kw, status in ((dict(ratio=65536), 1), (dict(co=None), 1), (dict(pts=None), 1), (dict(voff=None), 1),
                       (dict(verts=None), 1), (dict(w=32769), 2), (dict(h=32769), 2), (dict(w=0), 1)):
        assert L.canny_hip_polygons_from_chains(*args(**kw)) == status, kw
        assert np.all(voff == GUARD64) and np.all(verts == GUARD), f"{kw}: a rejected call writes nothing"
    assert L.canny_hip_polygons_from_chains(*args(w=32768, h=32768)) == 0


def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1200
    assert capi.load().canny_hip_version() >= 1200
    for word in ("362", "cv::arcLength", "0.02 %", "CANNY_HIP_POLYGON_PART_SIMPLIFY", "CANNY_HIP_POLYGON_PART_SCAN",
                 "CANNY_HIP_POLYGON_PART_EMIT", "open-curve", "hole borders"):
        assert word in header, word


# ---- the CLI's grammar ------------------------------------------------------------------------------------------------
def test_cli_y_needs_t_and_a_well_formed_tolerance(tmp_path):
    """-y without -t and a malformed -y are usage errors like -g without -l: a message and exit status 2, before any frame
    is read or any device is touched; -y without a value falls through to the usage text like every flag that lacks one."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    run = lambda flags: subprocess.run([exe, "1.0", "50", "150", "-o", str(tmp_path)] + flags, capture_output=True,
                                       text=True, timeout=60)
    r = run(["-y", "2"])
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -y needs the contours of -t")
    r = run(["-y", "2,0.02", "-m", "3"])
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -y needs")
    for value in ("abc", "-1", "1,2", "1,", ",1", "1,0.5,3", "1,-0.1", "1x", "nan", " 1", "1e30"):
        r = run(["-t", "-y", value])
        assert r.returncode == 2 and r.stderr.startswith("ERROR: -y expects epsilon[,ratio]"), value
    r = run(["-t", "-y"])
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-y epsilon[,ratio]" in r.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_polygons_host.cpp has its own main and is compiled together with csrc/canny_polygons_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_polygons_host"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_polygons_host.cpp"),
                           os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_polygons_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed chains ok" in r.stdout, r.stdout + r.stderr
