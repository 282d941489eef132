"""CPU-only checks of the sub-pixel edgel rule (include/canny_hip.h): the host function
canny_hip_edgels_from_plane against tests/edgels_rule.py word for word, the rule's two restatements (numpy and plain Python
ints) against each other, the invariants of every record, the accuracy of the refined positions on synthetic straight
edges, the launch plan of the index-driven kernel, the -e grammar of the command line, and the host function under the
host compiler's sanitizers in a stand-alone program.  No GPU is needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import edgels_rule as er
import oracle
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_and_beyond(h, w):
    """Every pixel index of an h x w frame, then indices that are none."""
    return np.concatenate([np.arange(h * w, dtype=np.uint32),
                           np.array([h * w, h * w + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32)])


def check_plane(P, idx=None):
    """Host function == numpy rule == scalar rule on the given indices (default: all and beyond); the invariants."""
    P = np.ascontiguousarray(P)
    h, w = P.shape
    idx = all_and_beyond(h, w) if idx is None else np.asarray(idx, np.uint32)
    want = er.edgels_at(P, idx)
    got = capi.edgels_from_plane(P, idx)
    assert got.dtype == np.int32 and got.shape == (idx.size, 4)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} records differ, first at index {idx[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    step = max(1, idx.size // 400)  # the plain-Python form on a sample (all of a small plane)
    for q in range(0, idx.size, step):
        assert tuple(int(v) & 0xFFFFFFFF for v in got[q]) == tuple(v & 0xFFFFFFFF for v in er.edgel_scalar(P, int(idx[q])))
    x, y, gx, gy, mag, d, refined, invalid = er.unpack(got)
    assert np.array_equal(invalid, idx >= h * w)
    assert not got[invalid][:, :3].any() and np.all(got[invalid][:, 3].view(np.uint32) == er.INVALID)
    ok = ~invalid
    px, py = (idx[ok] % w).astype(np.int64), (idx[ok] // w).astype(np.int64)
    tx, ty = got[ok, 0] - 256 * px, got[ok, 1] - 256 * py
    assert np.all(np.abs(tx) <= 128) and np.all(np.abs(ty) <= 128)
    steps = np.array(er.STEPS)[d[ok]]
    t = np.where(steps[:, 0] == 1, tx, ty)  # both offsets are t_q8 times the step
    assert np.array_equal(tx, t * steps[:, 0]) and np.array_equal(ty, t * steps[:, 1])
    r = refined[ok]
    assert np.all((px[r] - steps[r, 0] >= 0) & (px[r] + steps[r, 0] < w) & (py[r] - 1 >= -1 + np.abs(steps[r, 1])) &
                  (py[r] + np.abs(steps[r, 1]) < h)), "a refined edgel has a neighbour outside the frame"
    assert not (tx[~r].any() or ty[~r].any())
    ogx, ogy = oracle.xy_gradient(P.astype(np.int16))
    assert np.array_equal(gx[ok], ogx.reshape(-1)[idx[ok]]) and np.array_equal(gy[ok], ogy.reshape(-1)[idx[ok]])
    return got


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_u8_planes(seed):
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 256, (37, 53)).astype(np.uint8)
    rec = check_plane(P)
    assert er.unpack(rec)[6].any(), "no refined edgel at all"
    check_plane(np.ascontiguousarray(P.astype(np.int16)))  # the same values as shorts: the same records
    assert np.array_equal(capi.edgels_from_plane(P.astype(np.int16), all_and_beyond(37, 53)), rec)


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_random_s16_planes_over_the_full_range(seed):
    """Sums beyond short wrap, M reaches towards 2^31, the root needs 64 bits."""
    rng = np.random.default_rng(seed)
    P = rng.integers(-32768, 32768, (37, 53)).astype(np.int16)
    rec = check_plane(P)
    mag_q4 = rec[:, 3].view(np.uint32) & er.MAG_MASK
    assert mag_q4.max() > 16 * 32768, "no magnitude beyond one component's range"


def test_s16_extremes_reach_the_largest_magnitude():
    P = np.full((9, 11), -32768, np.int16)
    P[:, 5:] = 32767
    P[4:, :] ^= -1  # rows 4.. swap the ends
    check_plane(P)
    # the pair (-32768, -32768) itself: M = 2^31, mag_q4 = floor(sqrt(2^39)) = 741455
    assert er.mag_q4_scalar(-32768, -32768) == 741455 == int(er.mag_q4(-32768, -32768))
    for kind in range(3):
        yy, xx = np.mgrid[0:9, 0:11]
        board = ((xx + yy) & 1, xx & 1, (yy >> 1) & 1)[kind]
        check_plane(np.where(board, 32767, -32768).astype(np.int16))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_flat_plane_has_zero_gradient_and_no_refinement(dtype):
    rec = check_plane(np.full((6, 8), 77, dtype))[:48]
    assert not rec[:, 2].any() and not rec[:, 3].any()
    assert np.array_equal(rec[:, 0], 256 * (np.arange(48) % 8)) and np.array_equal(rec[:, 1], 256 * (np.arange(48) // 8))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_designed_ties(dtype):
    """b == a > c gives t_q8 = -128 (and b == c > a +128); b == a == c is not refined."""
    tie = np.tile(np.array([0, 0, 10, 20, 30, 30, 30, 30], dtype), (6, 1))
    rec = check_plane(tie)
    for x, t in ((3, -128), (2, 128)):
        r = rec[2 * 8 + x]
        assert (r[0], r[1]) == (256 * x + t, 512) and r[3] & er.REFINED and (r[3] & er.MAG_MASK) == 16 * 80
    ramp = np.tile((10 * np.arange(8)).astype(dtype), (6, 1))
    rec = check_plane(ramp)
    inner = rec.reshape(-1, 4)[[2 * 8 + x for x in range(2, 6)]]
    assert np.all(inner[:, 3] == 16 * 80) and np.array_equal(inner[:, 0], 256 * np.arange(2, 6))
    # the same along the other three steps
    check_plane(np.ascontiguousarray(tie.T))
    yy, xx = np.mgrid[0:12, 0:12]
    prof = np.array([0, 0, 0, 0, 10, 20, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30])
    d1 = er.unpack(check_plane(prof[xx + yy].astype(dtype)))
    d3 = er.unpack(check_plane(prof[xx - yy + 11].astype(dtype)))
    assert (d1[5][d1[6]] == 1).any() and (d3[5][d3[6]] == 3).any()


@pytest.mark.parametrize("shape", [(2, 2), (2, 70), (70, 2)])
def test_thin_frames(shape):
    rng = np.random.default_rng(shape[1])
    check_plane(rng.integers(0, 256, shape).astype(np.uint8))
    check_plane(rng.integers(-32768, 32768, shape).astype(np.int16))


def test_every_border_pixel():
    rng = np.random.default_rng(9)
    for P in (rng.integers(0, 256, (9, 11)).astype(np.uint8), rng.integers(-2000, 2000, (9, 11)).astype(np.int16)):
        yy, xx = np.mgrid[0:9, 0:11]
        border = np.flatnonzero(((yy == 0) | (yy == 8) | (xx == 0) | (xx == 10)).reshape(-1))
        for q in border:  # all of them through the plain-Python form
            got = capi.edgels_from_plane(P, [q])[0]
            assert tuple(int(v) & 0xFFFFFFFF for v in got) == tuple(v & 0xFFFFFFFF for v in er.edgel_scalar(P, int(q)))
        check_plane(P, border)


def test_lists_in_any_order_with_invalid_indices():
    rng = np.random.default_rng(11)
    P = rng.integers(0, 256, (12, 17)).astype(np.uint8)
    idx = rng.integers(0, 12 * 17, 300).astype(np.uint32)
    idx[::7] = rng.integers(12 * 17, 2 ** 32, idx[::7].size, dtype=np.uint64).astype(np.uint32)
    idx[5] = 12 * 17  # the first index that is none
    rec = check_plane(P, idx)
    assert er.unpack(rec)[7].sum() == idx[::7].size + (5 % 7 != 0)


def test_statuses_and_empty_list():
    L = capi.load()
    P = np.zeros((2, 2), np.uint8)
    one, out = np.zeros(1, np.uint32), np.zeros(4, np.int32)
    hp = capi._hp
    assert L.canny_hip_edgels_from_plane(None, 1, 2, 2, hp(one), 1, hp(out)) == 1
    assert L.canny_hip_edgels_from_plane(hp(P), 1, 1, 4, hp(one), 1, hp(out)) == 1
    assert L.canny_hip_edgels_from_plane(hp(P), 1, 4, 1, hp(one), 1, hp(out)) == 1
    assert L.canny_hip_edgels_from_plane(hp(P), 1, 2, 2, None, 1, hp(out)) == 1
    assert L.canny_hip_edgels_from_plane(hp(P), 1, 2, 2, hp(one), 1, None) == 1
    assert L.canny_hip_edgels_from_plane(hp(P), 1, 2, 2, None, 0, None) == 0
    assert capi.edgels_from_plane(P, []).shape == (0, 4)


def test_arithmetic_restatements_agree():
    """numpy forms == plain-Python forms, on the Sobel domain's edge and on random s16 pairs and triples."""
    rng = np.random.default_rng(21)
    gx = np.concatenate([rng.integers(-32768, 32768, 20000), [-32768, 32767, 0, 0, -1020, 1020, 1, -1]])
    gy = np.concatenate([rng.integers(-32768, 32768, 20000), [-32768, -32768, 0, 5, 1020, -1020, 1, 1]])
    gx[:4000] //= 64
    gy[2000:6000] //= 64
    assert np.array_equal(er.mag_q4(gx, gy), [er.mag_q4_scalar(int(a), int(b)) for a, b in zip(gx, gy)])
    assert np.array_equal(er.direction(gx, gy), [er.dir_scalar(int(a), int(b)) for a, b in zip(gx, gy)])
    abc = rng.integers(0, 741456, (20000, 3))
    abc[:8000] = rng.integers(0, 40, (8000, 3))
    t, ok = er.offsets(abc[:, 0], abc[:, 1], abc[:, 2])
    want = [er.offset_scalar(int(a), int(b), int(c)) for a, b, c in abc]
    assert np.array_equal(t, [w[0] for w in want]) and np.array_equal(ok, [w[1] for w in want])
    assert np.abs(t).max() == 128
    # the octant boundaries: tan 22.5 deg = 13573 / 32768 to 15 bits
    assert er.dir_scalar(32768, 13573) == 1 and er.dir_scalar(32767, 13572) == 0 and er.dir_scalar(100, 41) == 0
    assert er.dir_scalar(100, 42) == 1 and er.dir_scalar(100, -42) == 3 and er.dir_scalar(-100, -42) == 1
    assert er.dir_scalar(100, 241) == 1 and er.dir_scalar(100, 242) == 2 and er.dir_scalar(0, -3) == 2
    assert er.dir_scalar(0, 0) == 0 and er.dir_scalar(-7, 0) == 0


# ---- accuracy of the rule on straight edges -----------------------------------------------------------------------------
_PHI = np.vectorize(lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))))


def edge_plane(theta_deg: float, rho: float) -> np.ndarray:
    """40 x 40, round(255 * Phi(d / 1.4)), d = x cos(theta) + y sin(theta) - rho: a straight edge blurred by sigma 1.4."""
    yy, xx = np.mgrid[0:40, 0:40]
    t = math.radians(theta_deg)
    d = xx * math.cos(t) + yy * math.sin(t) - rho
    return np.round(255.0 * _PHI(d / 1.4)).astype(np.uint8)


ACCURACY = {}  # theta -> (pixels, unrefined mean, refined mean, refined max), filled by the test below


@pytest.mark.parametrize("theta", list(range(0, 181, 10)))
def test_refined_positions_lie_on_the_edge(theta):
    """Per angle, over eight sub-pixel phases of the line: every interior pixel with mag_q4 >= 800 that is a strict maximum
    along the rule's own step is refined, the refined positions are on average less than a quarter as far from the true line
    as the pixel centres, and none is further than 0.1 px.  (DESIGN.md section 23 has the table: centres 0.21-0.35 px,
    refined 0.011-0.037 px, largest 0.068 px.)"""
    t = math.radians(theta)
    ct, st = math.cos(t), math.sin(t)
    centre, refined_d = [], []
    for k in range(8):
        rho = 19.5 * ct + 19.5 * st + k / 8.0  # through the middle of the plane, in eight steps of 1/8 pixel
        P = edge_plane(theta, rho)
        yy, xx = np.mgrid[2:38, 2:38]
        idx = (yy * 40 + xx).reshape(-1)
        rec = capi.edgels_from_plane(P, idx)
        assert np.array_equal(rec, er.edgels_at(P, idx))
        x, y, gx, gy, mag, d, refined, _ = er.unpack(rec)
        b = rec[:, 3].view(np.uint32) & er.MAG_MASK
        steps = np.array(er.STEPS)[d]
        mags = lambda px, py: er.mag_q4(*er.sobel_pairs(P, py, px))
        px, py = idx % 40, idx // 40
        a, c = mags(px - steps[:, 0], py - steps[:, 1]), mags(px + steps[:, 0], py + steps[:, 1])
        pick = (b >= 800) & (b > a) & (b > c)
        assert refined[pick].all(), "a strict maximum along the step was not refined"
        centre.append(np.abs(px[pick] * ct + py[pick] * st - rho))
        refined_d.append(np.abs(x[pick] * ct + y[pick] * st - rho))
    centre, refined_d = np.concatenate(centre), np.concatenate(refined_d)
    assert centre.size >= 150  # (a phase that puts the line midway between two pixels has ties and no strict maximum)
    ACCURACY[theta] = (centre.size, centre.mean(), refined_d.mean(), refined_d.max())
    print(f"theta {theta:3d}: {centre.size} pixels, centre mean {centre.mean():.4f}, refined mean {refined_d.mean():.4f}, "
          f"max {refined_d.max():.4f}, ratio {centre.mean() / refined_d.mean():.1f}")
    assert refined_d.mean() < centre.mean() / 4
    assert refined_d.max() <= 0.1


# ---- the launch plan of the index-driven kernel --------------------------------------------------------------------------
def test_edgels_plan_one_item_below_and_above_the_cap():
    small = capi.edgels_plan(3, 16, 16, 1)
    assert (small.per_group, small.grid, small.trips, small.aux) == (256, 1, 1, 0)
    for h, w in ((16, 16), (70, 128), (2160, 3840)):
        grid = capi.edgels_plan(1, h, w, 1).grid
        assert grid == min(1024, max(1, -(-h * w // 1024)))
        full = grid * 256
        assert capi.edgels_plan(1, h, w, full).trips == 1 and capi.edgels_plan(1, h, w, full + 1).trips == 2
        assert capi.edgels_plan(1, h, w, full + 1).units == full + 1
    L = capi.load()
    out = np.zeros(5, np.uint64)
    for args in ((1, 16, 16, 0), (0, 16, 16, 5), (1, 1, 16, 5), (1, 16, 1, 5), (70000, 16, 16, 5)):
        assert L.canny_hip_selftest_edgels_plan(*args, capi._hp(out)) != 0
    assert L.canny_hip_selftest_edgels_plan(1, 16, 16, 5, None) == 1
    assert capi.launch_plan("points_rows", 4097, 256, 8).trips == 2  # the row kernel goes by the existing kind


# ---- header, bindings, command line ------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1300
    assert capi.load().canny_hip_version() >= 1300
    for word in ("13573", "CANNY_HIP_EDGEL_REFINED", "CANNY_HIP_EDGEL_INVALID", "CANNY_HIP_EDGEL_PART_LAYOUT",
                 "CANNY_HIP_EDGEL_PART_REFINE", "floor division", "ALONG the edge", "Devernay"):
        assert word in header, word
    for name in ("canny_hip_dev_canny_edgels", "canny_hip_dev_edgels_at", "canny_hip_canny_edgels",
                 "canny_hip_edgels_from_plane", "canny_hip_dev_edgels_arith", "canny_hip_edgels_profile_get",
                 "canny_hip_selftest_edgels_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert len(capi.PLAN_KINDS) == 18


def test_unpack_helpers():
    P = np.tile(np.array([0, 0, 10, 20, 30, 30, 30, 30], np.uint8), (6, 1))
    rec = capi.edgels_from_plane(P, [2 * 8 + 3, 999])
    x, y = capi.edgels_xy(rec)
    gx, gy = capi.edgels_gradient(rec)
    d, refined, invalid = capi.edgels_flags(rec)
    assert (x[0], y[0], gx[0], gy[0], capi.edgels_magnitude(rec)[0]) == (2.5, 2.0, 80, 0, 80.0)
    assert (d[0], refined[0], invalid[0], invalid[1], refined[1]) == (0, True, False, True, False)


def test_cli_e_grammar(tmp_path):
    """-e takes no value: with fewer than three positionals the usage text (which names it) is printed and the program
    exits 0 before any device is touched, as for every other flag; nothing is written."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, "1.0", "50", "-e", "-o", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-e: sub-pixel edgel" in r.stderr
    assert "canny_edgels.txt" in r.stderr
    r = subprocess.run([exe, "-e", "1.0", "150", "50", "-o", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_edgels_host.cpp has its own main and is compiled together with csrc/canny_edgels_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_edgels_host"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_edgels_host.cpp"),
                           os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_edgels_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed planes ok" in r.stdout, r.stdout + r.stderr
