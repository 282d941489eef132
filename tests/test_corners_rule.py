"""The corner rule (include/canny_hip.h) without a GPU: the host function
canny_hip_corners_from_plane against tests/corners_rule.py word for word, the rule's two Python forms against each other,
the response arithmetic against Python ints, the designed accuracy and tie cases, every refused call, the launch plans."""
import os
import re
import subprocess

import numpy as np
import pytest

import corners_rule as cr
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(cr.MIN_EIGEN, 0), (cr.HARRIS, 10)]
SENT = -0x5A5A5A5A5A5A5A5B


def same(P, mode, block, k_q8, quality_q16=655, min_response=0, min_dist=0, corners_max=256):
    """The host function and the numpy rule on one plane: records, counts, maximum and every response."""
    rec, nc, rmax, R = capi.corners_from_plane(P, mode, block, k_q8, quality_q16, min_response, min_dist, corners_max,
                                               want_response=True)
    want, want_nc, want_rmax, want_R = cr.corners(P, mode, block, k_q8, quality_q16, min_response, min_dist, corners_max)
    assert np.array_equal(R, want_R), "the response planes differ"
    assert (nc, rmax) == (want_nc, want_rmax), (nc, rmax, want_nc, want_rmax)
    assert np.array_equal(rec, want), f"{len(rec)} records against {len(want)}"
    rec2, nc2, rmax2, _ = capi.corners_from_plane(P, mode, block, k_q8, quality_q16, min_response, min_dist, corners_max)
    assert np.array_equal(rec2, rec) and (nc2, rmax2) == (nc, rmax), "the outputs depend on the response plane"
    return rec, nc, rmax


# ---- the host function against the rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [3, 5, 7])
@pytest.mark.parametrize("mode,k_q8", [(0, 0), (1, 0), (1, 10), (1, 33), (1, 64)])
def test_host_function_equals_the_rule_on_random_planes(mode, k_q8, block):
    rng = np.random.default_rng(100 * mode + 10 * block + k_q8)
    P = rng.integers(0, 256, (41, 57), dtype=np.uint8)
    rec, nc, rmax = same(P, mode, block, k_q8, quality_q16=3000, min_dist=5, corners_max=64)
    if k_q8 < 64:
        assert nc > 20 and 0 < len(rec) < nc
    else:
        assert nc == 0 and rmax <= 0  # 256 * det - 64 * trace^2 = -64 (a - b)^2 - 256 sxy^2
    # smoother planes, every quality and an absolute floor
    Q = cr.blur14641(rng.integers(0, 256, (33, 70), dtype=np.uint8) // 64 * 64)
    for q, floor_, md, cmax in ((0, 0, 0, 4096), (65536, 0, 0, 7), (655, 10 ** 5, 3, 50), (20000, 0, 10, 1)):
        same(Q, mode, block, k_q8, q, floor_, md, cmax)


@pytest.mark.parametrize("mode,k_q8", MODES)
def test_flat_plane_has_no_candidate(mode, k_q8):
    for value in (0, 77, 255):
        for block in (3, 5, 7):
            rec, nc, rmax = same(np.full((12, 19), value, np.uint8), mode, block, k_q8, quality_q16=0)
            assert (len(rec), nc, rmax) == (0, 0, 0)


@pytest.mark.parametrize("shape", [(2, 2), (2, 70), (70, 2)])
@pytest.mark.parametrize("mode,k_q8", MODES)
def test_thin_frames(shape, mode, k_q8):
    rng = np.random.default_rng(shape[0] * 71 + shape[1] + mode)
    for block in (3, 5, 7):
        P = rng.integers(0, 256, shape, dtype=np.uint8)
        rec, nc, _ = same(P, mode, block, k_q8, quality_q16=100, corners_max=100)
        assert nc >= 1 or mode == cr.HARRIS
    P = np.array([[0, 255], [255, 0]], np.uint8)
    same(P, mode, 3, k_q8)


@pytest.mark.parametrize("mode,k_q8", MODES)
def test_plain_int_form_at_every_pixel(mode, k_q8):
    rng = np.random.default_rng(911 + mode)
    P = cr.blur14641(rng.integers(0, 2, (9, 11), dtype=np.uint8) * 255)
    for block in (3, 5, 7):
        R = cr.response_plane(P, mode, block, k_q8)
        want = [[cr.response_scalar(P, y, x, mode, block, k_q8) for x in range(11)] for y in range(9)]
        assert R.tolist() == want
        cut = cr.threshold_of(int(R.max()), 655, 0)
        cand = [[cr.candidate_scalar(P, y, x, mode, block, k_q8, cut) for x in range(11)] for y in range(9)]
        assert cr.candidates(R, cut).tolist() == cand
        _, nc, _ = same(P, mode, block, k_q8, corners_max=99)
        assert nc == sum(map(sum, cand))


def test_plateaus_go_to_the_first_pixel_in_raster_order():
    R = np.zeros((6, 8), np.int64)
    R[1:3, 2:5] = 9          # a plateau: its first pixel wins
    R[4, 0] = R[4, 1] = 5    # two equal neighbours on the frame's edge
    R[5, 7] = 1
    got = np.argwhere(cr.candidates(R, 1)).tolist()
    assert got == [[1, 2], [4, 0], [5, 7]]


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def test_response_arithmetic_against_python_ints():
    t = cr.arith_triples()
    assert len(t) >= 1 << 20
    f = capi.corner_response_of
    for mode, k_q8 in ((0, 0), (1, 10), (1, 64)):
        rows = t.tolist() if mode == 0 else t[:200000].tolist()
        want = [cr.response_of(a, b, c, mode, k_q8) for a, b, c in rows]
        got = [f(a, b, c, mode, k_q8) for a, b, c in rows]
        assert got == want
        assert cr.response_array(t[:len(rows), 0], t[:len(rows), 1], t[:len(rows), 2], mode, k_q8).tolist() == want
    M = cr.MAX_SUM
    assert cr.response_of(M, M, 0, 0, 0) == 2 * M < 1 << 27
    assert cr.response_of(M, M, 0, 1, 0) == 256 * M * M < 1 << 60
    for bad in ((-1, 0, 0, 0, 0), (0, M + 1, 0, 0, 0), (0, 0, M + 1, 0, 0), (0, 0, -M - 1, 1, 3), (1, 1, 1, 2, 0),
                (1, 1, 1, 0, 1), (1, 1, 1, 1, 65), (1, 1, 1, 1, -1), (1, 1, 1, -1, 0)):
        with pytest.raises(capi.CannyHipError) as ei:
            f(*bad)
        assert ei.value.status == 1


# ---- the designed cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [3, 5, 7])
@pytest.mark.parametrize("mode,k_q8", MODES)
def test_the_square_has_four_corners(mode, k_q8, block):
    rec, nc, _ = same(cr.square_plane(), mode, block, k_q8)
    assert nc == 4 and len(rec) == 4
    lo, hi = (22, 41) if block == 7 else (21, 42)
    assert sorted(map(tuple, rec[:, :2].tolist())) == [(lo, lo), (lo, hi), (hi, lo), (hi, hi)]
    for x, y in rec[:, :2]:
        assert min(abs(x - 20), abs(x - 43)) <= 2 and min(abs(y - 20), abs(y - 43)) <= 2
    assert rec[:, 3].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("mode,k_q8", MODES)
def test_the_checkerboard_ties(mode, k_q8):
    P = cr.checkerboard_plane()
    rec, nc, rmax = same(P, mode, 5, k_q8, corners_max=4096)
    assert nc == 196 and len(rec) == 196
    values, counts = np.unique(rec[:, 2], return_counts=True)
    assert counts.tolist() == [98, 98] and values[1] == rmax
    base = rec[:, 1] * 64 + rec[:, 0]
    assert (np.diff(base[:98]) > 0).all() and (np.diff(base[98:]) > 0).all(), "ties go by ascending base"
    for cmax in (50, 98, 99, 150):          # the cut inside a tie group, on its end, in the next one
        for md in (0, 6, 9):
            got, nc2, _ = same(P, mode, 5, k_q8, min_dist=md, corners_max=cmax)
            assert nc2 == 196
            if md == 0:
                assert np.array_equal(got, rec[:cmax])
            else:                            # four candidates sit round every crossing, 5 px apart: some are removed
                assert 0 < len(got) < cmax and got[-1, 3] > len(got) - 1
                assert np.array_equal(got[:, :3], rec[got[:, 3], :3]), "rank is the position in the selected order"


# ---- refused calls ---------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    L = capi.load()
    P = np.arange(48, dtype=np.uint8).reshape(6, 8)
    good = dict(plane=P, h=6, w=8, mode=0, block=3, k=0, q=655, floor_=0, md=0, cmax=4)

    def call(**kw):
        a = dict(good, **kw)
        rec = np.full(4 * 4 + 8, SENT, np.int64)
        resp = np.full(48 + 8, SENT, np.int64)
        n, nc, rmax = capi.C.c_int(-7), capi.C.c_int(-7), capi.C.c_longlong(-7)
        plane = capi._hp(a["plane"]) if a["plane"] is not None else None
        st = L.canny_hip_corners_from_plane(plane, a["h"], a["w"], a["mode"], a["block"], a["k"], a["q"], a["floor_"],
                                            a["md"], a["cmax"], capi._hp(rec) if a.get("rec", 1) else None,
                                            capi.C.byref(n) if a.get("count", 1) else None, capi.C.byref(nc),
                                            capi.C.byref(rmax), capi._hp(resp))
        if st:
            assert (rec == SENT).all() and (resp == SENT).all() and (n.value, nc.value, rmax.value) == (-7, -7, -7)
        else:
            assert (rec[16:] == SENT).all() and (resp[48:] == SENT).all()
        return st

    assert call() == 0
    invalid = [dict(plane=None), dict(rec=0), dict(count=0), dict(h=1), dict(w=1), dict(h=0), dict(mode=2), dict(mode=-1),
               dict(block=4), dict(block=1), dict(block=9), dict(k=1), dict(mode=1, k=65), dict(mode=1, k=-1), dict(q=-1),
               dict(q=65537), dict(floor_=-1), dict(md=-1), dict(cmax=0), dict(cmax=-3)]
    for kw in invalid:
        assert call(**kw) == 1, kw
    for kw in (dict(cmax=4097), dict(h=65536, w=32768), dict(h=1 << 20, w=1 << 20)):
        assert call(**kw) == 2, kw
    # a misaligned record buffer
    raw = np.zeros(8 * 20, np.uint8)
    off = (8 - raw.ctypes.data % 8) % 8 + 4
    n = capi.C.c_int(-7)
    st = L.canny_hip_corners_from_plane(capi._hp(P), 6, 8, 0, 3, 0, 655, 0, 0, 4, capi.C.c_void_p(raw.ctypes.data + off),
                                        capi.C.byref(n), None, None, None)
    assert st == 1 and n.value == -7 and not raw.any()


# ---- the launch plans --------------------------------------------------------------------------------------------------------
def test_plans_one_item_below_and_above_a_full_trip():
    for h, w in ((2, 2), (16, 64), (17, 64), (16, 65), (70, 128), (2160, 3840)):
        plan, chunk = capi.corners_plan("tiles", 3, h, w)
        tiles = -(-h // 16) * -(-w // 64)
        assert (plan.units, plan.per_group, plan.grid, plan.aux, chunk) == (tiles, 1, min(tiles, 1024), 0, 3)
        assert plan.trips == -(-tiles // 1024)
    assert capi.corners_plan("tiles", 1, 16 * 32, 64 * 32)[0].trips == 1       # 1024 tiles: a full trip
    assert capi.corners_plan("tiles", 1, 16 * 32 + 1, 64 * 32)[0].trips == 2   # one row of tiles more
    assert capi.corners_plan("tiles", 1, 16 * 32, 64 * 32 - 63)[0].trips == 1
    assert capi.corners_plan("tiles", 1, 16 * 32, 64 * 32 + 1)[0].trips == 2
    assert capi.corners_plan("tiles", 5000, 16, 16)[1] == 1024                # frames of a chunk
    full = 1024 * 256
    for n, trips in ((1, 1), (full - 1, 1), (full, 1), (full + 1, 2), (2 * full + 1, 3)):
        plan, _ = capi.corners_plan("arith", n=n)
        assert (plan.units, plan.per_group, plan.trips) == (n, 256, trips)
        assert plan.grid == min(1024, -(-n // 256))
    L = capi.load()
    out = np.zeros(6, np.uint64)
    for args in ((0, 1, 1, 16, 0), (0, 1, 16, 1, 0), (0, 0, 16, 16, 0), (0, 70000, 16, 16, 0), (1, 1, 16, 16, 0),
                 (2, 1, 16, 16, 5), (-1, 1, 16, 16, 5)):
        assert L.canny_hip_selftest_corners_plan(*args, capi._hp(out)) != 0, args
    assert L.canny_hip_selftest_corners_plan(0, 1, 16, 16, 0, None) == 1
    assert len(capi.PLAN_KINDS) == 18  # the corners' launches have no kind of their own


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1900
    assert capi.load().canny_hip_version() >= 1900
    for word in ("CANNY_HIP_CORNER_WORDS 4", "CANNY_HIP_CORNERS_MIN_EIGEN = 0", "CANNY_HIP_CORNERS_HARRIS = 1", "ceil_sqrt",
                 "50,979,600", "quality_q16", "min_response", "cornerSubPix", "CANNY_HIP_CORNER_PART_MAX",
                 "CANNY_HIP_CORNER_PART_ACCEPT", "Gaussian-weighted", "0.19.0"):
        assert word in header, word
    for name in ("canny_hip_dev_canny_corners", "canny_hip_dev_corners_plane", "canny_hip_canny_corners",
                 "canny_hip_corners_from_plane", "canny_hip_corner_response_of", "canny_hip_dev_corners_arith",
                 "canny_hip_corners_profile_get", "canny_hip_selftest_corners_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert capi.CORNER_DTYPE.itemsize == 8 * capi.CORNER_WORDS == 32
    assert (capi.CORNERS_MAX_SUM, cr.MAX_SUM) == (50979600, 50979600)


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_corners_host.cpp has its own main and is compiled together with csrc/canny_corners_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_corners_host"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_corners_host.cpp"),
                           os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_corners_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "designed planes ok" in r.stdout, r.stdout + r.stderr
