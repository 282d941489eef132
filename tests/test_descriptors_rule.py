"""CPU-only checks of the corner-descriptor and Hamming-matching rule (include/canny_hip.h): the
committed pattern against its generator, canny_hip_corner_descriptors_from_plane and canny_hip_match_descriptors against
tests/descriptors_rule.py word for word, the rule's two Python forms against each other, the designed scene, every refused
call, the launch plans."""
import os
import re
import subprocess

import numpy as np
import pytest

import corners_rule as cr
import descriptors_rule as dr
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A5A5A5A5A


# ---- the pattern -----------------------------------------------------------------------------------------------------------
def test_generator_takes_491_attempts():
    tests, attempts = dr.base_tests()
    assert (len(tests), attempts) == (256, 491)


def test_committed_table_equals_the_generator():
    pat = dr.pattern()
    for k in range(32):
        assert np.array_equal(capi.descriptor_pattern(k), pat[k]), k
    text = open(os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_desc_pattern.h")).read()
    numbers = re.sub(r"/\*.*?\*/", "", text, flags=re.S).replace("\n", " ").split(",")
    values = np.array([int(v) for v in numbers if v.strip()], np.int8)
    assert np.array_equal(values.reshape(32, 256, 4), pat)
    L = capi.load()
    out = np.full((257, 4), 99, np.int8)
    for k in (-1, 32, 1000):
        assert L.canny_hip_descriptor_pattern(k, capi._hp(out)) == 1 and (out == 99).all()
    assert L.canny_hip_descriptor_pattern(0, None) == 1
    assert L.canny_hip_descriptor_pattern(31, capi._hp(out)) == 0 and (out[256] == 99).all()


def test_pattern_is_bounded_distinct_and_never_degenerate():
    pat = dr.pattern().astype(int)
    assert np.abs(pat).max() == 13
    for k in range(32):
        tests = set(map(tuple, pat[k].tolist()))
        either = tests | {(c, d, a, b) for a, b, c, d in tests}
        assert len(tests) == 256 and len(either) == 512, f"rotation {k}: tests coincide"
        assert all((a, b) != (c, d) for a, b, c, d in tests), k
    assert np.array_equal(pat[0], np.array(dr.base_tests()[0]))


def test_rotation_by_eight_steps_is_the_quarter_turn():
    """rot_{k+8} = (x, y) -> (-y, x) of rot_k: it holds exactly for EVERY k, because no product x * C - y * S of a pattern
    offset falls on a half (v + 8192 a multiple of 16384), the one place where rd(-v) != -rd(v)."""
    pat = dr.pattern().astype(int)
    for k in range(32):
        p, q = pat[k], pat[(k + 8) % 32]
        assert np.array_equal(np.stack([-p[:, 1], p[:, 0], -p[:, 3], p[:, 2]], 1), q), k
    tests, _ = dr.base_tests()
    for k in range(32):
        c, s = dr.cos_q14(k), dr.sin_q14(k)
        for ax, ay, bx, by in tests:
            for x, y in ((ax, ay), (bx, by)):
                assert (x * c - y * s + 8192) % 16384 != 0 and (x * s + y * c + 8192) % 16384 != 0, (k, x, y)
    assert [dr.cos_q14(k) for k in range(9)] == list(dr.COS_Q14)
    for k in range(32):
        assert abs(dr.cos_q14(k) - 16384 * np.cos(2 * np.pi * k / 32)) <= 0.5 + 1e-9
        assert abs(dr.sin_q14(k) - 16384 * np.sin(2 * np.pi * k / 32)) <= 0.5 + 1e-9


# ---- the host function against the rule ------------------------------------------------------------------------------------
def same(P, xy, steered):
    desc, meta = capi.corner_descriptors_from_plane(P, xy, steered)
    want, want_meta = dr.describe(P, xy, steered)
    assert np.array_equal(meta, want_meta), "meta words differ"
    assert np.array_equal(desc, want), "descriptor words differ"
    return desc, meta


def border_records(h, w):
    """Records at every border position of a frame, a few inside, and some outside it."""
    xs = sorted({0, 1, 14, 15, 16, w // 2, w - 17, w - 16, w - 15, w - 2, w - 1} & set(range(w)))
    ys = sorted({0, 1, 14, 15, 16, h // 2, h - 17, h - 16, h - 15, h - 2, h - 1} & set(range(h)))
    inside = [(x, y) for y in ys for x in xs]
    outside = [(-1, 0), (0, -1), (w, 0), (0, h), (w + 100, h + 100), (-(1 << 40), 3), (3, 1 << 40), (-1, -1)]
    return np.array(inside + outside, np.int64)


@pytest.mark.parametrize("steered", [False, True])
def test_host_function_equals_the_rule_on_random_planes(steered):
    rng = np.random.default_rng(5 + steered)
    for shape in ((41, 57), (33, 70), (64, 64)):
        P = rng.integers(0, 256, shape, dtype=np.uint8)
        Q = cr.blur14641(P // 64 * 64)
        for plane in (P, Q):
            xy = np.concatenate([border_records(*shape),
                                 np.stack([rng.integers(0, shape[1], 60), rng.integers(0, shape[0], 60)], 1)])
            desc, meta = same(plane, xy, steered)
            inside = meta >= 0
            assert inside.sum() > 60 and (~inside).sum() == 8 and not desc[~inside].any()
            if steered:
                assert len(set((meta[inside] & 255).tolist())) > 8, "the orientations vary"
            else:
                assert not (meta[inside] & 255).any()


def test_vector_rule_equals_the_scalar_rule():
    rng = np.random.default_rng(11)
    P = cr.blur14641(rng.integers(0, 256, (24, 37), dtype=np.uint8))
    xy = border_records(24, 37)[::3]
    for steered in (False, True):
        words, meta = dr.describe(P, xy, steered)
        for i, (x, y) in enumerate(xy.tolist()):
            w, m = dr.describe_scalar(P, x, y, steered)
            assert w == [int(v) for v in words[i]] and m == meta[i], (i, x, y)


@pytest.mark.parametrize("value", [0, 77, 255])
def test_flat_plane_gives_k_0_and_zero_descriptors(value):
    P = np.full((40, 52), value, np.uint8)
    for steered in (False, True):
        desc, meta = same(P, border_records(40, 52)[:-8], steered)
        assert not desc.any() and not (meta & 255).any()
        assert meta[np.flatnonzero((border_records(40, 52)[:-8] == (26, 20)).all(1))[0]] == 0


@pytest.mark.parametrize("shape", [(2, 2), (2, 70), (70, 2)])
def test_thin_frames(shape):
    rng = np.random.default_rng(shape[0] * 71 + shape[1])
    P = rng.integers(0, 256, shape, dtype=np.uint8)
    h, w = shape
    xy = np.array([(x, y) for y in range(h) for x in range(w)] + [(-1, 0), (w, h - 1), (0, h)], np.int64)
    for steered in (False, True):
        _, meta = same(P, xy, steered)
        assert (meta[:-3] >= 256).all() and (meta[-3:] == -1).all()


def test_frame_corners_and_the_border_flag():
    rng = np.random.default_rng(3)
    P = rng.integers(0, 256, (50, 60), dtype=np.uint8)
    xy = np.array([(0, 0), (59, 0), (0, 49), (59, 49), (15, 15), (44, 34), (14, 15), (15, 14), (45, 34), (44, 35)], np.int64)
    _, meta = same(P, xy, True)
    assert (meta >> 8).tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1]


def test_steering_follows_a_quarter_turn():
    """A plane turned by 90 degrees turns the orientation by 8 steps and leaves the steered descriptor unchanged, exactly:
    the disc, the pattern (see above) and the clamped reads all commute with the quarter turn away from the border."""
    rng = np.random.default_rng(8)
    P = cr.blur14641(rng.integers(0, 256, (60, 60), dtype=np.uint8))
    xy = np.stack([rng.integers(16, 44, 30), rng.integers(16, 44, 30)], 1)
    R = np.ascontiguousarray(np.rot90(P, -1))                        # clockwise: (x, y) -> (59 - y, x), y down
    xr = np.stack([59 - xy[:, 1], xy[:, 0]], 1)
    d0, m0 = same(P, xy, True)
    d1, m1 = same(R, xr, True)
    assert np.array_equal(d0, d1) and np.array_equal((m0 + 8) % 32, m1)


# ---- the host matcher ------------------------------------------------------------------------------------------------------
random_set = dr.random_set


SETTINGS = [(64, 205, 1), (0, 0, 0), (256, 0, 1), (256, 256, 0), (40, 1, 1), (100, 205, 0), (256, 205, 1)]


def same_match(q, t, max_distance, ratio_q8, options):
    got, n = capi.match_descriptors(q, t, max_distance, ratio_q8, options)
    want, want_n = dr.match(q, t, max_distance, ratio_q8, options)
    assert np.array_equal(got, want) and n == want_n, (len(q), len(t), max_distance, ratio_q8, options)
    return got, n


@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (1, 1), (2, 1), (1, 2), (63, 64), (64, 65), (65, 63), (257, 300),
                                   (300, 257)])
def test_host_matcher_equals_the_rule_on_random_sets(nq, nt):
    rng = np.random.default_rng(1000 * nq + nt)
    both = random_set(rng, nq + nt)
    q, t = both[:nq], both[nq:]
    seen = 0
    for s in SETTINGS:
        got, _ = same_match(q, t, *s)
        seen |= int(np.bitwise_or.reduce(got[:, 3])) if nq else 0
    if nt == 0:
        assert (got[:, 0] == -1).all() and (got[:, 1:3] == 257).all() and not (got[:, 3] & 4).any()
    if nt == 1 and nq:
        assert (got[:, 0] == 0).all() and (got[:, 2] == 257).all()
    if min(nq, nt) >= 63:
        assert seen == 15


def test_plain_int_matcher_equals_the_vector_rule():
    rng = np.random.default_rng(77)
    both = random_set(rng, 40, 12)
    for s in SETTINGS:
        a, na = dr.match(both[:23], both[23:], *s)
        b, nb = dr.match_scalar(both[:23], both[23:], *s)
        assert np.array_equal(a, b) and na == nb, s


duplicated_sets = dr.duplicated_sets


def test_duplicates_go_to_the_smaller_index():
    q, t = duplicated_sets(np.random.default_rng(21))
    for s in SETTINGS:
        got, _ = same_match(q, t, *s)
    got, _ = same_match(q, t, 256, 205, 1)
    assert (got[:20, 1] == 0).all() and (got[:20, 2] == 0).all(), "a duplicate is at distance 0 twice"
    assert got[:20, 0].tolist() == list(range(5, 15)) * 2
    assert (got[:10, 3] & 4).all() and not (got[10:20, 3] & 4).any(), "the mutual test goes to the smaller query"
    assert not (got[:20, 3] & 2).any(), "0 * 256 < 205 * 0 does not hold"
    got0, _ = same_match(q, t, 256, 0, 1)
    assert (got0[:10, 3] == 15).all()
    same_match(q, q, 0, 0, 1)


# ---- the scene -------------------------------------------------------------------------------------------------------------
_SCENE = {}


def scene():
    if not _SCENE:
        big = synth_frame(300, 400, 7)
        A = cr.blur14641(big[10:250, 10:330])
        rng = np.random.default_rng(1)
        noisy = np.clip(big[14:254, 17:337].astype(np.int64) + rng.integers(-4, 5, (240, 320)), 0, 255).astype(np.uint8)
        B = cr.blur14641(noisy)
        rng = np.random.default_rng(1)
        turned = np.clip(big[10:250, 10:330].astype(np.int64) + rng.integers(-4, 5, (240, 320)), 0, 255).astype(np.uint8)
        R = cr.blur14641(np.ascontiguousarray(np.rot90(turned)))
        for name, P in (("A", A), ("B", B), ("R", R)):
            _SCENE[name] = (P, cr.corners(P, quality_q16=655, min_dist=8, corners_max=256)[0])
    return _SCENE


def right_matches(ca, cb, matches, expect):
    n_acc = n_right = 0
    for i, (j, _, _, flags) in enumerate(matches.tolist()):
        if flags & 8:
            ex, ey = expect(int(ca[i, 0]), int(ca[i, 1]))
            n_acc += 1
            n_right += abs(int(cb[j, 0]) - ex) <= 2 and abs(int(cb[j, 1]) - ey) <= 2
    return n_acc, n_right


@pytest.mark.parametrize("steered", [False, True])
def test_scene_views_a_and_b(steered):
    (A, ca), (B, cb) = scene()["A"], scene()["B"]
    assert len(ca) == 48 and len(cb) == 48
    da, _ = capi.corner_descriptors_from_plane(A, ca, steered)
    db, _ = capi.corner_descriptors_from_plane(B, cb, steered)
    got, n = capi.match_descriptors(da, db, 64, 205, capi.MATCH_CROSS_CHECK)
    n_acc, n_right = right_matches(ca, cb, got, lambda x, y: (x - 7, y - 4))
    print(f"A/B steered={steered}: accepted {n_acc}, right {n_right}")
    assert n == n_acc and n_acc >= 40 and n_acc - n_right <= 2


def test_scene_rotated_view():
    (A, ca), (R, cr_) = scene()["A"], scene()["R"]
    expect = lambda x, y: (y, 319 - x)   # np.rot90 takes pixel (y, x) to (W - 1 - x, y)
    for steered, check in ((True, lambda right: right >= 40), (False, lambda right: right <= 5)):
        da, _ = capi.corner_descriptors_from_plane(A, ca, steered)
        db, _ = capi.corner_descriptors_from_plane(R, cr_, steered)
        got, _ = capi.match_descriptors(da, db, 64, 205, capi.MATCH_CROSS_CHECK)
        n_acc, n_right = right_matches(ca, cr_, got, expect)
        print(f"rotated steered={steered}: accepted {n_acc}, right {n_right}")
        assert check(n_right), (steered, n_acc, n_right)
        for s in ((256, 0, 0), (64, 0, 1)):
            if not steered:
                loose, _ = capi.match_descriptors(da, db, *s)
                assert right_matches(ca, cr_, loose, expect)[1] <= 5


# ---- refused calls ---------------------------------------------------------------------------------------------------------
def test_refused_descriptor_calls_write_nothing():
    L = capi.load()
    P = np.arange(48, dtype=np.uint8).reshape(6, 8)
    rec = np.array([[1, 2, 0, 0], [3, 4, 0, 0]], np.int64)

    def call(plane=P, h=6, w=8, corners=rec, count=2, options=0, desc=1, meta=1):
        d = np.full(2 * 4 + 8, SENT, np.uint64)
        m = np.full(2 + 8, -7, np.int32)
        st = L.canny_hip_corner_descriptors_from_plane(capi._hp(plane) if plane is not None else None, h, w,
                                                       capi._hp(corners) if corners is not None else None, count, options,
                                                       capi._hp(d) if desc else None, capi._hp(m) if meta else None)
        if st:
            assert (d == SENT).all() and (m == -7).all()
        else:
            assert (d[4 * count:] == SENT).all() and (m[count:] == -7).all()
        return st

    assert call() == 0 and call(count=0) == 0 and call(count=0, corners=None) == 0 and call(options=1) == 0
    for kw in (dict(plane=None), dict(corners=None), dict(desc=0), dict(meta=0), dict(h=1), dict(w=1), dict(h=0),
               dict(count=-1), dict(options=2), dict(options=-1)):
        assert call(**kw) == 1, kw
    for kw in (dict(count=4097), dict(h=65536, w=32768)):
        assert call(**kw) == 2, kw
    raw = np.zeros(8 * 20, np.uint8)
    off = (8 - raw.ctypes.data % 8) % 8 + 4
    m = np.full(4, -7, np.int32)
    st = L.canny_hip_corner_descriptors_from_plane(capi._hp(P), 6, 8, capi._hp(rec), 2, 0,
                                                   capi.C.c_void_p(raw.ctypes.data + off), capi._hp(m))
    assert st == 1 and not raw.any() and (m == -7).all()


def test_refused_match_calls_write_nothing():
    L = capi.load()
    q = random_set(np.random.default_rng(1), 3)
    t = random_set(np.random.default_rng(2), 4)

    def call(qd=q, nq=3, td=t, nt=4, md=64, ratio=205, options=1, out=1, acc=1):
        m = np.full(3 * 4 + 8, -7, np.int32)
        a = capi.C.c_int(-7)
        st = L.canny_hip_match_descriptors(capi._hp(qd) if qd is not None else None, nq,
                                           capi._hp(td) if td is not None else None, nt, md, ratio, options,
                                           capi._hp(m) if out else None, capi.C.byref(a) if acc else None)
        if st:
            assert (m == -7).all() and a.value == -7
        else:
            assert (m[4 * nq:] == -7).all()
        return st

    assert call() == 0 and call(nt=0, td=None) == 0 and call(nq=0, qd=None, out=0) == 0
    for kw in (dict(qd=None), dict(td=None), dict(out=0), dict(acc=0), dict(nq=-1), dict(nt=-1), dict(md=-1), dict(md=257),
               dict(ratio=-1), dict(ratio=257), dict(options=2), dict(options=-1)):
        assert call(**kw) == 1, kw
    for kw in (dict(nq=4097), dict(nt=4097)):
        assert call(**kw) == 2, kw


# ---- the launch plans ------------------------------------------------------------------------------------------------------
def test_plans_one_item_below_and_above_a_full_trip():
    full = 2048 * 4
    for n, stride, trips in ((1, 1, 1), (1, 4096, 1), (2, 4096, 1), (3, 4096, 2), (full - 1, 1, 1), (full, 1, 1),
                             (full + 1, 1, 2), (65535, 4096, 32768)):
        plan = capi.descriptors_plan("describe", n, stride)
        assert (plan.units, plan.per_group, plan.aux, plan.trips) == (n * stride, 4, 0, trips)
        assert plan.grid == min(2048, -(-n * stride // 4))
    for n, stride, units in ((1, 1, 1), (1, 256, 1), (1, 257, 2), (127, 4096, 2032), (2047, 256, 2047), (2048, 256, 2048),
                             (2049, 256, 2049), (1025, 300, 2050), (1 << 20, 4096, 1 << 24)):
        plan = capi.descriptors_plan("match", n, stride)
        assert (plan.units, plan.per_group, plan.grid, plan.aux) == (units, 1, min(units, 2048), 0)
        assert plan.trips == -(-units // 2048)
    L = capi.load()
    out = np.zeros(5, np.uint64)
    for args in ((0, 0, 16), (0, 1, 0), (0, 1, 4097), (0, 65536, 1), (1, 0, 16), (1, (1 << 20) + 1, 16), (1, 1, 4097),
                 (2, 1, 16), (-1, 1, 16)):
        assert L.canny_hip_selftest_descriptors_plan(*args, capi._hp(out)) != 0, args
    assert L.canny_hip_selftest_descriptors_plan(0, 1, 16, None) == 1
    assert not out.any()
    assert len(capi.PLAN_KINDS) == 18  # the descriptors' launches have no kind of their own


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2000
    assert capi.load().canny_hip_version() >= 2000
    for word in ("CANNY_HIP_DESC_BITS 256", "CANNY_HIP_DESC_RADIUS 15", "CANNY_HIP_DESC_STEERED = 1", "0x43414E59",
                 "1664525", "1013904223", "491 attempts", "16069", "CANNY_HIP_MATCH_CROSS_CHECK = 1",
                 "CANNY_HIP_DESC_PART_DESCRIBE", "CANNY_HIP_DESC_PART_FINALIZE", "RANSAC", "scale pyramids", "0.20.0"):
        assert word in header, word
    for name in ("canny_hip_dev_canny_corner_descriptors", "canny_hip_dev_corner_descriptors",
                 "canny_hip_canny_corner_descriptors", "canny_hip_corner_descriptors_from_plane",
                 "canny_hip_descriptor_pattern", "canny_hip_dev_match_descriptors", "canny_hip_match_descriptors",
                 "canny_hip_descriptors_profile_get", "canny_hip_selftest_descriptors_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert capi.DESC_MATCH_DTYPE.itemsize == 4 * capi.MATCH_WORDS
    assert (capi.DESC_BITS, capi.DESC_RADIUS, capi.DESC_ROTATIONS) == (dr.DESC_BITS, dr.DESC_RADIUS, dr.DESC_ROTATIONS)
    assert capi.consecutive_pairs(4).tolist() == [[0, 1], [1, 2], [2, 3]] and capi.consecutive_pairs(1).shape == (0, 2)


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_descriptors_host.cpp has its own main and is compiled together with csrc/canny_descriptors_host.cpp
    alone: nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_descriptors_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_descriptors_host.cpp"),
                           os.path.join(csrc, "canny_descriptors_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "descriptors ok" in r.stdout, r.stdout + r.stderr
