"""CPU-only checks of the frame-to-frame motion rule (include/canny_hip.h): canny_hip_estimate_motion
(plain C++) against tests/motion_rule.py word for word on designed sets, the width bounds with Python ints as the judge, every
refused call, the scene of tests/test_descriptors_rule.py, and the host rule under the host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_rule as mr
from canny_edge_amd import capi
from test_descriptors_rule import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A5A5A5A5A


def same(qc, tc, matches, model, thr_q4, hypotheses, seed):
    got, flags = capi.estimate_motion(qc, tc, matches, model, thr_q4, hypotheses, seed)
    want, want_flags = mr.estimate(qc, len(qc), tc, len(tc), matches, model, thr_q4, hypotheses, seed)
    assert got.tolist() == want.tolist(), (model, thr_q4, hypotheses, seed)
    assert np.array_equal(flags, want_flags), "inlier flags differ"
    return got, flags


# model, (a11, a12, a21, a22, tx, ty)
MOTIONS = {"shift": (mr.TRANSLATION, (1, 0, 0, 1, 5, 37)), "quarter turn about a point": (mr.SIMILARITY, (0, -1, 1, 0, 700, 20)),
           "scale 2": (mr.SIMILARITY, (2, 0, 0, 2, 3, 4)), "shear": (mr.AFFINE, (1, 1, 0, 1, 7, 9))}


@pytest.mark.parametrize("name", sorted(MOTIONS))
@pytest.mark.parametrize("wrong", [30, 40, 50])
def test_exact_integer_motions_are_refitted_exactly(name, wrong):
    model, motion = MOTIONS[name]
    rng = np.random.default_rng(len(name) * 100 + wrong)
    qc, tc, mt = mr.designed(rng, 100, motion, wrong)
    got, flags = same(qc, tc, mt, model, 16, 96, 11)
    a11, a12, a21, a22, tx, ty = motion
    assert got[0] == 3 and got[1] == 100 and 100 - wrong <= got[2] <= 100 - wrong + 3
    assert got[4:12].tolist() == [65536 * a11, 65536 * a12, 65536 * tx, 65536 * a21, 65536 * a22, 65536 * ty, 0, 0]
    assert int((flags == 1).sum()) == got[2] and (flags >= 0).all()
    # the affine model finds the simpler motions too
    if model != mr.AFFINE:
        wide, _ = same(qc, tc, mt, mr.AFFINE, 16, 200, 11)
        assert wide[4:12].tolist() == got[4:12].tolist()


@pytest.mark.parametrize("m", [0, 1, 2, 3])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_fewer_correspondences_than_the_sample_give_no_model(m, model):
    c = np.array([(10 + 7 * i, 20 + 3 * i * i, 15 + 7 * i, 18 + 3 * i * i) for i in range(m)], np.int64).reshape(-1, 4)
    got, flags = same(*mr.from_correspondences(c), model, 16, 8, 1)
    assert got[1] == m and (got[0] & 1) == (m > model)
    if m <= model:
        assert got.tolist() == [0, m, 0, -1] + [0] * 8 + [-1, -1, -1, 0] and (flags == 0).all()


def test_coincident_query_points_make_every_hypothesis_invalid():
    c = np.array([(33, 44, 10 * i, 3 * i) for i in range(12)], np.int64)
    for model in (mr.SIMILARITY, mr.AFFINE):
        got, flags = same(*mr.from_correspondences(c), model, 4095, 64, 2)
        assert got.tolist() == [0, 12, 0, -1] + [0] * 8 + [-1, -1, -1, 0] and (flags == 0).all()
    got, _ = same(*mr.from_correspondences(c), mr.TRANSLATION, 0, 64, 2)
    assert got[0] == 3 and got[2] == 1 and got[15] == 1


def test_collinear_points_under_affine_and_the_refit_limit():
    """Collinear query points make every AFFINE sample invalid (D == 0): no model, so no refit either.  A valid AFFINE sample
    is itself three inliers that are not collinear, so det > 0 whenever there is a model: the rule's det <= 0 branch is reached
    only through mr.refit on a set of its own, never through a call.  What does clear the refit bit beside a set model bit is
    the magnitude limit: a scale above 256 (|a| > 2^24)."""
    line = np.array([(5 * i, 10 * i, 5 * i + 1, 10 * i) for i in range(12)], np.int64)
    got, flags = same(*mr.from_correspondences(line), mr.AFFINE, 8, 48, 1)
    assert got.tolist() == [0, 12, 0, -1] + [0] * 8 + [-1, -1, -1, 0] and (flags == 0).all()
    assert mr.refit(line, mr.AFFINE) == (False, [0] * 8), "det == 0: the refit bit is clear, words 4..11 are zero"
    # SIMILARITY on the same line is valid and exact: Dn > 0
    got, _ = same(*mr.from_correspondences(line), mr.SIMILARITY, 0, 16, 3)
    assert got[0] == 3 and got[2] == 12 and got[4:12].tolist() == [65536, 0, 65536, 0, 65536, 0, 0, 0]
    # one point off the line: every valid sample holds it, and the affine map through the sample carries the whole line
    bent = np.concatenate([line, np.array([(300, 7, 301, 7)], np.int64)])
    for seed in range(8):
        got, flags = same(*mr.from_correspondences(bent), mr.AFFINE, 0, 64, seed)
        assert got[0] == 3 and got[2] == 13 and 12 in got[12:15].tolist()
        assert got[4:12].tolist() == [65536, 0, 65536, 0, 65536, 0, 0, 0]
    # scale 65535: a model, no refit, words 4..11 zero; scale 256 is the last that is refitted
    for scale, refit in ((65535, False), (257, False), (256, True)):
        c = np.array([(x, y, scale * x, scale * y) for x, y in ((0, 0), (1, 0), (0, 1), (1, 1))], np.int64)
        for model in (mr.SIMILARITY, mr.AFFINE):
            got, flags = same(*mr.from_correspondences(c), model, 16, 16, 2)
            assert got[0] == (3 if refit else 1) and got[2] == 4 and (flags == 1).all()
            assert got[4:12].tolist() == ([65536 * scale, 0, 0, 0, 65536 * scale, 0, 0, 0] if refit else [0] * 8)


def tie_seed():
    for seed in range(1000):
        first = [mr.sample(h, seed, 10, 1)[0] for h in range(8)]
        groups = [0 if i < 4 else 1 if i < 8 else 2 for i in first]
        if groups[0] == 2 and 0 in groups and 1 in groups:
            return seed, next(h for h, g in enumerate(groups) if g != 2)
    raise AssertionError("no such seed")


def test_equal_counts_go_to_the_smaller_h():
    seed, h_first = tie_seed()
    got, flags = same(*mr.from_correspondences(mr.tie_set()), mr.TRANSLATION, 16, 8, seed)
    assert h_first > 0 and got[3] == h_first and got[2] == 4
    group = 0 if mr.sample(h_first, seed, 10, 1)[0] < 4 else 1
    assert flags.tolist() == ([1] * 4 + [0] * 6 if group == 0 else [0] * 4 + [1] * 4 + [0] * 2)


def threshold_seed(model):
    for seed in range(10000):
        idx = mr.sample(0, seed, 8, model + 1)
        if max(idx) < 6 and (model == 0 or abs(idx[0] - idx[1]) == 1):
            return seed
    raise AssertionError("no such seed")


@pytest.mark.parametrize("model", [mr.TRANSLATION, mr.SIMILARITY])
def test_the_threshold_is_inclusive(model):
    """thr_q4 = 48 is 3 px: off by (3, 0) is an inlier (on the equality), off by (3, 1) is not; under SIMILARITY with D = 25."""
    got, flags = same(*mr.from_correspondences(mr.threshold_set(model)), model, 48, 1, threshold_seed(model))
    assert flags.tolist() == [1] * 7 + [0] and got[2] == 7 and got[15] == (1 if model == 0 else 25)
    got, flags = same(*mr.from_correspondences(mr.threshold_set(model)), model, 47, 1, threshold_seed(model))
    assert flags.tolist() == [1] * 6 + [0, 0]


EXTREME = [(0, 0, 65535, 65535), (65535, 65535, 0, 0), (0, 65535, 65535, 0), (65535, 0, 0, 65535),
           (0, 0, 0, 65535), (65535, 65535, 65535, 0), (0, 65535, 0, 0), (65535, 0, 65535, 65535)]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_the_width_bounds_hold_at_4096_correspondences_with_extreme_coordinates(model):
    rng = np.random.default_rng(53 + model)
    c = np.zeros((4096, 4), np.int64)
    c[:, :2] = rng.integers(0, 65536, (4096, 2))
    c[:, 2:] = 65535 - c[:, :2]
    c[::2, 2:] = rng.integers(0, 65536, (2048, 2))
    c[:8] = EXTREME
    for thr in (4095, 16, 0):
        got, _ = same(*mr.from_correspondences(c), model, thr, 48, 5)
        assert got[1] == 4096 and got[0] & 1
        same(*mr.from_correspondences(c[:8]), model, thr, 256, 5)     # every sample an extreme one
    # points at the range's ends only, all inliers: the largest sums and covariances of the refit
    ends = np.array([(x, y, x, y) for x in (0, 65535) for y in (0, 65535)] * 1024, np.int64)
    got, _ = same(*mr.from_correspondences(ends), model, 4095, 8, 1)
    assert got[2] == 4096
    if got[0] == 3:
        assert got[4:12].tolist() == [65536, 0, 0, 0, 65536, 0, 0, 0]
    # the bounds of the header, from Python ints
    for idx in ([0, 1, 2], [2, 3, 0], [4, 5, 6]):
        D, *M = mr.hypothesis(c, idx, model)
        assert abs(D) <= 1 << 33 and max(abs(v) for v in M) <= 1 << 34


def test_slots_that_are_no_correspondence_are_skipped():
    rng = np.random.default_rng(9)
    qc, tc, mt = mr.designed(rng, 40, (1, 0, 0, 1, 4, 6), 10)
    c = np.concatenate([qc[:, :2], tc[mt[:, 0], :2]], 1)
    qg, tg, mg = mr.with_gaps(rng, c, 30)
    got, flags = same(qg, tg, mg, mr.TRANSLATION, 16, 32, 3)
    plain, plain_flags = same(qc, tc, mt, mr.TRANSLATION, 16, 32, 3)
    assert got[1] == 40 and (flags == -1).sum() == 30 and got[:12].tolist() == plain[:12].tolist()
    assert np.array_equal(flags[flags >= 0], plain_flags)
    # a train count below a match's index: the rule clamps nothing but the counts
    got2, flags2 = capi.estimate_motion(qg, tg[:35], mg, mr.TRANSLATION, 16, 32, 3)
    want2, wf2 = mr.estimate(qg, 70, tg[:35], 35, mg, mr.TRANSLATION, 16, 32, 3)
    assert got2.tolist() == want2.tolist() and np.array_equal(flags2, wf2) and got2[1] < 40


def test_refused_calls_write_nothing():
    L = capi.load()
    qc, tc, mt = mr.from_correspondences(np.array([(i, 2 * i, i + 1, 2 * i) for i in range(5)], np.int64))

    def call(q=qc, nq=5, t=tc, nt=5, m=mt, model=0, thr=16, hyp=8, out=1, inl=1):
        rec = np.full(16 + 8, SENT, np.uint64)
        fl = np.full(5 + 8, -7, np.int32)
        st = L.canny_hip_estimate_motion(capi._hp(q) if q is not None else None, nq, capi._hp(t) if t is not None else None,
                                         nt, capi._hp(m) if m is not None else None, model, thr, hyp, 1,
                                         capi._hp(rec) if out else None, capi._hp(fl) if inl else None)
        if st:
            assert (rec == SENT).all() and (fl == -7).all()
        else:
            assert (rec[16:] == SENT).all() and (fl[nq if inl else 0:] == -7).all()
        return st

    assert call() == 0 and call(inl=0) == 0 and call(nq=0, q=None, m=None) == 0 and call(nt=0, t=None) == 0
    for kw in (dict(q=None), dict(t=None), dict(m=None), dict(out=0), dict(nq=-1), dict(nt=-1), dict(model=-1), dict(model=3),
               dict(thr=-1), dict(thr=4096), dict(hyp=0), dict(hyp=-1)):
        assert call(**kw) == 1, kw
    for kw in (dict(nq=4097), dict(nt=4097), dict(hyp=4097)):
        assert call(**kw) == 2, kw
    raw = np.zeros(8 * 20, np.uint8)
    off = (8 - raw.ctypes.data % 8) % 8 + 4
    fl = np.full(5, -7, np.int32)
    st = L.canny_hip_estimate_motion(capi._hp(qc), 5, capi._hp(tc), 5, capi._hp(mt), 0, 16, 8, 1,
                                     capi.C.c_void_p(raw.ctypes.data + off), capi._hp(fl))
    assert st == 1 and not raw.any() and (fl == -7).all()


# ---- the scene of the descriptor tests -------------------------------------------------------------------------------------
def test_scene_views_a_and_b_recover_the_shift():
    """A -> B, TRANSLATION, thr_q4 = 96 (6 px), 64 hypotheses.  The descriptor tests assert at least 38 right matches within
    +-2 px of (-7, -4) and at most 2 wrong ones; any right match as the hypothesis has every right match within sqrt(32) < 6
    px, so inliers >= n_right, and the refit shift lies within (38 * 2 + 2 * 8) / 40 < 2.5 px of (-7, -4) per component."""
    (A, ca), (B, cb) = scene()["A"], scene()["B"]
    for steered in (False, True):
        da, _ = capi.corner_descriptors_from_plane(A, ca, steered)
        db, _ = capi.corner_descriptors_from_plane(B, cb, steered)
        mt, n_acc = capi.match_descriptors(da, db, 64, 205, capi.MATCH_CROSS_CHECK)
        n_right = sum(1 for i, (j, _, _, f) in enumerate(mt.tolist())
                      if f & 8 and abs(int(cb[j, 0]) - int(ca[i, 0]) + 7) <= 2 and abs(int(cb[j, 1]) - int(ca[i, 1]) + 4) <= 2)
        got, flags = same(ca, cb, mt, mr.TRANSLATION, 96, 64, 0)
        tx, ty = got[6] / 65536, got[9] / 65536
        print(f"A/B steered={steered}: accepted {n_acc}, right {n_right}, inliers {got[2]}, shift ({tx:.3f}, {ty:.3f})")
        assert got[0] == 3 and got[1] == n_acc and got[2] >= n_right >= 38
        assert abs(tx + 7) <= 2.5 and abs(ty + 4) <= 2.5


THR_TURN = 48   # 3 px


def test_scene_turned_view_recovers_the_quarter_turn():
    """A -> R, SIMILARITY, the steered descriptors: the refit model takes the four frame corners no further from where the true
    turn (x, y) -> (y, 319 - x) takes them than the inlier threshold used.  Measured: 46 accepted matches, 46 inliers, and
    0.000 px -- the turned view's corners sit exactly on the turned positions, so the refit is the turn itself (README)."""
    (A, ca), (R, cr_) = scene()["A"], scene()["R"]
    da, _ = capi.corner_descriptors_from_plane(A, ca, True)
    db, _ = capi.corner_descriptors_from_plane(R, cr_, True)
    mt, n_acc = capi.match_descriptors(da, db, 64, 205, capi.MATCH_CROSS_CHECK)
    want, want_flags = mr.estimate(ca, len(ca), cr_, len(cr_), mt, mr.SIMILARITY, THR_TURN, 64, 0)
    worst = 0.0
    for x, y in ((0, 0), (319, 0), (0, 239), (319, 239)):
        u, v = mr.apply_q16(want, x, y)
        worst = max(worst, float(np.hypot(u - y, v - (319 - x))))
    print(f"A/R: accepted {n_acc}, inliers {want[2]}, frame corners off by at most {worst:.3f} px")
    got, flags = capi.estimate_motion(ca, cr_, mt, mr.SIMILARITY, THR_TURN, 64, 0)
    assert got.tobytes() == want.tobytes() and flags.tobytes() == want_flags.tobytes()
    assert want[0] == 3 and worst < THR_TURN / 16


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2100
    assert capi.load().canny_hip_version() >= 2100
    for word in ("CANNY_HIP_MOTION_WORDS 16", "CANNY_HIP_MOTION_MAX_HYPOTHESES 4096", "CANNY_HIP_MOTION_TRANSLATION = 0",
                 "CANNY_HIP_MOTION_SIMILARITY = 1", "CANNY_HIP_MOTION_AFFINE = 2", "0x9E3779B9", "1664525", "1013904223",
                 "CANNY_HIP_MOTION_PART_GATHER", "CANNY_HIP_MOTION_PART_SCORE", "CANNY_HIP_MOTION_PART_REFIT", "homography",
                 "0.21.0"):
        assert word in header, word
    for name in ("canny_hip_dev_estimate_motion", "canny_hip_estimate_motion", "canny_hip_canny_motion",
                 "canny_hip_motion_profile_get", "canny_hip_selftest_motion_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert capi.MOTION_DTYPE.itemsize == 8 * capi.MOTION_WORDS == 8 * mr.WORDS
    assert (capi.MOTION_TRANSLATION, capi.MOTION_SIMILARITY, capi.MOTION_AFFINE) == (mr.TRANSLATION, mr.SIMILARITY, mr.AFFINE)
    assert capi.MOTION_MAX_HYPOTHESES == mr.MAX_HYPOTHESES


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_motion_host.cpp has its own main and is compiled together with csrc/canny_motion_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_motion_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_motion_host.cpp"),
                           os.path.join(csrc, "canny_motion_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "motion ok" in r.stdout, r.stdout + r.stderr
