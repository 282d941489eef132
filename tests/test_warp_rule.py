"""CPU-only checks of the frame-alignment rules (include/canny_hip.h): canny_hip_compose_motion and
canny_hip_warp_frames (plain C++) against tests/warp_rule.py byte for byte, known answers that do not come from the rule
(np.rot90, slices, np.fliplr), the limits, every refused call, the scene of tests/test_descriptors_rule.py, and the host rules
under the host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_rule as mr
import warp_rule as wr
from canny_edge_amd import capi
from test_descriptors_rule import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = wr.ONE
BOTH = (wr.NEAREST, wr.BILINEAR)


def plane(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def same(src, xforms, out_h, out_w, interp, border):
    """The host C++ against the rule; returns (frames, valid as bool)."""
    src = np.asarray(src, np.uint8)
    src = src[None] if src.ndim == 2 else src
    xforms = np.asarray(xforms, np.int64).reshape(-1, 8)
    got, bits = capi.warp_frames(src, xforms, out_h, out_w, interp, border)
    want, want_bits = wr.warp(src, xforms, out_h, out_w, interp, border)
    assert np.array_equal(got, want), (interp, border, xforms.tolist())
    assert np.array_equal(bits, want_bits), ("valid bits", interp, border, xforms.tolist())
    return got, wr.unpack_valid(bits, out_w)


def same_chain(motion, first_frame=0):
    got = capi.compose_motion(motion, first_frame)
    want = wr.compose(motion, first_frame)
    assert got.view(np.int64).reshape(-1, 8).tolist() == want.tolist()
    return want


# ---- known answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", BOTH)
def test_the_identity_returns_the_input_and_all_valid_bits(interp):
    P = plane(37, 53, 1)
    out, valid = same(P, wr.record(wr.IDENTITY), 37, 53, interp, 9)
    assert np.array_equal(out[0], P) and valid.all()


@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("dx,dy", [(5, 3), (-4, 7), (0, -6), (60, 0), (0, 40)])
def test_an_integer_shift_is_a_slice_plus_border(interp, dx, dy):
    P = plane(37, 53, 2)
    out, valid = same(P, wr.record(wr.shift(dx, dy)), 37, 53, interp, 200)
    want, inside = np.full((37, 53), 200, np.uint8), np.zeros((37, 53), bool)
    ys, xs = np.arange(37), np.arange(53)
    oy, ox = ys[(ys + dy >= 0) & (ys + dy < 37)], xs[(xs + dx >= 0) & (xs + dx < 53)]
    if len(oy) and len(ox):
        want[oy[0]:oy[-1] + 1, ox[0]:ox[-1] + 1] = P[oy[0] + dy:oy[-1] + dy + 1, ox[0] + dx:ox[-1] + dx + 1]
        inside[oy[0]:oy[-1] + 1, ox[0]:ox[-1] + 1] = True
    assert np.array_equal(out[0], want) and np.array_equal(valid[0], inside)


@pytest.mark.parametrize("interp", BOTH)
def test_the_quarter_turn_is_rot90(interp):
    """R = np.rot90(P) holds P's pixel (x, y) at (y, W - 1 - x), the relation of tests/test_descriptors_rule.py's turned view:
    warping R by that map to P's geometry gives P back."""
    P = plane(41, 67, 3)
    R = np.ascontiguousarray(np.rot90(P))
    out, valid = same(R, wr.record(wr.quarter_turn(67)), 41, 67, interp, 0)
    assert np.array_equal(out[0], P) and valid.all()


@pytest.mark.parametrize("interp", BOTH)
def test_a_mirror_is_fliplr(interp):
    P = plane(20, 70, 4)
    out, valid = same(P, wr.record((-ONE, 0, 69 * ONE, 0, ONE, 0)), 20, 70, interp, 0)
    assert np.array_equal(out[0], np.fliplr(P)) and valid.all()


@pytest.mark.parametrize("interp", BOTH)
def test_scale_two_takes_every_second_pixel(interp):
    P = plane(40, 66, 5)
    out, valid = same(P, wr.record((2 * ONE, 0, 0, 0, 2 * ONE, 0)), 20, 33, interp, 0)
    assert np.array_equal(out[0], P[::2, ::2]) and valid.all()


def test_half_a_pixel_bilinear_is_the_rounded_mean_of_two_neighbours():
    P = plane(12, 40, 6)
    out, valid = same(P, wr.record((ONE, 0, 32768, 0, ONE, 0)), 12, 39, wr.BILINEAR, 0)
    p = P.astype(int)
    assert np.array_equal(out[0], (p[:, :-1] + p[:, 1:] + 1) >> 1) and valid.all()


def test_four_composed_quarter_turns_are_the_identity_and_shifts_add():
    q = wr.quarter_turn(50)
    chain = same_chain([wr.motion_record(q)] * 4, 3)
    assert chain[:, 0].tolist() == [1] * 5 and chain[:, 1].tolist() == [3, 4, 5, 6, 7]
    assert tuple(chain[4, 2:]) == wr.IDENTITY and tuple(chain[2, 2:]) == (-ONE, 0, 49 * ONE, 0, -ONE, 49 * ONE)
    shifts = [(3, -2), (0.5, 0.25), (-7.125, 4)]
    chain = same_chain([wr.motion_record(wr.shift(*s)) for s in shifts])
    assert tuple(chain[3, 2:]) == wr.shift(3 + 0.5 - 7.125, -2 + 0.25 + 4)
    assert same_chain(np.zeros((0, 16), np.int64), 5).tolist() == [[1, 5, ONE, 0, 0, 0, ONE, 0]]


# ---- the rule's corners -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("tx", [-1, -129, -32768, -32769, 127, 128])
def test_negative_positions_are_floored(interp, tx):
    """tx = -1: 1/65536 px left of the grid.  NEAREST rounds it back onto the pixel; BILINEAR: X8 = (X + 128) >> 8 is x * 256 for
    tx = -1 (the input, all valid) and x * 256 - 1 for tx = -129: ix = x - 1, fx = 255, so column 0 mixes the border in and is
    not valid."""
    P = plane(9, 21, 7)
    out, valid = same(P, wr.record((ONE, 0, tx, 0, ONE, tx)), 9, 21, interp, 77)
    if tx in (-1, 127) or (interp == wr.NEAREST and tx in (-129, 128, -32768)):
        assert np.array_equal(out[0], P) and valid.all()
    elif interp == wr.BILINEAR and tx == -129:
        assert not valid[0, 0].any() and not valid[0, :, 0].any() and valid[0, 1:, 1:].all()
        assert out[0, 0, 0] == (77 + 255 * 77 + 255 * 77 + 255 * 255 * int(P[0, 0]) + 32768) >> 16
    elif interp == wr.NEAREST and tx == -32769:
        assert np.array_equal(out[0, 1:, 1:], P[:-1, :-1]) and (out[0, 0] == 77).all() and not valid[0, 0].any()


LEAVING = {"left": wr.shift(-30.25, 2.5), "right": wr.shift(30.75, -1.5), "top": wr.shift(3.5, -25.25),
           "bottom": wr.shift(-2.25, 22.5), "outside to the left": wr.shift(-200, 0), "outside below": wr.shift(0, 90),
           "outside, turned": (0, ONE, 500 * ONE, -ONE, 0, -3 * ONE), "one column inside": wr.shift(-63, 0.5)}


@pytest.mark.parametrize("interp", BOTH)
@pytest.mark.parametrize("name", sorted(LEAVING))
def test_footprints_that_leave_the_source(interp, name):
    P = plane(40, 64, 8)
    out, valid = same(P, wr.record(LEAVING[name]), 40, 64, interp, 13)
    if name.startswith("outside"):
        assert (out == 13).all() and not valid.any()
    else:
        assert valid.any() and not valid.all()


@pytest.mark.parametrize("interp", BOTH)
def test_the_magnitude_limits(interp):
    """|a| = 2^24 and |t| = 2^36 are usable; one past either is not: the frame is the border and no bit is valid."""
    P = plane(30, 30, 9)
    A, T = wr.LIM_A, wr.LIM_T
    for coef in ((A, 0, 0, 0, A, 0), (-A, A, 0, A, -A, 0), (ONE, 0, T, 0, ONE, 0), (ONE, 0, -T, 0, ONE, T),
                 (A, A, -T, -A, -A, T)):
        out, valid = same(P, wr.record(coef), 8, 70, interp, 5)
        assert out[0, 0, 0] == (P[0, 0] if coef[2] == 0 else 5) and bool(valid[0, 0, 0]) == (coef[2] == 0)
    for i in range(6):
        for sign in (1, -1):
            coef = list(wr.IDENTITY)
            coef[i] = sign * ((T if i in (2, 5) else A) + 1)
            out, valid = same(P, wr.record(coef), 8, 70, interp, 5)
            assert (out == 5).all() and not valid.any()
    # the widest X: |a| = 2^24 at x = y = 32767 with |t| = 2^36 stays under 2^41
    assert 2 * A * 32767 + T < 1 << 41
    small = np.full((1, 1, 1), 200, np.uint8)
    out, valid = same(small, wr.record((-A, -A, T, A, A, -T)), 1, 32768, interp, 1)
    assert out.shape == (1, 1, 32768)


@pytest.mark.parametrize("interp", BOTH)
def test_records_select_their_source_and_unusable_ones_give_the_border(interp):
    src = np.stack([plane(16, 24, s) for s in (10, 11, 12)])
    recs = [wr.record(wr.IDENTITY, 2), wr.record(wr.shift(1, 1), 0), wr.record(wr.IDENTITY, 3), wr.record(wr.IDENTITY, -1),
            wr.record(wr.IDENTITY, 1, flags=0), wr.record(wr.IDENTITY, 1, flags=2), wr.record(wr.IDENTITY, 1, flags=3),
            wr.record(wr.IDENTITY, 2)]
    out, valid = same(src, np.stack(recs), 16, 24, interp, 99)
    assert np.array_equal(out[0], src[2]) and np.array_equal(out[7], src[2]) and np.array_equal(out[6], src[1])
    for o in (2, 3, 4, 5):
        assert (out[o] == 99).all() and not valid[o].any()


def test_a_chain_broken_by_a_missing_refit_bit_or_by_the_limit_stays_broken():
    good = wr.motion_record(wr.shift(2, 1))
    for bad in (wr.motion_record(wr.shift(1, 1), flags=1), wr.motion_record(wr.shift(1, 1), flags=2),
                wr.motion_record(wr.shift(1, 1), flags=0), wr.motion_record((wr.LIM_A + 1, 0, 0, 0, ONE, 0)),
                wr.motion_record((ONE, 0, 0, 0, ONE, -wr.LIM_T - 1))):
        chain = same_chain([good, good, bad, good, good], 2)
        assert chain[:, 0].tolist() == [1, 1, 1, 0, 0, 0] and chain[:, 1].tolist() == [2, 3, 4, 5, 6, 7]
        assert not chain[3:, 2:].any() and tuple(chain[2, 2:]) == wr.shift(4, 2)
    # every record within the limits, the composed one past them: scale 256 twice, and a translation that grows past 2^36
    big = wr.motion_record((wr.LIM_A, 0, 0, 0, wr.LIM_A, 0))
    chain = same_chain([big, big, good])
    assert chain[:, 0].tolist() == [1, 1, 0, 0] and tuple(chain[1, 2:]) == (wr.LIM_A, 0, 0, 0, wr.LIM_A, 0)
    far = wr.motion_record((ONE, 0, wr.LIM_T, 0, ONE, 0))
    chain = same_chain([far, wr.motion_record(wr.shift(0, 0)), wr.motion_record((ONE, 0, 1, 0, ONE, 0)), good])
    assert chain[:, 0].tolist() == [1, 1, 1, 0, 0] and chain[2, 4] == wr.LIM_T
    # the widths of the header, from Python ints: the largest products of a step
    assert 2 * wr.LIM_A * wr.LIM_A < 1 << 50 and 2 * wr.LIM_A * wr.LIM_T < 1 << 62
    ext = wr.motion_record((-wr.LIM_A, wr.LIM_A, wr.LIM_T, wr.LIM_A, -wr.LIM_A, -wr.LIM_T))
    same_chain([ext, ext, ext])
    tilt = wr.motion_record((65000, -9000, -wr.LIM_T, 9000, 65000, wr.LIM_T))
    same_chain([tilt] * 40)


def test_random_chains_and_random_warps_follow_the_rule():
    rng = np.random.default_rng(20)
    for n in (1, 2, 7, 70):
        motion = np.zeros((n, 16), np.int64)
        motion[:, 0] = np.where(rng.random(n) < 0.97, 3, rng.integers(0, 4, n))
        motion[:, 4:10] = rng.integers(-70000, 70000, (n, 6))
        motion[:, [6, 9]] = rng.integers(-(1 << 30), 1 << 30, (n, 2))
        same_chain(motion, int(rng.integers(0, 100)))
    src = np.stack([plane(33, 47, s) for s in (21, 22)])
    for interp in BOTH:
        recs = []
        for k in range(8):
            lin = rng.integers(-2 * ONE, 2 * ONE, 4)
            recs.append(wr.record(wr.about_centre(*(int(v) for v in lin), 23 + rng.random() * 4, 16 + rng.random() * 4), k % 2))
        recs.append(wr.record(wr.small_turn(47, 33), 1))
        same(src, np.stack(recs), 29, 71, interp, 31)


def test_refused_calls_leave_the_sentinels_untouched():
    L = capi.load()
    src = np.stack([plane(10, 12, 30)] * 2)
    motion = np.stack([wr.motion_record(wr.shift(1, 0))] * 3)

    def warp(src_=src, n_src=2, sh=10, sw=12, xf=1, n_out=2, oh=6, ow=9, interp=1, border=0, out=1, valid=1, off=0):
        x = np.zeros(2 * 8 + 1, np.int64)
        x[:16] = np.stack([wr.record(wr.IDENTITY, 1)] * 2).ravel()
        o, v = np.full(2 * 6 * 9 + 8, 0x5A, np.uint8), np.full(2 * 6 * 2 + 8, 0x5A, np.uint8)
        st = L.canny_hip_warp_frames(capi._hp(src_) if src_ is not None else None, n_src, sh, sw,
                                     capi.C.c_void_p(x.ctypes.data + off) if xf else None, n_out, oh, ow, interp, border,
                                     capi._hp(o) if out else None, capi._hp(v) if valid else None)
        if st:
            assert (o == 0x5A).all() and (v == 0x5A).all(), "a refused call wrote something"
        else:
            assert (o[108:] == 0x5A).all() and (v[24:] == 0x5A).all() and (not valid or (v[:24] != 0x5A).all())
        return st

    assert warp() == 0 and warp(valid=0) == 0 and warp(border=255) == 0 and warp(interp=0) == 0
    for kw in (dict(src_=None), dict(xf=0), dict(out=0), dict(n_src=0), dict(n_out=0), dict(sh=0), dict(sw=0), dict(oh=0),
               dict(ow=0), dict(n_src=-1), dict(oh=-3), dict(interp=2), dict(interp=-1), dict(border=-1), dict(border=256),
               dict(off=4)):
        assert warp(**kw) == 1, kw
    for kw in (dict(sh=32769), dict(sw=32769), dict(oh=32769), dict(ow=32769), dict(n_src=65536), dict(n_out=65536),
               dict(sh=32768, sw=32768 * 2), dict(oh=32768 * 2, ow=32768)):
        assert warp(**kw) == 2, kw
    # planes of 2^31 pixels within the dimension limit do not exist (32768^2 = 2^30): the plane limit is the dimensions'
    buf = np.full(400, 0x5A, np.uint8)
    x = np.stack([wr.record(wr.IDENTITY)])
    for so, oo in ((0, 0), (0, 119), (100, 0), (0, 100)):     # the source is 10 x 12 = 120 bytes, the output 10 x 12 too
        st = L.canny_hip_warp_frames(capi.C.c_void_p(buf.ctypes.data + so), 1, 10, 12, capi._hp(x), 1, 10, 12, 0, 0,
                                     capi.C.c_void_p(buf.ctypes.data + oo), None)
        assert st == 1 and (buf == 0x5A).all(), (so, oo)
    st = L.canny_hip_warp_frames(capi.C.c_void_p(buf.ctypes.data), 1, 10, 12, capi._hp(x), 1, 10, 12, 0, 0,
                                 capi.C.c_void_p(buf.ctypes.data + 120), None)
    assert st == 0 and (buf[240:] == 0x5A).all() and np.array_equal(buf[:120], buf[120:240])

    def chain(m=motion, n=3, first=0, out=1, off=0):
        x = np.full(4 * 8 + 9, 0x5A5A5A5A5A5A5A5A, np.int64)
        st = L.canny_hip_compose_motion(capi._hp(m) if m is not None else None, n, first,
                                        capi.C.c_void_p(x.ctypes.data + off) if out else None)
        if st:
            assert (x == 0x5A5A5A5A5A5A5A5A).all(), "a refused call wrote something"
        else:
            assert (x[8 * (n + 1):] == 0x5A5A5A5A5A5A5A5A).all()
        return st

    assert chain() == 0 and chain(n=0) == 0 and chain(m=None, n=0) == 0 and chain(first=7) == 0
    for kw in (dict(m=None), dict(out=0), dict(n=-1), dict(first=-1), dict(off=4)):
        assert chain(**kw) == 1, kw
    assert chain(n=65536) == 2


# ---- the scene of the descriptor tests -------------------------------------------------------------------------------------
def mad(a, b, valid):
    return float(np.abs(a.astype(int) - b.astype(int))[valid].mean())


def estimate(ca, P_b, cb, model, thr_q4, steered):
    da, _ = capi.corner_descriptors_from_plane(scene()["A"][0], ca, steered)
    db, _ = capi.corner_descriptors_from_plane(P_b, cb, steered)
    mt, _ = capi.match_descriptors(da, db, 64, 205, capi.MATCH_CROSS_CHECK)
    got, _ = capi.estimate_motion(ca, cb, mt, model, thr_q4, 64, 0)
    return got


def test_scene_views_are_aligned_by_the_estimated_motion():
    """The scene of tests/test_descriptors_rule.py.  B is A's scene shifted by (-7, -4) with noise: the estimated shift (as in
    tests/test_motion_rule.py: TRANSLATION, 6 px, 64 hypotheses), chained and applied with BILINEAR, must align B onto A about
    as well as the true integer shift does, and far better than no alignment.  R is the noisy scene turned by a quarter: the
    SIMILARITY estimate turns it back, NEAREST and BILINEAR alike.
    Measured (mean absolute difference in grey levels over the valid pixels): unaligned 11.36; estimated shift
    (-6.977, -3.977) 0.603 over 96.2 %; true shift 0.582 over 96.2 %; R by its estimated model 0.576 over 100 %."""
    (A, ca), (B, cb), (R, cr_) = scene()["A"], scene()["B"], scene()["R"]
    h, w = A.shape
    motion = estimate(ca, B, cb, mr.TRANSLATION, 96, False)
    chain = same_chain([motion])
    assert chain[1, 0] == 1 and chain[1, 1] == 1
    out, valid = same(np.stack([A, B]), chain, h, w, wr.BILINEAR, 0)
    assert np.array_equal(out[0], A) and valid[0].all()
    true, true_valid = same(B, wr.record(wr.shift(-7, -4)), h, w, wr.BILINEAR, 0)
    e_est, e_true, e_none = mad(out[1], A, valid[1]), mad(true[0], A, true_valid[0]), mad(B, A, valid[1])
    print(f"A/B: shift ({chain[1, 4] / ONE:.3f}, {chain[1, 7] / ONE:.3f}), aligned {e_est:.3f} over {valid[1].mean():.1%}, "
          f"true shift {e_true:.3f} over {true_valid[0].mean():.1%}, unaligned {e_none:.3f}")
    assert e_est <= 2 * e_true and e_est < e_none / 4 and valid[1].mean() > 0.9

    motion = estimate(ca, R, cr_, mr.SIMILARITY, 48, True)
    chain = same_chain([motion])
    rec = chain[1].copy()
    rec[1] = 0                                        # R is the only source plane of this call (its geometry differs from A's)
    near, near_valid = same(R, rec, h, w, wr.NEAREST, 0)
    bil, bil_valid = same(R, rec, h, w, wr.BILINEAR, 0)
    e_turn = mad(bil[0], A, bil_valid[0])
    print(f"A/R: model {chain[1, 2:].tolist()}, aligned {e_turn:.3f} over {bil_valid[0].mean():.1%}")
    assert np.array_equal(near, bil) and np.array_equal(near_valid, bil_valid)
    assert e_turn <= 2 * e_true and e_turn < e_none / 4 and bil_valid[0].mean() > 0.9


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2200
    assert capi.load().canny_hip_version() >= 2200
    for word in ("CANNY_HIP_XFORM_WORDS 8", "CANNY_HIP_WARP_NEAREST = 0", "CANNY_HIP_WARP_BILINEAR = 1", "0.22.0", "2^50",
                 "2^62", "2^41", "CANNY_HIP_WARP_PART_COMPOSE", "CANNY_HIP_WARP_PART_WARP", "\"warp_route\"", "bicubic",
                 "inverting a model", "CANNY_HIP_WARP_LDS_BYTES %d" % capi.WARP_LDS_BYTES):
        assert word in header, word
    for name in ("canny_hip_dev_compose_motion", "canny_hip_compose_motion", "canny_hip_dev_warp_frames",
                 "canny_hip_warp_frames", "canny_hip_canny_align", "canny_hip_warp_profile_get",
                 "canny_hip_selftest_warp_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for method in ("dev_compose_motion", "dev_warp_frames", "canny_align", "warp_profile_get"):
        assert hasattr(capi.Context, method), method
    assert capi.XFORM_DTYPE.itemsize == 8 * capi.XFORM_WORDS == 8 * wr.XFORM_WORDS
    assert (capi.WARP_NEAREST, capi.WARP_BILINEAR) == (wr.NEAREST, wr.BILINEAR)


# ---- the host rules under the host compiler's sanitizers ----------------------------------------------------------------
def test_host_rules_run_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_warp_host.cpp has its own main and is compiled together with csrc/canny_warp_host.cpp alone: nothing of
    it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_warp_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_warp_host.cpp"),
                           os.path.join(csrc, "canny_warp_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "warp ok" in r.stdout, r.stdout + r.stderr
