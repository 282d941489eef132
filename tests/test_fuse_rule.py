"""CPU-only checks of the temporal-fusion rule (include/canny_hip.h): canny_hip_fuse_frames and
canny_hip_change_mask (plain C++) against tests/fuse_rule.py byte for byte, known answers that do not come from the rule
(np.median, np.ma.median / min / max, the float64 mean), the moving object, every refused call, and the host rules under the
host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_rule as fr
from canny_edge_amd import capi
from fuse_rule import GROUP_LENS, HEIGHTS, VALID, VALUES, WIDTHS, moving_object, valid_bits, values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(frames, bits, group_len, step, op, fill=0, min_count=1):
    """The host C++ against the rule; returns (fused, count)."""
    got = capi.fuse_frames(frames, bits, group_len, step, op, fill, min_count)
    want = fr.fuse(frames, bits, group_len, step, op, fill, min_count)
    assert np.array_equal(got[0], want[0]), ("fused", frames.shape, group_len, step, op, fill, min_count)
    assert np.array_equal(got[1], want[1]), ("count", frames.shape, group_len, step, op, fill, min_count)
    return got


def same_mask(frames, bits, bg, bc, per, thr, min_count=1):
    got = capi.change_mask(frames, bg, bits, bc, per, thr, min_count)
    want = fr.change_mask(frames, bits, bg, bc, per, thr, min_count)
    assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist(), (frames.shape, per, thr, min_count)
    return got


# ---- the host C++ against the rule, over the shapes and patterns of the GPU tests -----------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_host_follows_the_rule_on_every_shape(w):
    for i, h in enumerate(HEIGHTS):
        for j, group_len in enumerate((1, 2, 3, 8, 9)):
            k = WIDTHS.index(w) + 5 * i + j
            step = (1, 2, group_len)[k % 3]
            n = group_len + 2 * step + (step > 1)
            frames = values(VALUES[k % len(VALUES)], n, h, w, k)
            bits = valid_bits(VALID[(k // 2) % len(VALID)], n, h, w, k)
            for op in fr.OPS:
                same(frames, bits, group_len, step, op, (0, 77)[k % 2], (1, 2, group_len)[(k // 3) % 3])
            bg, bc = fr.fuse(frames, bits, n, n, fr.MEDIAN, 0, 1)
            for thr in (0, 1, 49, 254, 255):
                same_mask(frames, bits, bg, bc if k % 2 else None, n, thr, (1, 2)[k % 2])


@pytest.mark.parametrize("kind", VALID)
def test_host_follows_the_rule_on_every_group_len_and_pattern(kind):
    for i, group_len in enumerate(GROUP_LENS):
        h, w = ((33, 67), (17, 257))[i % 2] if group_len < 64 else (3, 67)
        frames = values(VALUES[i % len(VALUES)], group_len + 1, h, w, i)
        bits = valid_bits(kind, group_len + 1, h, w, i)
        for op in fr.OPS:
            same(frames, bits, group_len, 1, op, 77, (1, 2, group_len)[i % 3])
    frames = values("random", 7, 9, 21, 5)
    bits = valid_bits(kind, 7, 9, 21, 5)
    for per in (1, 3, 7, 100):
        bg = values("random", -(-7 // per), 9, 21, 6)
        bc = values("ties", -(-7 // per), 9, 21, 7)
        for thr in (0, 1, 49, 254, 255):
            same_mask(frames, bits, bg, bc, per, thr, 8)
            same_mask(frames, bits, bg, None, per, thr, 255)


def test_the_vector_rule_and_the_python_int_rule_agree():
    frames, bits = values("random", 9, 4, 11, 1), valid_bits("half", 9, 4, 11, 1)
    valid = fr.unpack_bits(bits, 11)
    for op in fr.OPS:
        fused, count = fr.fuse(frames, bits, 9, 1, op, 200, 3)
        for y in range(4):
            for x in range(11):
                v = [int(frames[f, y, x]) for f in range(9) if valid[f, y, x]]
                assert (int(fused[0, y, x]), int(count[0, y, x])) == fr.fuse_pixel(v, op, 200, 3)


# ---- known answers that do not come from the rule ------------------------------------------------------------------------
@pytest.mark.parametrize("group_len", [1, 3, 5, 9, 33, 255])
def test_the_median_of_an_odd_all_valid_window_is_numpy_median(group_len):
    frames = values("random", group_len, 6, 13, group_len)
    fused, count = same(frames, None, group_len, group_len, fr.MEDIAN)
    assert np.array_equal(fused[0], np.median(frames, 0).astype(np.uint8)) and (count == group_len).all()


def masked(frames, bits):
    return np.ma.masked_array(frames.astype(np.int64), mask=~fr.unpack_bits(bits, frames.shape[2]))


def test_the_median_under_a_random_mask_is_ma_median_where_the_count_is_odd():
    frames, bits = values("random", 11, 9, 21, 2), valid_bits("half", 11, 9, 21, 2)
    fused, count = same(frames, bits, 11, 11, fr.MEDIAN)
    odd = count[0] % 2 == 1
    assert odd.sum() > 30 and np.array_equal(fused[0][odd], np.ma.median(masked(frames, bits), 0).filled(0)[odd].astype(np.uint8))


def test_the_mean_is_the_float_mean_rounded_half_up():
    """floor(mean + 0.5) in float64 agrees with (2 s + c) // (2 c) on every pair (s, c) of the domain (checked below), so the
    comparison is safe."""
    for c in (1, 2, 3, 7, 64, 254, 255):
        s = np.arange(255 * c + 1, dtype=np.int64)
        assert np.array_equal(np.floor(s / c + 0.5).astype(np.int64), (2 * s + c) // (2 * c))
    frames, bits = values("random", 10, 9, 21, 3), valid_bits("half", 10, 9, 21, 3)
    fused, count = same(frames, None, 10, 10, fr.MEAN)
    assert np.array_equal(fused[0], np.floor(frames.astype(np.float64).mean(0) + 0.5).astype(np.uint8))
    fused, count = same(frames, bits, 10, 10, fr.MEAN)
    some = count[0] > 0
    assert np.array_equal(fused[0][some], np.floor(masked(frames, bits).mean(0).filled(0)[some] + 0.5).astype(np.uint8))


def test_min_and_max_are_ma_min_and_ma_max_and_empty_pixels_are_fill():
    frames, bits = values("random", 6, 9, 21, 4), valid_bits("sparse", 6, 9, 21, 4)
    m = masked(frames, bits)
    for op, ref in ((fr.MIN, m.min(0)), (fr.MAX, m.max(0))):
        fused, count = same(frames, bits, 6, 6, op, 77)
        some = count[0] > 0
        assert (~some).sum() > 20 and np.array_equal(fused[0][some], ref.filled(0)[some].astype(np.uint8))
        assert (fused[0][~some] == 77).all()
    for op in fr.OPS:
        fused, count = same(frames, valid_bits("zeros", 6, 9, 21, 4), 6, 6, op, 123)
        assert (fused == 123).all() and (count == 0).all()
        fused, count = same(frames, bits, 6, 6, op, 9, 2)                    # the true count where fill was written
        assert (fused[0][count[0] < 2] == 9).all() and (count[0] == fr.unpack_bits(bits, 21).sum(0)).all()


def test_a_permuted_stack_gives_the_same_bytes_and_a_window_of_one_returns_the_frame():
    frames, bits = values("random", 8, 9, 21, 5), valid_bits("half", 8, 9, 21, 5)
    order = np.random.default_rng(5).permutation(8)
    for op in fr.OPS:
        a, b = same(frames, bits, 8, 8, op, 1, 2), same(frames[order], bits[order], 8, 8, op, 1, 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        fused, count = same(frames, bits, 1, 1, op, 55)
        valid = fr.unpack_bits(bits, 21)
        assert np.array_equal(fused[valid], frames[valid]) and (fused[~valid] == 55).all() and np.array_equal(count, valid)


def test_input_pad_bits_change_nothing():
    frames = values("random", 5, 9, 21, 6)
    clean = valid_bits("half", 5, 9, 21, 6)
    dirty = clean.copy()
    dirty[..., -1] |= 0x07
    bg = frames[:1]
    for op in fr.OPS:
        a, b = same(frames, clean, 5, 5, op), same(frames, dirty, 5, 5, op)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = same_mask(frames, clean, bg, None, 5, 10), same_mask(frames, dirty, bg, None, 5, 10)
    assert np.array_equal(a[0], b[0]) and not (a[0][..., -1] & 0x07).any()


def test_the_moving_object():
    bg, frames, patch = moving_object()
    fused, count = same(frames, None, 3, 3, fr.MEDIAN)
    assert np.array_equal(fused[0], bg) and (count == 3).all()
    mask, changed = same_mask(frames, None, fused, count, 3, 49, 3)
    assert np.array_equal(fr.unpack_bits(mask, 70), patch) and changed.tolist() == [54, 54, 54]
    mask, changed = same_mask(frames, None, fused, count, 3, 50, 3)
    assert not mask.any() and changed.tolist() == [0, 0, 0]


# ---- refused calls ------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_sentinels_untouched():
    L = capi.load()
    n, h, w = 4, 6, 9
    frames, bits = values("random", n, h, w, 7), valid_bits("half", n, h, w, 7)
    vp = capi.C.c_void_p

    def fuse(fr_=1, valid=1, n=n, h=h, w=w, gl=2, step=2, op=1, fill=0, mc=1, fused=1, count=1):
        o, c = np.full(2 * 6 * 9 + 8, 0x5A, np.uint8), np.full(2 * 6 * 9 + 8, 0x5A, np.uint8)
        st = L.canny_hip_fuse_frames(capi._hp(frames) if fr_ else None, capi._hp(bits) if valid else None, n, h, w, gl, step, op,
                                     fill, mc, capi._hp(o) if fused else None, capi._hp(c) if count else None)
        if st:
            assert (o == 0x5A).all() and (c == 0x5A).all(), "a refused call wrote something"
        else:
            g = fr.n_groups(n, gl, step) * h * w
            assert (o[g:] == 0x5A).all() and (c[g:] == 0x5A).all() and (count or (c == 0x5A).all())
        return st

    assert fuse() == 0 and fuse(valid=0) == 0 and fuse(count=0) == 0 and fuse(gl=4, step=9, fill=255, mc=255) == 0
    for kw in (dict(fr_=0), dict(fused=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(gl=0), dict(gl=5), dict(gl=256, n=300),
               dict(step=0), dict(step=-2), dict(op=-1), dict(op=4), dict(fill=-1), dict(fill=256), dict(mc=0), dict(mc=256)):
        assert fuse(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert fuse(**kw) == 2, kw

    def mask(fr_=1, valid=1, n=n, h=h, w=w, bg=1, bc=0, per=2, thr=10, mc=1, out=1, changed=1, off=0):
        m, ch = np.full(4 * 6 * 2 + 8, 0x5A, np.uint8), np.full(6, 0x5A5A5A5A5A5A5A5A, np.int64)
        st = L.canny_hip_change_mask(capi._hp(frames) if fr_ else None, capi._hp(bits) if valid else None, n, h, w,
                                     capi._hp(frames) if bg else None, capi._hp(frames) if bc else None, per, thr, mc,
                                     capi._hp(m) if out else None, vp(ch.ctypes.data + off) if changed else None)
        if st:
            assert (m == 0x5A).all() and (ch == 0x5A5A5A5A5A5A5A5A).all(), "a refused call wrote something"
        else:
            assert (m[48:] == 0x5A).all() and (ch[4:] == 0x5A5A5A5A5A5A5A5A).all() and (changed or (ch == 0x5A5A5A5A5A5A5A5A).all())
        return st

    assert mask() == 0 and mask(valid=0, changed=0) == 0 and mask(bc=1, per=1000, thr=255, mc=255) == 0 and mask(thr=0) == 0
    for kw in (dict(fr_=0), dict(bg=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(per=0), dict(per=-1), dict(thr=-1),
               dict(thr=256), dict(mc=0), dict(mc=256), dict(off=4)):
        assert mask(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536)):
        assert mask(**kw) == 2, kw
    # outputs that overlap an input or each other
    buf = np.full(1000, 0x5A, np.uint8)
    at = lambda o: vp(buf.ctypes.data + o)
    for f_at, o_at, c_at in ((0, 0, 600), (0, 215, 600), (100, 0, 600), (0, 600, 100), (0, 300, 350)):
        st = L.canny_hip_fuse_frames(at(f_at), None, 4, 6, 9, 2, 2, 1, 0, 1, at(o_at), at(c_at))   # frames 216 B, outputs 108 B
        assert st == 1 and (buf == 0x5A).all(), (f_at, o_at, c_at)
    for f_at, m_at, ch_at in ((0, 200, 600), (0, 600, 208), (300, 280, 600), (0, 600, 640)):
        st = L.canny_hip_change_mask(at(f_at), None, 4, 6, 9, at(f_at), None, 4, 1, 1, at(m_at), at(ch_at))   # mask 48 B, changed 32 B
        assert st == 1 and (buf == 0x5A).all(), (f_at, m_at, ch_at)
    assert L.canny_hip_fuse_frames(at(0), None, 4, 6, 9, 2, 2, 1, 0, 1, at(216), at(324)) == 0 and (buf[432:] == 0x5A).all()


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2300
    assert capi.load().canny_hip_version() >= 2300
    for word in ("CANNY_HIP_FUSE_MEAN   = 0", "CANNY_HIP_FUSE_MEDIAN = 1", "CANNY_HIP_FUSE_MIN    = 2", "CANNY_HIP_FUSE_MAX    = 3",
                 "0.23.0", "(2 s + c) / (2 c)", "(c - 1) >> 1", "PAD BITS OF THE INPUT ARE IGNORED", "PAD\n *     BITS WRITTEN 0",
                 "CANNY_HIP_FUSE_PART_FUSE = 0", "CANNY_HIP_FUSE_PART_MASK = 1", "\"fuse_route\"", "exponential update",
                 "morphology on the mask", "CANNY_HIP_FUSE_MAX_GROUP %d" % capi.FUSE_MAX_GROUP,
                 "CANNY_HIP_FUSE_MEAN_ROW %d" % capi.FUSE_MEAN_ROW):
        assert word in header, word
    for name in ("canny_hip_dev_fuse_frames", "canny_hip_fuse_frames", "canny_hip_dev_change_mask", "canny_hip_change_mask",
                 "canny_hip_canny_background", "canny_hip_fuse_profile_get", "canny_hip_selftest_fuse_plan",
                 "canny_hip_selftest_fuse_mean"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for method in ("dev_fuse_frames", "dev_change_mask", "canny_background", "fuse_profile", "selftest_fuse_mean"):
        assert hasattr(capi.Context, method), method
    assert (capi.FUSE_MEAN, capi.FUSE_MEDIAN, capi.FUSE_MIN, capi.FUSE_MAX) == fr.OPS
    assert (capi.FUSE_ROUTE_AUTO, capi.FUSE_ROUTE_REGISTERS, capi.FUSE_ROUTE_PASSES) == (0, 1, 2)
    assert capi.FUSE_MEAN_ROW == fr.MEAN_ROW and capi.FUSE_MAX_GROUP == fr.MAX_GROUP


def test_the_reciprocal_of_the_mean_is_exact_on_the_whole_domain():
    """What the kernels compute, in Python ints: M(c) = (2^32 - 1) // (2c) + 1 and q = (n * M(c)) >> 32 with n = 2s + c, against
    the rule on all 8.3 M pairs -- the proof the header states, and what canny_hip_selftest_fuse_mean repeats on the device."""
    for c in range(1, 256):
        m = (2 ** 32 - 1) // (2 * c) + 1
        e = m * 2 * c - 2 ** 32
        assert 0 <= e < 2 * c and m < 2 ** 32 and (2 * 255 * c + c) * e < 2 ** 32
        s = np.arange(255 * c + 1, dtype=np.uint64)
        n = 2 * s + c
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(2 * c)), c


# ---- the host rules under the host compiler's sanitizers ----------------------------------------------------------------
def test_host_rules_run_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_fuse_host.cpp has its own main and is compiled together with csrc/canny_fuse_host.cpp alone: nothing of
    it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_fuse_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_fuse_host.cpp"),
                           os.path.join(csrc, "canny_fuse_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fuse ok" in r.stdout, r.stdout + r.stderr
