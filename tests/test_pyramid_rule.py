"""The image pyramid rule (include/canny_hip.h) without a GPU: tests/pyramid_rule.py against scipy and
against the rule's stated facts, the layout arithmetic, the host rule canny_hip_pyramid / canny_hip_pyr_up through ctypes byte
for byte, every refused call with its outputs untouched, the header, and tests/cpp/test_pyramid_host.cpp under the host
compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import pyramid_rule as R
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (3, 5), (2, 9), (7, 6), (33, 70))
K = np.array(R.TAPS, np.int64)
SENT = 0x5A


def random_planes(n, h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def ups(h, w):
    return [(oh, ow) for oh in (2 * h - 1, 2 * h) for ow in (2 * w - 1, 2 * w)]


# ---- the rule is scipy's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_down_is_scipys_mirror_correlation_decimated(h, w):
    planes = random_planes(3, h, w)
    got = R.pyr_down(planes)
    assert got.shape == (3, (h + 1) // 2, (w + 1) // 2) and got.dtype == np.uint8
    for f in range(3):
        t = ndimage.correlate1d(planes[f].astype(np.int64), K, axis=0, mode="mirror")
        t = ndimage.correlate1d(t, K, axis=1, mode="mirror")[::2, ::2]
        assert np.array_equal(got[f], (t + 128) >> 8), (h, w, f)


@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_up_is_scipys_mirror_correlation_of_the_zero_inserted_grid(h, w):
    planes = random_planes(2, h, w, 1)
    for f in range(2):
        z = np.zeros((2 * h, 2 * w), np.int64)
        z[::2, ::2] = planes[f]
        t = ndimage.correlate1d(ndimage.correlate1d(z, K, axis=0, mode="mirror"), K, axis=1, mode="mirror")
        want = (t + 32) >> 6
        for oh, ow in ups(h, w):                                     # cropping the last row or column changes no value
            got = R.pyr_up(planes, oh, ow)
            assert got.shape == (2, oh, ow) and np.array_equal(got[f], want[:oh, :ow]), (h, w, oh, ow)


def test_fold_is_reflect_101_and_loops_on_short_axes():
    assert [R.fold(p, 1) for p in range(-5, 6)] == [0] * 11
    assert [R.fold(p, 2) for p in range(-4, 6)] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [R.fold(p, 3) for p in range(-4, 7)] == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]
    assert [R.fold(p, 5) for p in range(-2, 7)] == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    for n in (3, 4, 7):                                              # numpy's own mirror
        assert [R.fold(p, n) for p in range(-2, n + 2)] == np.pad(np.arange(n), 2, mode="reflect").tolist()
    for n in range(1, 12):
        assert R.down_matrix(n).sum(axis=1).tolist() == [16] * ((n + 1) // 2)
        for on in (2 * n - 1, 2 * n):
            assert R.up_matrix(n, on).sum(axis=1).tolist() == [8] * on


# ---- the facts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_a_constant_plane_stays_constant(h, w):
    for v in (0, 1, 127, 254, 255):
        flat = np.full((2, h, w), v, np.uint8)
        assert (R.pyr_down(flat) == v).all()
        for oh, ow in ups(h, w):
            assert (R.pyr_up(flat, oh, ow) == v).all()


@pytest.mark.parametrize("h,w", SHAPES)
def test_flips(h, w):
    """pyrDown commutes with the flip of an axis of ODD length (its samples 0, 2, .. are symmetric about the middle); of even
    length the decimation grid moves.  pyrUp to 2 s - 1 samples commutes with the flip in every output sample of that axis BUT
    THE TWO ENDS: the rule's ends differ, s[-1] := s[1] (a mirror) and s[w] := s[w - 1] (the zero-inserted grid's mirror)."""
    planes = random_planes(2, h, w, 2)
    for axis, n in ((1, h), (2, w)):
        flipped = np.flip(planes, axis)
        if n % 2:
            assert np.array_equal(R.pyr_down(flipped), np.flip(R.pyr_down(planes), axis)), (h, w, axis)
        oh, ow = (2 * h - 1, 2 * w) if axis == 1 else (2 * h, 2 * w - 1)
        inner = [slice(None)] * 3
        inner[axis] = slice(1, -1)
        a, b = R.pyr_up(flipped, oh, ow), np.flip(R.pyr_up(planes, oh, ow), axis)
        assert np.array_equal(a[tuple(inner)], b[tuple(inner)]), (h, w, axis)
    # the cases that do not hold, by example
    ramp = np.array([0, 3, 13, 30, 53, 83, 120, 163], np.uint8).reshape(1, 1, 8)
    assert not np.array_equal(R.pyr_down(np.flip(ramp, 2)), np.flip(R.pyr_down(ramp), 2))            # even length
    up, up_f = R.pyr_up(ramp, 1, 15), np.flip(R.pyr_up(np.flip(ramp, 2), 1, 15), 2)
    assert not np.array_equal(up, up_f) and np.array_equal(up[..., 1:-1], up_f[..., 1:-1])          # the two ends
    assert not np.array_equal(R.pyr_up(np.flip(ramp, 2), 1, 16), np.flip(R.pyr_up(ramp, 1, 16), 2))  # 2 s samples


def test_down_then_up_reproduces_a_linear_ramp_away_from_the_border():
    for h, w, c0, cy, cx in ((21, 30, 10, 3, 5), (20, 31, 250, -4, -3), (33, 16, 7, 0, 9)):
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = c0 + cy * yy + cx * xx
        assert ramp.min() >= 0 and ramp.max() <= 255
        ramp = ramp.astype(np.uint8)[None]
        down = R.pyr_down(ramp)
        assert np.array_equal(down[0, 1:-1, 1:-1], ramp[0, ::2, ::2][1:-1, 1:-1])
        back = R.pyr_up(down, h, w)
        assert np.array_equal(back[0, 4:-4, 4:-4], ramp[0, 4:-4, 4:-4]), (h, w)


# ---- the layout ------------------------------------------------------------------------------------------------------------
def test_the_layout():
    assert [R.max_levels(h, w) for h, w in ((1, 1), (1, 2), (2, 2), (3, 5), (5, 300), (70, 77), (65, 257), (32768, 1))] == \
        [0, 1, 1, 3, 9, 7, 9, 15]
    for n, h, w in ((1, 3, 5), (3, 70, 77), (7, 65, 257), (2, 5, 300), (128, 2160, 3840), (65535, 1, 2), (1, 32768, 32768)):
        top = R.max_levels(h, w)
        for levels in range(1, top + 1):
            rows, total = R.layout(n, h, w, levels)
            info, got_total = capi.pyramid_layout(n, h, w, levels)
            assert info.tolist() == [list(r) for r in rows] and got_total == total, (n, h, w, levels)
            hh, ww, end = h, w, 0
            for hl, wl, off, nbytes in rows:
                hh, ww = (hh + 1) // 2, (ww + 1) // 2
                assert (hl, wl, nbytes) == (hh, ww, n * hh * ww) and off % 256 == 0 and 0 <= off - end < 256
                end = off + nbytes
            assert total == end
        assert R.layout(n, h, w, top)[0][-1][:2] == (1, 1) and (top == 1 or R.layout(n, h, w, top - 1)[0][-1][:2] != (1, 1))
        for levels in (0, -1, top + 1, 16, 99):
            with pytest.raises(capi.CannyHipError) as ei:
                capi.pyramid_layout(n, h, w, levels)
            assert ei.value.status == 1, (n, h, w, levels)
    L = capi.load()
    info, total = np.full(8, -7, np.int64), np.full(1, -7, np.int64)
    for args in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 0, 2), (-1, 8, 8, 2), (1, 8, 8, 4), (1, 1, 1, 1)):
        assert L.canny_hip_pyramid_layout(*args, capi._hp(info), capi._hp(total)) == 1, args
    for args in ((65536, 8, 8, 2), (1, 32769, 8, 2), (1, 8, 32769, 2)):
        assert L.canny_hip_pyramid_layout(*args, capi._hp(info), capi._hp(total)) == 2, args
    assert L.canny_hip_pyramid_layout(1, 8, 8, 2, None, capi._hp(total)) == 1
    assert L.canny_hip_pyramid_layout(1, 8, 8, 2, capi._hp(info), None) == 1
    assert (info == -7).all() and (total == -7).all()


# ---- the host rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_host_follows_the_rule(h, w):
    L = capi.load()
    for n in (1, 3):
        planes = random_planes(n, h, w, 3 + n)
        planes[0] = R.named_planes(3, h, w, 5)[2]                    # a checkerboard among them
        for levels in range(1, R.max_levels(h, w) + 1):
            want = R.pyramid(planes, levels)
            got = capi.pyramid(planes, levels)
            assert len(got) == levels and all(np.array_equal(g, x) for g, x in zip(got, want)), (n, h, w, levels)
            total = R.layout(n, h, w, levels)[1]                     # the pads and the bytes behind the buffer stay
            buf = np.full(total + 16, SENT, np.uint8)
            assert L.canny_hip_pyramid(capi._hp(planes), n, h, w, levels, capi._hp(buf)) == 0
            assert np.array_equal(buf[:total], R.pack(want, n, h, w, SENT)) and (buf[total:] == SENT).all(), (n, h, w, levels)
        for oh, ow in ups(h, w):
            assert np.array_equal(capi.pyr_up(planes, oh, ow), R.pyr_up(planes, oh, ow)), (n, h, w, oh, ow)


def test_host_on_extreme_values_does_not_carry():
    for planes in (np.full((1, 9, 11), 255, np.uint8), R.named_planes(3, 12, 13, 0)[2:3], R.named_planes(3, 12, 13, 0)[2:3] ^ 255):
        n, h, w = planes.shape
        assert np.array_equal(capi.pyramid(planes, 2)[1], R.pyramid(planes, 2)[1])
        assert np.array_equal(capi.pyr_up(planes, 2 * h, 2 * w - 1), R.pyr_up(planes, 2 * h, 2 * w - 1))


# ---- refused calls ---------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_sentinels_untouched():
    L = capi.load()
    n, h, w = 2, 6, 9
    planes = random_planes(n, h, w)

    def down(src=1, n=n, h=h, w=w, levels=2, out=1):
        o = np.full(4096, SENT, np.uint8)
        st = L.canny_hip_pyramid(capi._hp(planes) if src else None, n, h, w, levels, capi._hp(o) if out else None)
        assert st == 0 or (o == SENT).all(), "a refused call wrote something"
        return st

    def up(src=1, n=n, h=h, w=w, oh=2 * h, ow=2 * w - 1, out=1):
        o = np.full(4096, SENT, np.uint8)
        st = L.canny_hip_pyr_up(capi._hp(planes) if src else None, n, h, w, oh, ow, capi._hp(o) if out else None)
        assert st == 0 or (o == SENT).all(), "a refused call wrote something"
        return st

    assert down() == 0 and down(levels=4) == 0 and up() == 0 and up(oh=2 * h - 1, ow=2 * w) == 0
    for kw in (dict(src=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(h=-6), dict(levels=0), dict(levels=-1),
               dict(levels=5), dict(levels=16), dict(h=1, w=1, levels=1)):
        assert down(**kw) == 1, kw
    for kw in (dict(src=0), dict(out=0), dict(n=0), dict(h=0, oh=0), dict(w=0, ow=0), dict(n=-1), dict(oh=2 * h + 1), dict(oh=2 * h - 2),
               dict(ow=2 * w + 1), dict(ow=2 * w - 2), dict(oh=h), dict(ow=0), dict(oh=-1)):
        assert up(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert down(**kw) == 2, kw
    for kw in (dict(h=32769, oh=2 * 32769), dict(n=65536), dict(h=16385, oh=32770), dict(w=20000, ow=39999)):
        assert up(**kw) == 2, kw
    # an output that overlaps the input
    buf = np.full(1024, SENT, np.uint8)
    at = lambda o: capi.C.c_void_p(buf.ctypes.data + o)
    total = R.layout(n, h, w, 2)[1]                                  # planes 108 B, the pyramid 256 + 12 B
    for i_at, o_at in ((0, 0), (0, 107), (300, 100), (267, 0)):
        assert L.canny_hip_pyramid(at(i_at), n, h, w, 2, at(o_at)) == 1 and (buf == SENT).all()
    assert total == 268 and L.canny_hip_pyramid(at(268), n, h, w, 2, at(0)) == 0
    assert (buf[30:256] == SENT).all() and (buf[268:] == SENT).all()  # level 1 is 2 x 3 x 5 = 30 B; then the pad
    buf[:] = SENT
    for i_at, o_at in ((0, 0), (0, 107), (500, 200)):                # the output 2 x 12 x 17 = 408 B
        assert L.canny_hip_pyr_up(at(i_at), n, h, w, 12, 17, at(o_at)) == 1 and (buf == SENT).all()
    assert L.canny_hip_pyr_up(at(0), n, h, w, 12, 17, at(108)) == 0 and (buf[108 + 408:] == SENT).all()


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2900
    assert capi.load().canny_hip_version() >= 2900
    for word in ("0.29.0: + image pyramids: pyrDown, pyrUp and whole pyramids of u8 planes", "reflect-101", "THE LOOP MATTERS",
                 "k = (1, 4, 6, 4, 1)", "+ 128) >> 8", "+ 32) >> 6", "WITHOUT A CARRY", "THE CALLER'S CHOICE", "s[-1] := s[min(1, w - 1)]",
                 "s[w] := s[w - 1]", "THE PAD BYTES", "A CONSTANT PLANE", "LINEAR RAMP", "\"pyramid_route\"", "\"pyramid\"",
                 "CANNY_HIP_PYR_PART_DOWN = 0", "CANNY_HIP_PYR_PART_UP = 1", "#define CANNY_HIP_PYR_MAX_LEVELS 15",
                 "two levels in one launch", "Laplacian pyramids", "cv::resize with arbitrary factors",
                 "multi-scale corners and descriptors as one call"):
        assert word in header, word
    for name in ("canny_hip_pyramid_layout", "canny_hip_dev_pyr_down", "canny_hip_dev_pyramid", "canny_hip_dev_pyr_up",
                 "canny_hip_pyramid_batch", "canny_hip_pyr_up_batch", "canny_hip_pyramid", "canny_hip_pyr_up",
                 "canny_hip_selftest_pyramid_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for method in ("dev_pyr_down", "dev_pyramid", "dev_pyr_up", "pyramid_batch", "pyr_up_batch"):
        assert hasattr(capi.Context, method), method
    for fn in ("pyramid_layout", "pyramid", "pyr_up", "pyramid_batch", "pyr_up_batch", "pyramid_plan"):
        assert callable(getattr(capi, fn)), fn
    assert (capi.PYR_ROUTE_AUTO, capi.PYR_ROUTE_DIRECT, capi.PYR_ROUTE_TILED) == (0, 1, 2)
    assert (capi.PYR_PART_DOWN, capi.PYR_PART_UP) == (0, 1) and capi.PYR_PARTS == ("down", "up")
    assert capi.PYR_MAX_LEVELS == R.MAX_LEVELS == 15


# ---- the host rule under the host compiler's sanitizers -------------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_pyramid_host.cpp has its own main and is compiled together with csrc/canny_pyramid_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_pyramid_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_pyramid_host.cpp"),
                           os.path.join(csrc, "canny_pyramid_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pyramid ok" in r.stdout, r.stdout + r.stderr
