"""The host-only entry points of the Hough circles (canny_hip_hough_circles_from_bits, canny_hip_hough_circles_step_of;
include/canny_hip.h) against the numpy restatement of the rule (tests/hough_circles_rule.py), the rule's
Sobel against the oracle's, a drawn frame on which the rule has to find the discs that were drawn, the statuses and the -r
grammar of the command line.  Every comparison is exact equality on whole arrays; the record buffer is sentinel-filled with
a guard behind it.  No GPU is needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hough_circles_rule as cr
import oracle
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.int32(-0x5A5A5A5B)
N_GUARD = 64


def random_case(h, w, density, seed, extremes=False):
    """(mask, gx, gy): a Bernoulli mask and gradient planes in the Sobel domain with zeros sprinkled in (both components on a
    twentieth of the pixels, one of them on another tenth); with `extremes` a share of the pixels holds the ends of s16."""
    rng = np.random.default_rng(seed)
    mask = rng.random((h, w)) < density
    gx, gy = (rng.integers(-1020, 1021, (h, w)).astype(np.int16) for _ in range(2))
    zero = rng.random((h, w))
    gx[zero < 0.10] = 0
    gy[(zero < 0.05) | (zero > 0.95)] = 0
    if extremes:
        pick = rng.random((h, w))
        ends = np.array([32767, -32768, -32767, 32767], np.int16)
        gx[pick < 0.2] = rng.choice(ends, (h, w))[pick < 0.2]
        gy[(pick > 0.1) & (pick < 0.3)] = rng.choice(ends, (h, w))[(pick > 0.1) & (pick < 0.3)]
    return mask, gx, gy


def _lib(mask, gx, gy, args):
    """The library's (records, n_peaks, accumulator); the record buffer is guarded."""
    h, w = mask.shape
    cap = args[-1]
    buf = np.full(cap * 6 + N_GUARD, SENT, np.int32)
    rec, n_peaks, acc = capi.hough_circles_from_bits(np.packbits(mask, axis=-1), gx, gy, h, w, *args, want_accum=True, out=buf)
    assert (buf[len(rec) * 6:] == SENT).all(), "slots past the count (or the guard) were written"
    return rec.copy(), n_peaks, acc


@pytest.mark.parametrize("cell_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("shape,density", [((37, 77), 0.02), ((37, 77), 0.3), ((70, 130), 0.02), ((70, 130), 0.3)],
                         ids=lambda v: str(v))
def test_host_rule_equals_numpy(shape, density, cell_shift):
    h, w = shape
    mask, gx, gy = random_case(h, w, density, seed=h * 131 + w + cell_shift, extremes=cell_shift == 2)
    seen = 0
    for lo, hi in [(1, 1), (3, 3), (1, 40), (20, 90)]:
        acc = cr.accumulate(mask, gx, gy, lo, hi, cell_shift)
        top = int(acc.max())
        for threshold, support, min_dist, cap in [(0, 0, 0, 4096), (top // 2, 1, 5, 64), (0, 2, 1000, 7), (top, 0, 0, 7)]:
            want, n_peaks = cr.circles(mask, acc, lo, hi, cell_shift, threshold, support, min_dist, cap)
            got, got_peaks, got_acc = _lib(mask, gx, gy, (lo, hi, cell_shift, threshold, support, min_dist, cap))
            what = f"{shape} {density} shift {cell_shift} radii {lo}..{hi} thr {threshold}/{support} dist {min_dist} cap {cap}"
            assert np.array_equal(got_acc, acc), f"{what}: accumulator"
            assert got_peaks == n_peaks, f"{what}: {got_peaks} peaks != {n_peaks}"
            assert np.array_equal(got, want), f"{what}: records"
            seen += len(want)
    assert seen > 0


def test_step_of_equals_the_numpy_step():
    values = [0, 1, -1, 2, 3, -3, 4, 5, 7, 255, -255, 256, 724, 1019, 1020, -1020, 1021, 4096, -4097, 32766, 32767, -32767,
              -32768]
    gx, gy = (v.ravel() for v in np.meshgrid(values, values))
    sx, sy = cr.step(gx, gy)
    got = np.array([capi.hough_circles_step_of(int(a), int(b)) for a, b in zip(gx, gy)])
    assert np.array_equal(got[:, 0], sx) and np.array_equal(got[:, 1], sy)
    assert capi.hough_circles_step_of(0, 0) == (0, 0)
    assert capi.hough_circles_step_of(-32768, -32768) == (-724, -724)
    assert capi.hough_circles_step_of(1, 1020) == (1, 1024) and capi.hough_circles_step_of(32767, 5) == (1024, 0)
    assert capi.hough_circles_step_of(3, 4) == (614, 819)  # 3072 / 5 = 614.4, 4096 / 5 = 819.2
    for bad in [(32768, 0), (0, -32769)]:
        with pytest.raises(capi.CannyHipError):
            capi.hough_circles_step_of(*bad)


@pytest.mark.parametrize("shape", [(2, 2), (2, 9), (9, 2), (37, 77), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_rules_sobel_is_the_oracles(shape):
    plane = np.random.default_rng(shape[0] * 7 + shape[1]).integers(0, 256, shape).astype(np.int16)
    gx, gy = cr.sobel(plane)
    ogx, ogy = oracle.xy_gradient(plane)
    assert np.array_equal(gx, ogx) and np.array_equal(gy, ogy)


DISCS = [(40, 44, 20, 200), (60, 96, 12, 160), (20, 100, 9, 220)]  # cy, cx, r, value


def disc_frame():
    img = np.full((96, 128), 40, np.uint8)
    yy, xx = np.mgrid[:96, :128]
    for cy, cx, r, v in DISCS:
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    return img


def test_the_rule_finds_the_drawn_discs():
    img = disc_frame()
    mask = oracle.canny(img, 1.4, 50, 150) != 0
    gx, gy = cr.sobel(oracle.gaussian(img, 1.4))
    assert int(mask.sum()) == 164 and not ((gx == 0) & (gy == 0) & mask).any()
    acc = cr.accumulate(mask, gx, gy, 5, 30, 0)
    rec, n_peaks = cr.circles(mask, acc, 5, 30, 0, 20, 10, 0, 256)
    assert n_peaks == 3 and rec[:, 3].tolist() == [30, 26, 26] and rec[:, 4].tolist() == [25, 19, 30]
    found = sorted((int(y2) // 2, int(x2) // 2, int(r)) for x2, y2, r in rec[:, :3])  # cell (ax, ay) = floor of the centre
    assert found == sorted((cy, cx, r) for cy, cx, r, _ in DISCS)
    got, got_peaks, got_acc = _lib(mask, gx, gy, (5, 30, 0, 20, 10, 0, 256))
    assert np.array_equal(got, rec) and got_peaks == 3 and np.array_equal(got_acc, acc)


def test_statuses_and_nothing_written():
    L = capi.load()
    mask, gx, gy = random_case(20, 30, 0.2, seed=3)
    bits = np.packbits(mask, axis=-1)
    out = np.full(6 * 8 + N_GUARD, SENT, np.int32)
    acc = np.full(22 * 32 + N_GUARD, SENT, np.int32)
    count, peaks = C.c_int(-77), C.c_int(-78)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(bits=ptr(bits), gx=ptr(gx), gy=ptr(gy), h=20, w=30, lo=2, hi=9, shift=0, thr=0, sup=0, dist=0, cap=8,
              rec=ptr(out), count=C.byref(count), peaks=C.byref(peaks), acc=ptr(acc))

    def call(**kw):
        a = dict(ok, **kw)
        return L.canny_hip_hough_circles_from_bits(a["bits"], a["gx"], a["gy"], a["h"], a["w"], a["lo"], a["hi"], a["shift"],
                                                   a["thr"], a["sup"], a["dist"], a["cap"], a["rec"], a["count"], a["peaks"],
                                                   a["acc"])

    invalid = [dict(lo=0), dict(lo=-1), dict(lo=10), dict(shift=-1), dict(shift=4), dict(cap=0), dict(cap=-3),
               dict(dist=-1), dict(count=None), dict(gx=None), dict(gy=None), dict(bits=None), dict(h=1), dict(w=1),
               dict(h=0), dict(w=-5)]
    unsupported = [dict(hi=capi.CIRCLES_MAX_RADIUS + 1), dict(cap=capi.HOUGH_MAX_LINES + 1)]
    for status, cases in ((1, invalid), (2, unsupported)):
        for kw in cases:
            assert call(**kw) == status, kw
            assert (out == SENT).all() and (acc == SENT).all() and count.value == -77 and peaks.value == -78, kw
    assert call(hi=capi.CIRCLES_MAX_RADIUS, cap=capi.HOUGH_MAX_LINES, rec=None) == 0 and count.value >= 0  # at the limits
    assert call(rec=None, peaks=None, acc=None) == 0
    assert call() == 0 and 0 < count.value <= 8 and peaks.value >= count.value
    assert (acc[22 * 32:] == SENT).all() and (acc[:32] == 0).all()


def test_cli_rejects_a_malformed_r_flag(tmp_path):
    """Grammar only: the flag is parsed before anything touches a device."""
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    for text in ("5,30", "5,30,20", "x", "5,30,20,10,", "5,30,20,10,0,1,7", "0,30,20,10", "30,5,20,10", "5,30,20,10,-1",
                 "5,30,20,10,0,4", "5;30;20;10"):
        r = subprocess.run([exe, "1.4", "50", "150", "-o", str(tmp_path), "-r", text], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "-r expects min_radius,max_radius,threshold,support" in r.stderr, text
        assert not (tmp_path / "canny_circles.txt").exists()
    r = subprocess.run([exe, "1.4", "50", "-r", "5,30,20,10"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr.startswith("USAGE:") and "-r min_radius" in r.stderr  # well-formed: the usual usage


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1100
    assert capi.load().canny_hip_version() >= 1100
    assert re.search(r"#define CANNY_HIP_CIRCLE_INTS 6\b", header) and capi.CIRCLE_INTS == 6
    assert re.search(r"#define CANNY_HIP_CIRCLES_MAX_RADIUS 1024\b", header) and capi.CIRCLES_MAX_RADIUS == 1024
    assert re.search(r"CANNY_HIP_CIRCLE_PARTS = 4\b", header) and len(capi.CIRCLE_PARTS) == 4
    for name in ("canny_hip_hough_circles_step_of", "canny_hip_hough_circles_from_bits", "canny_hip_dev_hough_circles_bits",
                 "canny_hip_dev_canny_hough_circles", "canny_hip_canny_hough_circles", "canny_hip_dev_hough_circles_steps",
                 "canny_hip_hough_circles_profile_get"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(capi.load(), name)
    for method in ("dev_canny_hough_circles", "dev_hough_circles_bits", "canny_hough_circles", "dev_hough_circles_steps",
                   "hough_circles_profile_get"):
        assert callable(getattr(capi.Context, method))
    assert callable(capi.hough_circles_from_bits) and callable(capi.hough_circles_step_of)
