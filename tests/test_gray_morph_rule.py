"""Grey-level morphology and median filtering, host side: tests/gray_morph_rule.py against answers that
do not come from the rule (scipy.ndimage), canny_hip_gray_morph (plain C++, no device) against the numpy rule byte for byte,
the two facts that tie the operator to the binary morphology, the header and bindings, the refused calls, and the host file
under the host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import gray_morph_rule as R
import morph_rule as M
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENTS = R.named_elements()
NAMES = tuple(ELEMENTS)
BORDER_CASES = ((R.BORDER_NEUTRAL, 0), (R.BORDER_REPLICATE, 0), (R.BORDER_CONSTANT, 0), (R.BORDER_CONSTANT, 255),
                (R.BORDER_CONSTANT, 77))
MEDIAN_BORDERS = tuple(b for b in BORDER_CASES if b[0] != R.BORDER_NEUTRAL)


def both(px, op, el, border=(R.BORDER_NEUTRAL, 0), iterations=1):
    """The host C++ and the numpy rule, compared."""
    rows, kw, kh = el
    px = np.asarray(px, np.uint8)
    px = px[None] if px.ndim == 2 else px
    out = capi.gray_morph(px, op, rows, kw, kh, border[0], border[1], iterations)
    want = R.gray_morph(px, op, rows, kw, kh, border[0], border[1], iterations)
    assert out.dtype == np.uint8 and np.array_equal(out, want), f"op {op} border {border} x{iterations}: the host differs from the rule"
    return out


def scipy_mode(border, erode):
    mode, value = border
    if mode == R.BORDER_REPLICATE:
        return dict(mode="nearest")
    return dict(mode="constant", cval=value if mode == R.BORDER_CONSTANT else (255 if erode else 0))


def sp_erode(px, fp, border, iterations=1):
    for _ in range(iterations):
        px = ndimage.grey_erosion(px, footprint=fp, **scipy_mode(border, True))
    return px


def sp_dilate(px, fp, border, iterations=1):
    for _ in range(iterations):
        px = ndimage.grey_dilation(px, footprint=fp, **scipy_mode(border, False))
    return px


def random_element(rng, kmax=9):
    kw, kh = (int(2 * rng.integers(0, kmax // 2 + 1) + 1) for _ in range(2))
    a = rng.random((kh, kw)) < rng.choice([0.3, 0.6, 0.9])
    a[rng.integers(kh), rng.integers(kw)] = True
    return M.rows_of(a)


# ---- the numpy rule against scipy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDER_CASES)
def test_the_primitives_are_scipy_grey_erosion_and_dilation(border):
    rng = np.random.default_rng(39 + border[0] * 256 + border[1])
    for k in range(24):
        el = random_element(rng) if k % 3 else ELEMENTS[("L", "rect5x3", "ring3x3", "cross5x5", "ellipse7x7", "rect3x5", "rect3x3", "1x1")[k // 3]]
        rows, kw, kh = el
        fp = M.element_array(rows, kw, kh)
        h, w = int(rng.integers(kh, kh + 20)), int(rng.integers(kw, kw + 30))
        px = R.named_planes(1, h, w, k)[("random", "few_valued", "two_valued")[k % 3]][0]
        it = 1 + k % 2
        assert np.array_equal(R.gray_morph(px[None], R.ERODE, rows, kw, kh, *border, it)[0], sp_erode(px, fp, border, it)), (k, el)
        assert np.array_equal(R.gray_morph(px[None], R.DILATE, rows, kw, kh, *border, it)[0], sp_dilate(px, fp, border, it)), (k, el)


def test_the_issues_own_check_13_x_17_with_an_asymmetric_5_x_3_element():
    px = np.random.default_rng(1317).integers(0, 256, (13, 17), dtype=np.uint8)
    fp = np.array([[1, 1, 0, 0, 0], [0, 1, 1, 1, 0], [0, 0, 0, 1, 1]], bool)
    rows, kw, kh = M.rows_of(fp)
    for border in BORDER_CASES:
        assert np.array_equal(both(px, R.ERODE, (rows, kw, kh), border)[0], sp_erode(px, fp, border))
        assert np.array_equal(both(px, R.DILATE, (rows, kw, kh), border)[0], sp_dilate(px, fp, border))
    assert np.array_equal(sp_erode(px, fp, (R.BORDER_REPLICATE, 0)), ndimage.minimum_filter(px, footprint=fp, mode="nearest"))


@pytest.mark.parametrize("k", [3, 5])
def test_the_median_is_scipy_median_filter(k):
    el = ELEMENTS["rect%dx%d" % (k, k)]
    for j, name in enumerate(("random", "few_valued", "two_valued", "checker", "impulse_bright", "ramp_xy")):
        px = R.named_planes(2, 9 + j, 14 + 3 * j, j)[name]
        for border in MEDIAN_BORDERS:
            kw = dict(mode="nearest") if border[0] == R.BORDER_REPLICATE else dict(mode="constant", cval=border[1])
            want = np.stack([ndimage.median_filter(f, size=k, **kw) for f in px])
            assert np.array_equal(both(px, R.MEDIAN, el, border), want), (name, border)
            twice = np.stack([ndimage.median_filter(f, size=k, **kw) for f in want])
            assert np.array_equal(both(px, R.MEDIAN, el, border, 2), twice), (name, border)


@pytest.mark.parametrize("border", BORDER_CASES)
def test_the_composites_are_compositions_of_scipys_primitives(border):
    rng = np.random.default_rng(border[0] * 1000 + border[1])
    for k, name in enumerate(("L", "rect5x3", "ellipse7x7", "ring3x3")):
        rows, kw, kh = ELEMENTS[name]
        fp = M.element_array(rows, kw, kh)
        px = R.named_planes(1, 21 + k, 33 + k, k)[("random", "few_valued")[k % 2]][0]
        it = 1 + k % 2
        e, d = sp_erode(px, fp, border, it), sp_dilate(px, fp, border, it)
        o, c = sp_dilate(e, fp, border, it), sp_erode(d, fp, border, it)
        sub = lambda a, b: np.clip(a.astype(int) - b.astype(int), 0, 255).astype(np.uint8)
        for op, want in ((R.OPEN, o), (R.CLOSE, c), (R.GRADIENT, sub(d, e)), (R.TOPHAT, sub(px, o)), (R.BLACKHAT, sub(c, px))):
            assert np.array_equal(both(px, op, (rows, kw, kh), border, it)[0], want), (name, op)
    # under a CONSTANT border the opening need not lie below the input: the difference saturates instead of wrapping
    px = np.full((1, 5, 5), 10, np.uint8)
    opened = both(px, R.OPEN, ELEMENTS["rect3x3"], (R.BORDER_CONSTANT, 200))
    assert (opened > px).any() and not both(px, R.TOPHAT, ELEMENTS["rect3x3"], (R.BORDER_CONSTANT, 200)).any()


# ---- the host C++ against the numpy rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_follows_the_rule_on_every_element_op_and_border(name):
    el = ELEMENTS[name]
    for op in R.OPS:
        if op == R.MEDIAN and name not in R.MEDIAN_NAMES:
            continue
        for b, border in enumerate(BORDER_CASES):
            if op == R.MEDIAN and border[0] == R.BORDER_NEUTRAL:
                continue
            k = 5 * (8 * NAMES.index(name) + op) + b
            n, h, w = (1, 3, 2)[k % 3], (1, 2, 15, 17, 33)[(k // 3) % 5], (1, 7, 9, 31, 33, 65)[k % 6]
            plane = R.named_planes(n, h, w, k)[R.PLANE_NAMES[k % len(R.PLANE_NAMES)]]
            both(plane, op, el, border, (1, 2, 1, 1, 3)[k % 5])


@pytest.mark.parametrize("plane", R.PLANE_NAMES)
def test_host_follows_the_rule_on_every_named_plane(plane):
    for j, name in enumerate(("rect3x3", "rect5x5", "L", "ellipse7x7", "far_bit", "rect31x31")):
        for b, border in enumerate(BORDER_CASES):
            k = 5 * (6 * R.PLANE_NAMES.index(plane) + j) + b
            px = R.named_planes(2, (17, 34)[k % 2], (33, 41, 129)[k % 3], k)[plane]
            both(px, R.OPS[k % 7], ELEMENTS[name], border, 1 + k % 2)
            if name in R.MEDIAN_NAMES and border[0] != R.BORDER_NEUTRAL:
                both(px, R.MEDIAN, ELEMENTS[name], border, 1 + k % 2)


@pytest.mark.parametrize("iterations", [1, 2, 16])
def test_host_follows_the_rule_on_frames_smaller_than_the_element(iterations):
    rng = np.random.default_rng(iterations)
    for border in BORDER_CASES:
        for op in R.MORPH_OPS:
            both(rng.integers(0, 256, (2, 1, 1), dtype=np.uint8), op, ELEMENTS["rect31x31"], border, iterations)
            both(rng.integers(0, 256, (2, 3, 2), dtype=np.uint8), op, ELEMENTS["random31_1"], border, iterations)
            both(rng.integers(0, 256, (1, 2, 3), dtype=np.uint8), op, ELEMENTS["L"], border, iterations)
        if border[0] != R.BORDER_NEUTRAL:
            both(rng.integers(0, 256, (3, 2, 3), dtype=np.uint8), R.MEDIAN, ELEMENTS["rect5x5"], border, iterations)
            both(rng.integers(0, 256, (3, 1, 1), dtype=np.uint8), R.MEDIAN, ELEMENTS["rect3x3"], border, iterations)


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_k_iterations_of_rect3_are_one_step_of_the_wider_rectangle(k):
    px = R.named_planes(2, 23, 37, k)["random"]
    wide = (M.element(M.RECT, 2 * k + 1, 2 * k + 1), 2 * k + 1, 2 * k + 1)
    for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
        for border in ((R.BORDER_NEUTRAL, 0), (R.BORDER_REPLICATE, 0)):
            assert np.array_equal(both(px, op, ELEMENTS["rect3x3"], border, k), both(px, op, wide, border)), (k, op, border)


def test_an_impulse_dilates_to_the_element_and_erodes_to_its_reflection():
    for name in ("L", "far_bit", "rect5x3", "random31_0"):
        rows, kw, kh = ELEMENTS[name]
        fp = M.element_array(rows, kw, kh)
        h, w, y, x = 37, 45, 18, 22                                 # REPLICATE: an element without its centre reads only background outside
        px = np.full((h, w), 3, np.uint8)
        px[y, x] = 250
        want = np.full((h, w), 3, np.uint8)
        want[y - kh // 2:y + kh // 2 + 1, x - kw // 2:x + kw // 2 + 1][fp] = 250
        assert np.array_equal(both(px, R.DILATE, (rows, kw, kh), (R.BORDER_REPLICATE, 0))[0], want), name
        want = np.full((h, w), 252, np.uint8)
        want[y - kh // 2:y + kh // 2 + 1, x - kw // 2:x + kw // 2 + 1][fp[::-1, ::-1]] = 5
        dark = np.full((h, w), 252, np.uint8)
        dark[y, x] = 5
        assert np.array_equal(both(dark, R.ERODE, (rows, kw, kh), (R.BORDER_REPLICATE, 0))[0], want), name


# ---- the two facts that tie the operator to the binary morphology ---------------------------------------------------------
BINARY_BORDER = {(R.BORDER_NEUTRAL, 0): M.BORDER_NEUTRAL, (R.BORDER_CONSTANT, 0): M.BORDER_ZERO, (R.BORDER_CONSTANT, 255): M.BORDER_ONE}


@pytest.mark.parametrize("thr", [0, 1, 127, 128, 254])
def test_threshold_decomposition(thr):
    for k, name in enumerate(("rect3x3", "L", "ellipse7x7", "rect5x3", "random31_1", "ring3x3")):
        rows, kw, kh = ELEMENTS[name]
        px = R.named_planes(2, 19 + k, 35 - k, 100 * thr + k)[("few_valued", "random")[k % 2]]
        for border, binary in BINARY_BORDER.items():
            for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
                it = 1 + (k + op) % 2
                got = both(px, op, (rows, kw, kh), border, it) > thr
                assert np.array_equal(got, M.morph_px(px > thr, op, rows, kw, kh, binary, it)), (name, border, op)
    # the median of a 0/1 plane is the majority of its window
    for k in (3, 5):
        px = R.named_planes(2, 14, 19, thr + k)["few_valued"]
        for border in ((R.BORDER_REPLICATE, 0), (R.BORDER_CONSTANT, 0), (R.BORDER_CONSTANT, 255)):
            got = both(px, R.MEDIAN, ELEMENTS["rect%dx%d" % (k, k)], border) > thr
            ones = R.padded((px > thr).astype(np.uint8), k // 2, k // 2, "median", border[0], int(border[1] > thr))
            count = sum(ones[:, j:j + 14, i:i + 19] for j in range(k) for i in range(k))
            assert np.array_equal(got, count > k * k // 2), (k, border)


def test_on_two_valued_planes_the_operator_is_the_binary_one():
    for k, name in enumerate(NAMES):
        rows, kw, kh = ELEMENTS[name]
        bits = M.named_patterns(2, 21, 37, k)[("random0.50", "random0.05", "random0.95", "checker")[k % 4]]
        px = bits.astype(np.uint8) * 255
        for border, binary in BINARY_BORDER.items():
            for op in R.MORPH_OPS:
                it = 1 + (k + op) % 2
                want = M.morph_px(bits, op, rows, kw, kh, binary, it).astype(np.uint8) * 255
                assert np.array_equal(both(px, op, (rows, kw, kh), border, it), want), (name, border, op)


# ---- the use case ---------------------------------------------------------------------------------------------------------
def test_blackhat_then_otsu_finds_the_blobs_on_a_ramp_and_otsu_alone_does_not():
    import binarize_rule as B
    plane, truth = R.blobs_on_ramp()
    h, w = plane.shape
    hat = both(plane, R.BLACKHAT, ELEMENTS["rect15x15"])
    # the closing restores the ramp under the blobs; at the frame's dark end the closing of a ramp is flat, a few grey levels
    assert (hat[0][truth] == 35).all() and hat[0][~truth].max() <= 8 and not hat[0][:, 7:][~truth[:, 7:]].any()
    bits, counts, thr = capi.binarize(hat, capi.BIN_OTSU)
    assert np.array_equal(B.unpack(bits, w)[0], truth) and counts.tolist() == [int(truth.sum())]
    labels, stats, n = capi.components_from_bits(bits[0], h, w)
    assert n == 8 and np.array_equal(labels != 0, truth)
    alone = B.unpack(capi.binarize(plane[None], capi.BIN_OTSU, invert=1)[0], w)[0]
    assert not np.array_equal(alone, truth) and capi.components_from_bits(B.pack(alone), h, w)[2] != 8


# ---- refused calls --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_sentinels_untouched():
    L = capi.load()
    n, h, w = 2, 6, 9
    planes = np.random.default_rng(3).integers(0, 256, (n, h, w), dtype=np.uint8)
    n_out = n * h * w

    def call(src=1, n=n, h=h, w=w, op=R.OPEN, rows=(7, 7, 7), kw=3, kh=3, mode=0, value=0, it=1, out=1):
        o = np.full(n_out + 8, 0x5A, np.uint8)
        r = np.array(rows, np.uint32) if rows is not None else None
        st = L.canny_hip_gray_morph(capi._hp(planes) if src else None, n, h, w, op, capi._hp(r) if r is not None else None, kw, kh,
                                    mode, value, it, capi._hp(o) if out else None)
        if st:
            assert (o == 0x5A).all(), "a refused call wrote something"
        else:
            assert (o[n_out:] == 0x5A).all()
        return st

    f5 = (31,) * 5
    assert call() == 0 and call(it=16, op=R.BLACKHAT, mode=2, value=255) == 0 and call(rows=(5, 0, 2)) == 0
    assert call(op=R.MEDIAN, mode=1) == 0 and call(op=R.MEDIAN, mode=2, value=9, rows=f5, kw=5, kh=5) == 0
    assert call(mode=0, value=999) == 0 and call(mode=1, value=-5) == 0          # border_value is ignored by the other two modes
    for kw in (dict(src=0), dict(out=0), dict(rows=None), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(op=-1), dict(op=8),
               dict(mode=-1), dict(mode=3), dict(mode=2, value=256), dict(mode=2, value=-1), dict(it=0), dict(it=17), dict(it=-1),
               dict(rows=(7, 8, 7)), dict(rows=(7, 7, 1 << 31)), dict(rows=(0, 0, 0)), dict(kw=2), dict(kw=4, rows=(15, 15, 15)),
               dict(kh=2), dict(kw=33), dict(kh=33, rows=(1,) * 33), dict(kw=0), dict(kh=0), dict(kw=-3),
               dict(op=R.MEDIAN, mode=0), dict(op=R.MEDIAN, mode=1, rows=(7, 5, 7)), dict(op=R.MEDIAN, mode=1, rows=(7,) * 5, kh=5),
               dict(op=R.MEDIAN, mode=1, rows=(127,) * 7, kw=7, kh=7), dict(op=R.MEDIAN, mode=1, rows=(1,), kw=1, kh=1),
               dict(op=R.MEDIAN, mode=1, rows=(31,) * 3, kw=5, kh=3)):
        assert call(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert call(**kw) == 2, kw
    # an output that overlaps the input: there is no in-place form
    buf = np.full(400, 0x5A, np.uint8)
    at = lambda o: capi.C.c_void_p(buf.ctypes.data + o)
    rows = np.array([7, 7, 7], np.uint32)
    for i_at, o_at in ((0, 0), (0, 107), (50, 0), (10, 100)):        # planes 108 B
        assert L.canny_hip_gray_morph(at(i_at), n, h, w, R.OPEN, capi._hp(rows), 3, 3, 0, 0, 1, at(o_at)) == 1 and (buf == 0x5A).all()
    assert L.canny_hip_gray_morph(at(0), n, h, w, R.OPEN, capi._hp(rows), 3, 3, 0, 0, 1, at(108)) == 0 and (buf[216:] == 0x5A).all()


# ---- header and bindings --------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2800
    assert capi.load().canny_hip_version() >= 2800
    for word in ("0.28.0: + grey-level morphology and median filtering of u8 planes", "min over b in B of in(p + b)",
                 "max over b in B of in(p - b)", "CANNY_HIP_GRAY_BORDER_NEUTRAL = 0", "CANNY_HIP_GRAY_BORDER_REPLICATE = 1",
                 "CANNY_HIP_GRAY_BORDER_CONSTANT = 2", "SATURATE AT 0", "THRESHOLD DECOMPOSITION", "TWO-VALUED PLANES",
                 "(k^2 - 1) / 2-th", "\"gray_morph_route\"", "no in-place form", "window medians above 5 x 5 by histogram",
                 "iteration fusing", "s16 planes", "grey-level reconstruction", "the batch pipeline or the multi-GPU sharder",
                 "\"gray_morph\""):
        assert word in header, word
    for name in ("canny_hip_dev_gray_morph", "canny_hip_gray_morph_batch", "canny_hip_gray_morph", "canny_hip_selftest_gray_morph_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for method in ("dev_gray_morph", "gray_morph_batch"):
        assert hasattr(capi.Context, method), method
    assert (capi.GRAY_ERODE, capi.GRAY_DILATE, capi.GRAY_OPEN, capi.GRAY_CLOSE, capi.GRAY_GRADIENT, capi.GRAY_TOPHAT,
            capi.GRAY_BLACKHAT, capi.GRAY_MEDIAN) == R.OPS
    assert (capi.GRAY_BORDER_NEUTRAL, capi.GRAY_BORDER_REPLICATE, capi.GRAY_BORDER_CONSTANT) == R.BORDERS
    for i, op in enumerate(("ERODE", "DILATE", "OPEN", "CLOSE", "GRADIENT", "TOPHAT", "BLACKHAT", "MEDIAN")):
        assert re.search(rf"CANNY_HIP_GRAY_{op} = {i}\b", header), op
    assert len(capi.GRAY_OPS) == 8 and capi.GRAY_OPS[7] == "median" and capi.GRAY_OPS[:7] == capi.MORPH_OPS


# ---- the host rule under the host compiler's sanitizers -------------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_gray_morph_host.cpp has its own main and is compiled together with csrc/canny_gray_morph_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_gray_morph_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_gray_morph_host.cpp"),
                           os.path.join(csrc, "canny_gray_morph_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gray morph ok" in r.stdout, r.stdout + r.stderr
