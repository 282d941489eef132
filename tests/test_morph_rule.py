"""Binary morphology, host side: canny_hip_morph_bits and canny_hip_morph_element (plain C++, no device)
against tests/morph_rule.py byte for byte, both against answers that do not come from the rule (scipy.ndimage, typed-out
elements, the algebra of openings and closings), the use case on the change masks of section 33, the refused calls, and the
host file under the host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import fuse_rule as fr
import morph_rule as R
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 257)
HEIGHTS = (1, 2, 15, 16, 17, 33, 65)
BATCHES = (1, 3, 5)
ITERATIONS = (1, 2, 5)
ELEMENTS = R.named_elements()
NAMES = tuple(ELEMENTS)
PATTERNS = tuple(R.named_patterns(1, 2, 2))


def both(bits, w, op, el, border=R.BORDER_NEUTRAL, iterations=1):
    """The host C++ and the numpy rule, compared; -> (out bits, counts)."""
    rows, kw, kh = el
    out, counts = capi.morph_bits(bits, w, op, rows, kw, kh, border, iterations)
    want, want_counts = R.morph(bits, w, op, rows, kw, kh, border, iterations)
    assert np.array_equal(out, want), f"w {w} op {op} border {border} x{iterations}: the host differs from the rule"
    assert counts.tolist() == want_counts.tolist()
    return out, counts


def both_px(px, op, el, border=R.BORDER_NEUTRAL, iterations=1):
    px = np.asarray(px, bool)
    px = px[None] if px.ndim == 2 else px
    return R.unpack(both(R.pack(px), px.shape[-1], op, el, border, iterations)[0], px.shape[-1])


def random_element(rng, kmax=9):
    kw, kh = (int(2 * rng.integers(0, kmax // 2 + 1) + 1) for _ in range(2))
    a = rng.random((kh, kw)) < rng.choice([0.3, 0.6, 0.9])
    a[rng.integers(kh), rng.integers(kw)] = True
    return R.rows_of(a)


# ---- the host C++ against the numpy rule, over the shapes, elements and patterns of the GPU tests ---------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_host_follows_the_rule_on_every_width_height_and_border(w):
    for i, h in enumerate(HEIGHTS):
        for border in R.BORDERS:
            k = 3 * (7 * WIDTHS.index(w) + i) + border
            n = BATCHES[k % 3]
            px = R.named_patterns(n, h, w, k)[PATTERNS[k % len(PATTERNS)]]
            both(R.pack_dirty(px, np.random.default_rng(k) if k % 2 else None), w, R.OPS[k % 7], ELEMENTS[NAMES[k % len(NAMES)]],
                 border, ITERATIONS[(k // 2) % 3])


@pytest.mark.parametrize("name", NAMES)
def test_host_follows_the_rule_on_every_element_op_and_border(name):
    for op in R.OPS:
        for border in R.BORDERS:
            k = 3 * (7 * NAMES.index(name) + op) + border + 1000
            n, h, w = BATCHES[k % 3], HEIGHTS[(k // 3) % 7], WIDTHS[k % 13]
            px = R.named_patterns(n, h, w, k)[PATTERNS[k % len(PATTERNS)]]
            both(R.pack_dirty(px), w, op, ELEMENTS[name], border, ITERATIONS[k % 3])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_host_follows_the_rule_on_every_pattern(pattern):
    for j, name in enumerate(("rect3x3", "rect31x31", "ellipse7x7", "far_bit", "alternating31", "random31_1")):
        for border in R.BORDERS:
            k = 3 * (6 * PATTERNS.index(pattern) + j) + border + 4000
            h, w = (17, 65)[k % 2], (33, 129, 257)[k % 3]
            both(R.pack_dirty(R.named_patterns(3, h, w, k)[pattern]), w, R.OPS[k % 7], ELEMENTS[name], border, 1 + k % 2)


# ---- answers that do not come from the rule -------------------------------------------------------------------------------
def scipy_steps(fn, px, structure, iterations, border_value):
    """scipy's `iterations` argument where it can be used: its iterated path corrupts memory when the image is smaller than the
    structure (seen here with scipy 1.15: a wrong answer or "double free or corruption"), so there the single step is repeated."""
    if px.shape[0] >= structure.shape[0] and px.shape[1] >= structure.shape[1]:
        return fn(px, structure, iterations=iterations, border_value=border_value)
    for _ in range(iterations):
        px = fn(px, structure, border_value=border_value)
    return px


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_the_primitives_are_scipy_binary_erosion_and_dilation(density):
    rng = np.random.default_rng(int(density * 100))
    for k in range(40):
        el = random_element(rng) if k % 4 else ELEMENTS[("L", "ring3x3", "cross5x5", "ellipse7x7")[(k // 4) % 4]]
        structure = R.element_array(*el)
        lo_h, lo_w = (1, 1) if k % 5 == 0 else (el[2], el[1])      # every fifth map may be smaller than its element
        h, w = int(rng.integers(lo_h, 40)), int(rng.integers(lo_w, 70))
        px = rng.random((h, w)) < density
        it = ITERATIONS[k % 3]
        for bv, border in ((0, R.BORDER_ZERO), (1, R.BORDER_ONE)):
            want_e = scipy_steps(ndimage.binary_erosion, px, structure, it, bv)
            want_d = scipy_steps(ndimage.binary_dilation, px, structure, it, bv)
            assert np.array_equal(both_px(px, R.ERODE, el, border, it)[0], want_e), (k, el, border)
            assert np.array_equal(both_px(px, R.DILATE, el, border, it)[0], want_d), (k, el, border)
        # the neutral border: the outside constrains nothing
        assert np.array_equal(both_px(px, R.ERODE, el, R.BORDER_NEUTRAL, it)[0], scipy_steps(ndimage.binary_erosion, px, structure, it, 1))
        assert np.array_equal(both_px(px, R.DILATE, el, R.BORDER_NEUTRAL, it)[0], scipy_steps(ndimage.binary_dilation, px, structure, it, 0))


@pytest.mark.parametrize("name", ["L", "far_bit", "ring3x3", "alternating31", "ellipse15x9", "random31_0", "rect5x3"])
def test_one_pixel_dilates_to_the_element_and_one_hole_erodes_to_its_reflection(name):
    """out(p) = OR over b of in(p - b) with one pixel q set is 1 exactly at p = q + b: the Minkowski sum pastes the element
    itself around q, as scipy.ndimage.binary_dilation does (the window a dilated pixel READS is the reflected one).  The
    reflection shows in the erosion: out(p) = AND over b of in(p + b) with one hole q is 0 exactly at p = q - b."""
    el = ELEMENTS[name]
    rows, kw, kh = el
    element = R.element_array(rows, kw, kh)
    h, w = 37, 45                                                   # w % 8 != 0: the last column shares its byte with pad bits
    for y, x in ((18, 22), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (20, w - 1)):
        px = np.zeros((h, w), bool)
        px[y, x] = True
        want = np.zeros((h + 30, w + 30), bool)                     # pasted around the pixel, then clipped by the frame
        want[15 + y - kh // 2:15 + y + kh // 2 + 1, 15 + x - kw // 2:15 + x + kw // 2 + 1] = element
        assert np.array_equal(both_px(px, R.DILATE, el, R.BORDER_ZERO)[0], want[15:15 + h, 15:15 + w]), (name, y, x)
        assert np.array_equal(want[15:15 + h, 15:15 + w], ndimage.binary_dilation(px, element))
        want[:] = False
        want[15 + y - kh // 2:15 + y + kh // 2 + 1, 15 + x - kw // 2:15 + x + kw // 2 + 1] = element[::-1, ::-1]
        assert np.array_equal(both_px(~px, R.ERODE, el, R.BORDER_ONE)[0], ~want[15:15 + h, 15:15 + w]), (name, y, x)


@pytest.mark.parametrize("name", NAMES)
def test_the_erosion_of_an_all_ones_map(name):
    el = ELEMENTS[name]
    a = R.element_array(*el)
    ys, xs = np.nonzero(a)
    dy0, dy1, dx0, dx1 = ys.min() - el[2] // 2, ys.max() - el[2] // 2, xs.min() - el[1] // 2, xs.max() - el[1] // 2
    h, w = 40, 43
    ones = np.ones((h, w), bool)
    assert both_px(ones, R.ERODE, el, R.BORDER_ONE)[0].all()
    want = np.zeros((h, w), bool)                                   # the frame shrunk by the element's extents
    want[max(0, -dy0):h - max(0, dy1), max(0, -dx0):w - max(0, dx1)] = True
    assert np.array_equal(both_px(ones, R.ERODE, el, R.BORDER_ZERO)[0], want)


def test_the_shapes_typed_out():
    bits = lambda *rows: [int(r[::-1], 2) for r in rows]            # typed left to right: column 0 first
    assert capi.morph_element(capi.MORPH_ELLIPSE, 5, 5).tolist() == bits("00100", "01110", "11111", "01110", "00100")
    assert capi.morph_element(capi.MORPH_ELLIPSE, 3, 3).tolist() == capi.morph_element(capi.MORPH_CROSS, 3, 3).tolist() == \
        bits("010", "111", "010")
    assert capi.morph_element(capi.MORPH_RECT, 3, 5).tolist() == bits("111", "111", "111", "111", "111")
    assert capi.morph_element(capi.MORPH_CROSS, 3, 5).tolist() == bits("010", "010", "111", "010", "010")
    assert capi.morph_element(capi.MORPH_ELLIPSE, 7, 7).tolist() == bits("0001000", "0111110", "0111110", "1111111", "0111110",
                                                                         "0111110", "0001000")   # skimage.morphology.disk(3)
    assert capi.morph_element(capi.MORPH_ELLIPSE, 1, 9).tolist() == [1] * 9 and capi.morph_element(capi.MORPH_ELLIPSE, 9, 1).tolist() == [511]
    for shape in (R.RECT, R.CROSS, R.ELLIPSE):
        for kw in range(1, 32, 2):
            for kh in (1, 3, 9, kw, 31):
                assert capi.morph_element(shape, kw, kh).tolist() == R.element(shape, kw, kh), (shape, kw, kh)
    for r in range(1, 16):                                          # the disk: dx^2 + dy^2 <= r^2
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        assert np.array_equal(R.element_array(capi.morph_element(capi.MORPH_ELLIPSE, 2 * r + 1).tolist(), 2 * r + 1, 2 * r + 1),
                              xx * xx + yy * yy <= r * r)
    for shape, kw, kh in ((3, 3, 3), (-1, 3, 3), (0, 2, 3), (0, 3, 4), (0, 33, 3), (0, 3, 0)):
        rows = np.full(40, 0x5A5A5A5A, np.uint32)
        assert capi.load().canny_hip_morph_element(shape, kw, kh, capi._hp(rows)) == 1 and (rows == 0x5A5A5A5A).all()
    assert capi.load().canny_hip_morph_element(0, 3, 3, None) == 1


# ---- properties, for random and asymmetric elements ---------------------------------------------------------------------
def test_the_algebra_of_openings_and_closings():
    rng = np.random.default_rng(34)
    elements = [ELEMENTS[n] for n in ("L", "ring3x3", "far_bit", "alternating31", "random31_1")] + [random_element(rng, 15) for _ in range(25)]
    for k, el in enumerate(elements):
        h, w = int(rng.integers(1, 50)), int(rng.integers(1, 80))
        x = rng.random((2, h, w)) < (0.2, 0.5, 0.8)[k % 3]
        it = 1 + k % 2
        opened, closed = both_px(x, R.OPEN, el, iterations=it), both_px(x, R.CLOSE, el, iterations=it)
        assert np.array_equal(both_px(opened, R.OPEN, el, iterations=it), opened) and not (opened & ~x).any(), k
        assert np.array_equal(both_px(closed, R.CLOSE, el, iterations=it), closed) and not (x & ~closed).any(), k
        rows, kw, kh = el
        eroded, dilated = both_px(x, R.ERODE, el, iterations=it), both_px(x, R.DILATE, el, iterations=it)
        assert np.array_equal(~eroded, both_px(~x, R.DILATE, (R.reflect(rows, kw, kh), kw, kh), iterations=it)), k
        for border in R.BORDERS:
            e, d = both_px(x, R.ERODE, el, border, it), both_px(x, R.DILATE, el, border, it)
            o, c = both_px(x, R.OPEN, el, border, it), both_px(x, R.CLOSE, el, border, it)
            assert np.array_equal(o, both_px(e, R.DILATE, el, border, it)) and np.array_equal(c, both_px(d, R.ERODE, el, border, it))
            assert np.array_equal(both_px(x, R.GRADIENT, el, border, it), d & ~e)
            assert np.array_equal(both_px(x, R.TOPHAT, el, border, it), x & ~o)
            assert np.array_equal(both_px(x, R.BLACKHAT, el, border, it), c & ~x)


# ---- border and iterations ------------------------------------------------------------------------------------------------
def test_input_pad_bits_change_nothing_and_output_pad_bits_are_zero():
    rng = np.random.default_rng(8)
    for k, w in enumerate((1, 7, 9, 31, 33, 65, 127)):
        px = rng.random((2, 19, w)) < 0.3
        px[..., -3:] = False                                         # a set pad column would show at once in a dilation
        clean, dirty, noisy = R.pack(px), R.pack_dirty(px), R.pack_dirty(px, rng)
        assert not np.array_equal(clean, dirty)
        for op in R.OPS:
            for border in R.BORDERS:
                el = ELEMENTS[("rect3x3", "rect31x1", "L", "ellipse7x7")[(k + op) % 4]]
                a = both(clean, w, op, el, border, 1 + op % 2)
                for other in (dirty, noisy):
                    b = both(other, w, op, el, border, 1 + op % 2)
                    assert np.array_equal(a[0], b[0]) and a[1].tolist() == b[1].tolist(), (w, op, border)
                assert not (a[0][..., -1] & (0xFF >> (w % 8))).any()
    # the pad column just right of the frame set, BORDER_ZERO, DILATE: nothing may leak in
    px = np.zeros((1, 5, 13), bool)
    out, counts = both(R.pack_dirty(px), 13, R.DILATE, ELEMENTS["rect3x3"], R.BORDER_ZERO)
    assert not out.any() and counts.tolist() == [0]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 15])
def test_k_iterations_of_rect3_are_one_step_of_the_wider_rectangle(k):
    rng = np.random.default_rng(k)
    px = rng.random((2, 41, 77)) < 0.5
    sparse = rng.random((2, 41, 77)) < 0.002
    wide = (R.element(R.RECT, 2 * k + 1, 2 * k + 1), 2 * k + 1, 2 * k + 1)
    for x in (px, sparse, ~sparse):
        for op in (R.ERODE, R.DILATE, R.OPEN, R.CLOSE):
            assert np.array_equal(both_px(x, op, ELEMENTS["rect3x3"], iterations=k), both_px(x, op, wide)), (k, op)


# ---- the use case ---------------------------------------------------------------------------------------------------------
def test_opening_the_change_masks_of_the_moving_object_returns_the_patch():
    bg, frames, patch = fr.moving_object()
    h, w = bg.shape
    fused, count = fr.fuse(frames, None, 3, 3, fr.MEDIAN, 0, 1)
    mask, changed = fr.change_mask(frames, None, fused, count, 3, 49, 3)
    assert np.array_equal(R.unpack(mask, w), patch)
    noisy = R.unpack(mask, w).copy()
    rng = np.random.default_rng(12)
    added = 0
    for f in range(3):
        for _ in range(30):
            y, x, two = int(rng.integers(0, h)), int(rng.integers(0, w - 1)), bool(rng.integers(0, 2))
            if noisy[f, max(y - 4, 0):y + 5, max(x - 4, 0):x + 6].any():
                continue                                             # at least 3 pixels from the patch and from other noise
            noisy[f, y, x:x + 1 + two] = True
            added += 1 + two
    assert added > 40
    noisy_bits = R.pack(noisy)
    assert noisy_bits.sum() != mask.sum()
    opened, counts = both(noisy_bits, w, R.OPEN, ELEMENTS["rect3x3"])
    assert np.array_equal(R.unpack(opened, w), patch) and counts.tolist() == [54, 54, 54]
    for f in range(3):
        assert capi.components_from_bits(noisy_bits[f], h, w)[2] > 10
        labels, stats, n = capi.components_from_bits(opened[f], h, w)
        assert n == 1 and stats[0][4] == 54 and np.array_equal(labels != 0, patch[f])


# ---- refused calls --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_sentinels_untouched():
    L = capi.load()
    n, h, w, rb = 2, 6, 9, 2
    bits = R.pack(np.random.default_rng(3).random((n, h, w)) < 0.5)
    vp = capi.C.c_void_p

    def morph(src=1, n=n, h=h, w=w, op=R.OPEN, rows=(7, 7, 7), kw=3, kh=3, border=2, it=1, out=1, counts=1, off=0):
        o, c = np.full(n_out + 8, 0x5A, np.uint8), np.full(4, 0x5A5A5A5A5A5A5A5A, np.int64)
        r = np.array(rows, np.uint32) if rows is not None else None
        st = L.canny_hip_morph_bits(capi._hp(bits) if src else None, n, h, w, op, capi._hp(r) if r is not None else None, kw, kh,
                                    border, it, capi._hp(o) if out else None, vp(c.ctypes.data + off) if counts else None)
        if st:
            assert (o == 0x5A).all() and (c == 0x5A5A5A5A5A5A5A5A).all(), "a refused call wrote something"
        else:
            assert (o[n_out:] == 0x5A).all() and (c[2:] == 0x5A5A5A5A5A5A5A5A).all() and (counts or (c == 0x5A5A5A5A5A5A5A5A).all())
        return st

    n_out = n * h * rb
    assert morph() == 0 and morph(counts=0) == 0 and morph(it=16, op=R.BLACKHAT, border=0) == 0 and morph(rows=(5, 0, 2)) == 0
    for kw in (dict(src=0), dict(out=0), dict(rows=None), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(op=-1), dict(op=7),
               dict(border=-1), dict(border=3), dict(it=0), dict(it=17), dict(it=-1), dict(rows=(7, 8, 7)), dict(rows=(7, 7, 1 << 31)),
               dict(rows=(0, 0, 0)), dict(kw=2), dict(kw=4, rows=(15, 15, 15)), dict(kh=2), dict(kw=33), dict(kh=33, rows=(1,) * 33),
               dict(kw=0), dict(kh=0), dict(kw=-3), dict(off=4), dict(off=1)):
        assert morph(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert morph(**kw) == 2, kw
    # an output that overlaps the input or the counts: there is no in-place form
    buf = np.full(400, 0x5A, np.uint8)
    at = lambda o: vp(buf.ctypes.data + o)
    rows = np.array([7, 7, 7], np.uint32)
    for i_at, o_at, c_at in ((0, 0, 200), (0, 23, 200), (10, 0, 200), (0, 100, 16), (0, 100, 120), (0, 100, 96)):   # maps 24 B, counts 16 B
        st = L.canny_hip_morph_bits(at(i_at), n, h, w, R.OPEN, capi._hp(rows), 3, 3, 2, 1, at(o_at), at(c_at))
        assert st == 1 and (buf == 0x5A).all(), (i_at, o_at, c_at)
    assert L.canny_hip_morph_bits(at(0), n, h, w, R.OPEN, capi._hp(rows), 3, 3, 2, 1, at(24), at(48)) == 0 and (buf[64:] == 0x5A).all()


# ---- header and bindings --------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2400
    assert capi.load().canny_hip_version() >= 2400
    for word in ("0.24.0: + binary morphology on packed bit maps", "THE PAD BITS OF THE INPUT ARE IGNORED",
                 "THE PAD BITS OF THE OUTPUT ARE WRITTEN 0", "(i - kw / 2, j - kh / 2)", "AND over b in B of in(p + b)",
                 "OR  over b in B of in(p - b)", "CANNY_HIP_MORPH_BORDER_NEUTRAL = 2", "DILATE & ~ERODE", "in & ~OPEN", "CLOSE & ~in",
                 "dx^2 ry^2 + dy^2 rx^2 <= rx^2 ry^2", "\"morph_route\"", "CANNY_HIP_MORPH_MAX_EXTENT %d" % capi.MORPH_MAX_EXTENT,
                 "CANNY_HIP_MORPH_MAX_ITERATIONS %d" % capi.MORPH_MAX_ITERATIONS, "hit-or-miss", "no in-place form"):
        assert word in header, word
    for name in ("canny_hip_dev_morph_bits", "canny_hip_dev_canny_morph", "canny_hip_canny_morph", "canny_hip_morph_bits",
                 "canny_hip_morph_element", "canny_hip_selftest_morph_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    for method in ("dev_morph_bits", "dev_canny_morph", "canny_morph"):
        assert hasattr(capi.Context, method), method
    assert (capi.MORPH_ERODE, capi.MORPH_DILATE, capi.MORPH_OPEN, capi.MORPH_CLOSE, capi.MORPH_GRADIENT, capi.MORPH_TOPHAT,
            capi.MORPH_BLACKHAT) == R.OPS
    assert (capi.MORPH_RECT, capi.MORPH_CROSS, capi.MORPH_ELLIPSE) == (R.RECT, R.CROSS, R.ELLIPSE)
    assert (capi.MORPH_BORDER_ZERO, capi.MORPH_BORDER_ONE, capi.MORPH_BORDER_NEUTRAL) == R.BORDERS
    for i, op in enumerate(("ERODE", "DILATE", "OPEN", "CLOSE", "GRADIENT", "TOPHAT", "BLACKHAT")):
        assert re.search(rf"CANNY_HIP_MORPH_{op} = {i}\b", header), op


# ---- the host rule under the host compiler's sanitizers -------------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_morph_host.cpp has its own main and is compiled together with csrc/canny_morph_host.cpp alone: nothing of
    it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_morph_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_morph_host.cpp"),
                           os.path.join(csrc, "canny_morph_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "morph ok" in r.stdout, r.stdout + r.stderr
