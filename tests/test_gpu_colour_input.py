"""Colour frame input on the GPU (canny_hip_*_color, canny_hip_*to_gray): the standalone conversion against numpy over
every (R,G,B) triple, the fused Gaussian against the two-pass form byte for byte, and every colour entry point against
the oracle on the converted plane (oracle.canny(gray(frame)))."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {0: (1868, 9617, 4899, 14), 1: (7471, 38470, 19595, 16)}  # (wb, wg, wr, shift): OpenCV, PIL
COLOUR = (capi.LAYOUT_BGR8, capi.LAYOUT_RGB8, capi.LAYOUT_BGRA8, capi.LAYOUT_RGBA8)
BGR_ORDER = (capi.LAYOUT_BGR8, capi.LAYOUT_BGRA8)
# sigma -> window 1 + 2 ceil(3 sigma): 3, 5, 7, 9 (fused), 11, 13, 15, 17 (marching, not fused)
SIGMA_OF_WINDOW = {3: 0.3, 5: 0.6, 7: 1.0, 9: 1.2, 11: 1.4, 13: 1.8, 15: 2.2, 17: 2.5}
FUSED_WINDOWS = (3, 5, 7, 9)


def gray_ref(rgb, rule):
    wb, wg, wr, s = RULES[rule]
    c = np.asarray(rgb).astype(np.uint32)
    return ((wb * c[..., 2] + wg * c[..., 1] + wr * c[..., 0] + (1 << (s - 1))) >> s).astype(np.uint8)


def interleave(rgb, layout, seed=0):
    """(..., 3) R,G,B -> the bytes of `layout` (alpha random: it must be ignored)."""
    ch = capi.LAYOUT_CHANNELS[layout]
    out = np.empty(rgb.shape[:-1] + (ch,), np.uint8)
    out[..., :3] = rgb[..., ::-1] if layout in BGR_ORDER else rgb
    if ch == 4:
        out[..., 3] = np.random.default_rng(seed).integers(0, 256, rgb.shape[:-1], dtype=np.uint8)
    return out


def colour_frame(h, w, seed=0):
    """A natural-looking R,G,B frame: three synthetic gray frames as channels."""
    return np.stack([synth_frame(h, w, seed * 3 + k) for k in range(3)], axis=-1)


@pytest.fixture(scope="module")
def ctx(hip):
    with capi.Context(0) as c:
        yield c


@pytest.fixture
def rule_ctx(ctx):
    """The module context, its colour options restored after each test."""
    yield ctx
    ctx.set_option("gray_rule", 0)
    ctx.set_option("fuse_gray", 1)


class Dev:
    """Device buffers of one test, freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 1))
        self.ptrs.append(p)
        return p

    def up(self, a, pad=0):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes + pad)
        self.ctx.h2d(p + pad, a)
        return p + pad

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.synchronize()
        self.ctx.d2h(out, p)
        return out

    def free(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.free(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free()


@pytest.fixture(scope="module")
def all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.empty((1 << 24, 3), np.uint8)
    rgb[:, 0], rgb[:, 1], rgb[:, 2] = v >> 16, (v >> 8) & 0xFF, v & 0xFF
    return rgb.reshape(4096, 4096, 3)


# ---- 1. exhaustive conversion ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("layout", COLOUR)
def test_to_gray_every_triple(rule_ctx, dev, all_triples, layout, rule):
    rule_ctx.set_option("gray_rule", rule)
    src = interleave(all_triples, layout, seed=layout)
    want = gray_ref(all_triples, rule)
    d_src, d_gray = dev.up(src), dev.alloc(1 << 24)
    for h, w, n in ((4096, 4096, 1), (2048, 4096, 2)):  # one frame, and two frames (crossing a frame boundary)
        rule_ctx.dev_to_gray(d_src, layout, h, w, n, d_gray)
        got = dev.down(d_gray, (4096, 4096), np.uint8)
        assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ ({n} frames)"


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", COLOUR)
def test_to_gray_unaligned_source_and_tail(rule_ctx, dev, layout, offset):
    h, w = 7, 1001  # 7007 pixels: 437 groups of 16 and a tail of 15
    rgb = np.random.default_rng(offset).integers(0, 256, (h, w, 3), dtype=np.uint8)
    d_src = dev.up(interleave(rgb, layout), pad=offset)
    d_gray = dev.alloc(h * w + 64)
    guard = np.full(h * w + 64, 0xA5, np.uint8)
    rule_ctx.h2d(d_gray, guard)
    rule_ctx.dev_to_gray(d_src, layout, h, w, 1, d_gray)
    got = dev.down(d_gray, (h * w + 64,), np.uint8)
    assert np.array_equal(got[:h * w].reshape(h, w), gray_ref(rgb, 0))
    assert (got[h * w:] == 0xA5).all(), "wrote past the plane"
    assert np.array_equal(rule_ctx.to_gray(interleave(rgb, layout), "bgr" if layout in BGR_ORDER else "rgb"),
                          gray_ref(rgb, 0))


# ---- 2. fused Gaussian plane -----------------------------------------------------------------------------------------
def _fused_vs_two_pass(ctx, dev, rgb, layout, sigma, n=1):
    h, w = rgb.shape[-3:-1]
    d_src = dev.up(interleave(rgb, layout))
    d_gray, d_a, d_b = dev.alloc(n * h * w), dev.alloc(n * h * w), dev.alloc(n * h * w)
    ctx.dev_to_gray(d_src, layout, h, w, n, d_gray)
    ctx.dev_gaussian_u8(d_gray, sigma, h, w, n, d_b)
    ctx.dev_gaussian_u8_color(d_src, layout, sigma, h, w, n, d_a)
    a, b = dev.down(d_a, (n * h * w,), np.uint8), dev.down(d_b, (n * h * w,), np.uint8)
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} smoothed pixels differ"


@pytest.mark.parametrize("window", FUSED_WINDOWS)
@pytest.mark.parametrize("layout", COLOUR)
def test_fused_gaussian_every_window(rule_ctx, dev, window, layout):
    for rule in (0, 1):
        rule_ctx.set_option("gray_rule", rule)
        _fused_vs_two_pass(rule_ctx, dev, colour_frame(67, 1031, window), layout, SIGMA_OF_WINDOW[window])


@pytest.mark.parametrize("window", [11, 13, 15, 17])
def test_fused_gaussian_unsupported_beyond_window_9(ctx, dev, window):
    rgb = colour_frame(64, 256)
    d_src, d_out = dev.up(interleave(rgb, capi.LAYOUT_BGR8)), dev.alloc(64 * 256)
    with pytest.raises(capi.CannyHipError) as ei:
        ctx.dev_gaussian_u8_color(d_src, capi.LAYOUT_BGR8, SIGMA_OF_WINDOW[window], 64, 256, 1, d_out)
    assert ei.value.status == 2  # CANNY_HIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("width", range(4, 14))  # 3W mod 4 takes every residue
def test_fused_gaussian_narrow_widths(rule_ctx, dev, width):
    for window in FUSED_WINDOWS:
        for layout in COLOUR:
            _fused_vs_two_pass(rule_ctx, dev, colour_frame(37, width, width), layout, SIGMA_OF_WINDOW[window], n=1)
    _fused_vs_two_pass(rule_ctx, dev, np.stack([colour_frame(19, width, s) for s in range(3)]), capi.LAYOUT_RGB8, 1.0,
                       n=3)


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
@pytest.mark.parametrize("rule", [0, 1])
def test_fused_gaussian_large_frames(rule_ctx, dev, h, w, rule):
    rule_ctx.set_option("gray_rule", rule)
    for layout in COLOUR:
        for window in (3, 9):
            _fused_vs_two_pass(rule_ctx, dev, colour_frame(h, w, layout), layout, SIGMA_OF_WINDOW[window])


def test_fused_gaussian_exhaustive_pattern(rule_ctx, dev, all_triples):
    for layout in (capi.LAYOUT_BGR8, capi.LAYOUT_RGBA8):
        _fused_vs_two_pass(rule_ctx, dev, all_triples, layout, 1.0)


# ---- 3. pipeline parity ----------------------------------------------------------------------------------------------
THRESHOLDS = [(50, 150), (1, 1), (100, 50), (0, 100), (255, 256)]


def _gray_canny_or_status(ctx, g, sigma, lo, hi):
    try:
        return ctx.canny(g, sigma, lo, hi), 0
    except capi.CannyHipError as e:
        return None, e.status


@pytest.mark.parametrize("lo,hi", THRESHOLDS)
@pytest.mark.parametrize("h,w", [(480, 640), (1080, 1024)])
def test_canny_color_matches_oracle(ctx, dev, h, w, lo, hi):
    rgb = colour_frame(h, w, 7)
    g = gray_ref(rgb, 0)
    want, status = _gray_canny_or_status(ctx, g, 1.0, lo, hi)
    for layout in COLOUR:
        src = interleave(rgb, layout)
        order = "bgr" if layout in BGR_ORDER else "rgb"
        d_src, d_out = dev.up(src), dev.alloc(h * w * 2)
        if status:
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.canny_color(src, 1.0, lo, hi, order)
            assert ei.value.status == status
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_canny_color(d_src, layout, 1.0, lo, hi, h, w, 1, d_out)
            assert ei.value.status == status
            continue
        assert np.array_equal(want, oracle.canny(g, 1.0, lo, hi))
        assert np.array_equal(ctx.canny_color(src, 1.0, lo, hi, order), want)
        ctx.dev_canny_color(d_src, layout, 1.0, lo, hi, h, w, 1, d_out)
        assert np.array_equal(dev.down(d_out, (h, w), np.int16), want)


# ---- 4. path selection -----------------------------------------------------------------------------------------------
def _fused_flag(ctx, dev, rgb, sigma, n=1):
    h, w = rgb.shape[-3:-1]
    d_src, d_out = dev.up(interleave(rgb, capi.LAYOUT_BGR8)), dev.alloc(n * h * w * 2)
    ctx.dev_canny_color(d_src, capi.LAYOUT_BGR8, sigma, 50, 150, h, w, n, d_out)
    got = dev.down(d_out, (n * h * w,), np.int16)
    return ctx.get_option("last_canny_fused_gray"), got


def test_fuse_gray_on_and_off_give_the_same_maps(rule_ctx, dev):
    rgb = colour_frame(2160, 3840, 3)
    for sigma in (0.6, 1.0, 1.2, 1.4):
        rule_ctx.set_option("fuse_gray", 1)
        f1, a = _fused_flag(rule_ctx, dev, rgb, sigma)
        rule_ctx.set_option("fuse_gray", 0)
        f0, b = _fused_flag(rule_ctx, dev, rgb, sigma)
        assert f0 == 0 and np.array_equal(a, b), sigma
        assert f1 == (1 if sigma <= 1.2 else 0), sigma


@pytest.mark.parametrize("case", ["sigma4", "width3", "gaussian_path1", "smoothed_u8_0", "fuse_classify_0"])
def test_fallback_paths_are_not_fused_and_match(ctx, dev, case):
    sigma, h, w, opt = 1.0, 64, 256, None
    if case == "sigma4":
        sigma = 4.0
    elif case == "width3":
        w = 3
    else:
        opt = {"gaussian_path1": ("gaussian_path", 1), "smoothed_u8_0": ("smoothed_u8", 0),
               "fuse_classify_0": ("fuse_classify", 0)}[case]
    rgb = colour_frame(h, w, 5)
    try:
        if opt:
            ctx.set_option(*opt)
        flag, got = _fused_flag(ctx, dev, rgb, sigma)
        want = ctx.canny(gray_ref(rgb, 0), sigma, 50, 150)
    finally:
        if opt:
            ctx.set_option(opt[0], {"gaussian_path": 0, "smoothed_u8": 1, "fuse_classify": 1}[opt[0]])
    assert flag == 0
    assert np.array_equal(got.reshape(h, w), want)


def test_fused_flag_set_on_a_fusable_4k_frame(ctx, dev):
    flag, got = _fused_flag(ctx, dev, colour_frame(2160, 3840, 4), 1.0)
    assert flag == 1


# ---- 5. channel order ------------------------------------------------------------------------------------------------
def test_channel_order_matters(ctx):
    h, w = 480, 640
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[..., 0] = synth_frame(h, w, 11)  # edges in R only
    frame = np.ascontiguousarray(rgb)
    as_bgr = ctx.canny_color(frame, 1.0, 20, 60, "bgr")  # bytes read as B,G,R: the R plane is taken for B
    as_rgb = ctx.canny_color(frame, 1.0, 20, 60, "rgb")
    assert np.array_equal(as_rgb, oracle.canny(gray_ref(rgb, 0), 1.0, 20, 60))
    assert np.array_equal(as_bgr, oracle.canny(gray_ref(rgb[..., ::-1], 0), 1.0, 20, 60))
    assert not np.array_equal(as_bgr, as_rgb)


# ---- 6. batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("layout", [capi.LAYOUT_BGR8, capi.LAYOUT_RGBA8])
def test_batch_color_formats(ctx, layout, pinned):
    n, h, w = 10, 270, 480
    frames = np.stack([interleave(colour_frame(h, w, s), layout, s) for s in range(n)])
    if pinned:
        buf = ctx.pinned_array(frames.shape, np.uint8)
        buf[...] = frames
        frames = buf
    order = "bgr" if layout in BGR_ORDER else "rgb"
    want = np.stack([ctx.canny_color(f, 1.4, 50, 150, order) for f in frames])
    ctx.set_option("tune_batch_chunk_frames", 3)
    try:
        s16 = ctx.canny_batch_color(frames, 1.4, 50, 150, order, fmt="s16")
        u8 = ctx.canny_batch_color(frames, 1.4, 50, 150, order, fmt="u8")
        bits = ctx.canny_batch_color(frames, 1.4, 50, 150, order, fmt="bits")
    finally:
        ctx.set_option("tune_batch_chunk_frames", 0)
    assert np.array_equal(s16, want)
    assert np.array_equal(u8, (want != 0).astype(np.uint8) * 255)
    assert np.array_equal(capi.unpack_bits(bits, w), want)


def test_batch_color_64_frames_1080p(ctx):
    n, h, w = 64, 1080, 1920
    base = [interleave(colour_frame(h, w, s), capi.LAYOUT_BGR8) for s in range(4)]
    frames = np.stack([base[i % 4] for i in range(n)])
    want = [oracle.canny(gray_ref(b[..., ::-1], 0), 1.0, 50, 150) for b in base]
    got = ctx.canny_batch_color(frames, 1.0, 50, 150, "bgr", fmt="u8")
    for i in range(n):
        assert np.array_equal(got[i], (want[i % 4] != 0).astype(np.uint8) * 255), i


# ---- 7. identity -----------------------------------------------------------------------------------------------------
def test_gray8_is_the_identity_everywhere(ctx, dev):
    h, w = 270, 480
    g = synth_frame(h, w, 9)
    assert np.array_equal(ctx.to_gray(g), g)
    assert np.array_equal(ctx.canny_color(g, 1.4, 50, 150), ctx.canny(g, 1.4, 50, 150))
    frames = np.stack([g, synth_frame(h, w, 10)])
    assert np.array_equal(ctx.canny_batch_color(frames, 1.4, 50, 150, fmt="bits"),
                          ctx.canny_batch(frames, 1.4, 50, 150, bits=True))
    d_g, d_a, d_b = dev.up(g), dev.alloc(h * w * 2), dev.alloc(h * w * 2)
    ctx.dev_to_gray(d_g, capi.LAYOUT_GRAY8, h, w, 1, d_a)
    assert np.array_equal(dev.down(d_a, (h, w), np.uint8), g)
    ctx.dev_gaussian_u8_color(d_g, capi.LAYOUT_GRAY8, 1.4, h, w, 1, d_a)
    ctx.dev_gaussian_u8(d_g, 1.4, h, w, 1, d_b)
    assert np.array_equal(dev.down(d_a, (h, w), np.uint8), dev.down(d_b, (h, w), np.uint8))
    ctx.dev_canny_color(d_g, capi.LAYOUT_GRAY8, 1.4, 50, 150, h, w, 1, d_a)
    ctx.dev_canny(d_g, 1.4, 50, 150, h, w, 1, d_b)
    assert np.array_equal(dev.down(d_a, (h, w), np.int16), dev.down(d_b, (h, w), np.int16))


# ---- 8. errors -------------------------------------------------------------------------------------------------------
def test_errors(ctx, dev):
    L, h = ctx._L, ctx._h
    import ctypes as C
    src = np.zeros((16, 16, 3), np.uint8)
    out = np.zeros((16, 16), np.int16)
    d = dev.alloc(4096)
    p = src.ctypes.data_as(C.c_void_p)
    o = out.ctypes.data_as(C.c_void_p)
    for bad in (-1, 5, 99):
        assert L.canny_hip_to_gray(h, p, bad, 16, 16, o) == 1
        assert L.canny_hip_canny_color(h, p, bad, 1.0, 50, 150, 16, 16, o) == 1
        assert L.canny_hip_canny_batch_color(h, p, bad, 1, 1.0, 50, 150, 16, 16, o) == 1
        assert L.canny_hip_dev_to_gray(h, C.c_void_p(d), bad, 16, 16, 1, C.c_void_p(d + 2048)) == 1
        assert L.canny_hip_dev_canny_color(h, C.c_void_p(d), bad, 1.0, 50, 150, 16, 16, 1, C.c_void_p(d + 2048)) == 1
    assert L.canny_hip_to_gray(h, None, capi.LAYOUT_BGR8, 16, 16, o) == 1
    assert L.canny_hip_canny_color(h, p, capi.LAYOUT_BGR8, 1.0, 50, 150, 16, 16, None) == 1
    assert L.canny_hip_dev_gaussian_u8_color(h, None, capi.LAYOUT_BGR8, 1.0, 16, 16, 1, C.c_void_p(d)) == 1
    assert L.canny_hip_canny_batch_color_bits(h, p, capi.LAYOUT_BGR8, 0, 1.0, 50, 150, 16, 16, o) == 1
    assert L.canny_hip_to_gray(h, p, capi.LAYOUT_BGR8, 0, 16, o) == 1
    assert L.canny_hip_dev_to_gray(h, C.c_void_p(d), capi.LAYOUT_RGB8, 16, -1, 1, C.c_void_p(d)) == 1
    assert L.canny_hip_dev_canny_color(h, C.c_void_p(d), capi.LAYOUT_BGR8, 1.0, 50, 150, 1, 16, 1, C.c_void_p(d + 2048)) == 2
    assert L.canny_hip_canny_color(h, p, capi.LAYOUT_BGR8, 0.0, 50, 150, 16, 16, o) == 1  # bad sigma, like canny()
    assert L.canny_hip_ctx_set_option(h, b"gray_rule", 2) == 1
    assert L.canny_hip_ctx_set_option(h, b"fuse_gray", 2) == 1
    assert L.canny_hip_ctx_set_option(h, b"last_canny_fused_gray", 1) == 1  # read-only


# ---- 9. CLI ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuda", [False, True])
def test_cli_reads_ppm(tmp_path, cuda):
    h, w = 240, 320
    rgb = colour_frame(h, w, 21)
    ppm = tmp_path / "f.ppm"
    ppm.write_bytes(b"P6\n# colour frame\n%d %d\n255\n" % (w, h) + rgb.tobytes())
    out = tmp_path / "d"
    out.mkdir()
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    args = [exe, "1.4", "50", "150", "-i", str(ppm), "-o", str(out), "-s"] + (["-c"] if cuda else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = gray_ref(rgb, 0)
    step0 = _read_pgm(out / "canny_step0_gray.pgm")
    assert np.array_equal(step0, g)
    edges = sorted(p for p in os.listdir(out) if p.endswith(".pgm") and "edge" in p)
    assert edges, os.listdir(out)
    got = _read_pgm(out / edges[-1])
    assert np.array_equal(got.astype(np.int16), oracle.canny(g, 1.4, 50, 150))


def _read_pgm(path):
    data = open(path, "rb").read()
    parts, pos = [], 0
    while len(parts) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos)
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        parts.append(data[pos:end])
        pos = end
    pos += 1
    w, h = int(parts[1]), int(parts[2])
    return np.frombuffer(data[pos:pos + w * h], np.uint8).reshape(h, w)
