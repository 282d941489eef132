"""The marching Gaussian's quotient form is chosen per pass: a wave at a frame's border divides by the full-window
weight with the one-instruction fma wherever that weight applies (the column pass of a border strip, the row pass
and the full-weight rows of a wave at a frame's top or bottom) and keeps the five-instruction division for per-lane
column weights and for the first and last C rows.  Every branch of that choice is compared with the oracle bit for
bit, on both output planes and on the colour entry point, and so is a launch whose segment length comes from the
whole-round search.

Shapes (strips are 244 columns wide at window 11, sigma 1.4; other windows have other strip widths, so the same
widths give them other mixes of border and interior strips):
  widths   8 = one strip, border on both sides; 244, 484 = border strips only; 724, 964 = one and two interior strips
  heights  7, 12 = every row renormalises (H < 2C+1 and just above); 40 = border rows and full-weight rows in one wave;
           300 with 67-row segments = top, interior and bottom segments are separate waves
Sigmas: 1.4, 1.0 and 2.0 sum (ascending float adds, as the launcher sums) to 1 + 2^-23, 1 and 1 + 2^-23, all in the
one-instruction table; 1.9362 (window 13) sums to 0x3f7ffffb = 1 - 5 * 2^-24, which is not, so the launcher's table
look-up misses and every wave keeps the long division.  Sigma 1.4 also runs with the switch "gaussian_fma_div" off."""
import numpy as np
import pytest

import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

WIDTHS = (8, 244, 484, 724, 964)
HEIGHTS = ((7, 0), (12, 0), (40, 0), (300, 67))  # (height, "tune_gaussian_seg")
# windows 11, 7, 13 and 13: full-window weights 1 + 2^-23, 1, 1 + 2^-23 and 1 - 5 * 2^-24 (not in the fma table)
SIGMAS = (1.4, 1.0, 2.0, 1.9362)
N = 2


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.Context(0) as c:
        yield c
        c.set_option("tune_gaussian_seg", 0)
        c.set_option("gaussian_fma_div", 1)


@pytest.fixture(scope="module")
def frames():
    """(h, w) -> N frames; made once."""
    return {(h, w): np.stack([synth_frame(h, w, 11 * h + w + i) for i in range(N)])
            for h, _ in HEIGHTS for w in WIDTHS}


@pytest.fixture(scope="module")
def smoothed(frames):
    """(h, w, sigma) -> the oracle's planes; computed once, shared by the tests below."""
    return {(h, w, s): np.stack([oracle.gaussian(f, s) for f in fr]) for (h, w), fr in frames.items() for s in SIGMAS}


def _both_planes(c, fr, sigma):
    n, h, w = fr.shape
    d_in, d_16, d_8 = c.malloc(fr.nbytes), c.malloc(fr.nbytes * 2), c.malloc(fr.nbytes)
    try:
        c.h2d(d_in, fr)
        c.dev_gaussian(d_in, sigma, h, w, n, d_16)
        c.dev_gaussian_u8(d_in, sigma, h, w, n, d_8)
        s16, u8 = np.empty(fr.shape, np.int16), np.empty(fr.shape, np.uint8)
        c.d2h(s16, d_16)
        c.d2h(u8, d_8)
    finally:
        for p in (d_in, d_16, d_8):
            c.free(p)
    return s16, u8


@pytest.mark.parametrize("sigma,fma_div", [(s, 1) for s in SIGMAS] + [(1.4, 0)])
def test_border_waves_equal_oracle(ctx, frames, smoothed, sigma, fma_div):
    ctx.set_option("gaussian_fma_div", fma_div)
    try:
        for h, seg in HEIGHTS:
            ctx.set_option("tune_gaussian_seg", seg)
            for w in WIDTHS:
                s16, u8 = _both_planes(ctx, frames[h, w], sigma)
                want = smoothed[h, w, sigma]
                assert np.array_equal(s16, want), (sigma, h, w, "s16", int((s16 != want).sum()))
                assert np.array_equal(u8.astype(np.int16), want), (sigma, h, w, "u8", int((u8 != want).sum()))
    finally:
        ctx.set_option("tune_gaussian_seg", 0)
        ctx.set_option("gaussian_fma_div", 1)


def test_table_miss_sigma_is_outside_the_table():
    """The weight of sigma 1.9362, summed as the launcher sums it, is in no row of the library's table."""
    taps = oracle.gaussian_kernel(1.9362)
    total = np.float32(taps[0])
    for k in taps[1:]:
        total = np.float32(total + k)
    assert len(taps) == 13 and int(total.view(np.uint32)) == 0x3F7FFFFB
    table = [np.float32(divisor) for divisor, _ in capi.fma_div_table()]
    assert len(table) >= 1 and all(d != total for d in table), table


def test_whole_round_segment_search(ctx):
    """1024 frames of 2200 x 8 fill the chip more than twice over (17408 waves at the first rule's 133-row segments,
    against 2 x 1024 SIMDs x 5 waves), so the launcher's whole-round segment search chooses the segment length; every
    wave is a border wave.  The frames repeat four distinct ones, so the oracle runs four times."""
    h, w, distinct, reps = 2200, 8, 4, 256
    base = np.stack([synth_frame(h, w, 900 + i) for i in range(distinct)])
    want = np.stack([oracle.gaussian(f, 1.4) for f in base])
    fr = np.ascontiguousarray(np.broadcast_to(base, (reps, distinct, h, w))).reshape(reps * distinct, h, w)
    ctx.set_option("tune_gaussian_seg", 0)
    ctx.set_option("gaussian_fma_div", 1)
    s16, u8 = _both_planes(ctx, fr, 1.4)
    assert np.array_equal(s16.reshape(reps, distinct, h, w), np.broadcast_to(want, (reps, distinct, h, w)))
    assert np.array_equal(u8.reshape(reps, distinct, h, w).astype(np.int16), np.broadcast_to(want, (reps, distinct, h, w)))


def test_segments_above_400_rows(ctx):
    """441-row segments (2200 rows = 5 segments: top, three interior, bottom), longer than any the search picks."""
    h, w = 2200, 724
    fr = np.stack([synth_frame(h, w, 950 + i) for i in range(N)])
    want = np.stack([oracle.gaussian(f, 1.4) for f in fr])
    ctx.set_option("tune_gaussian_seg", 441)
    try:
        s16, u8 = _both_planes(ctx, fr, 1.4)
    finally:
        ctx.set_option("tune_gaussian_seg", 0)
    assert np.array_equal(s16, want)
    assert np.array_equal(u8.astype(np.int16), want)


def _colour_case(ctx, sigma, layout, h, w):
    wb, wg, wr, shift = 1868, 9617, 4899, 14  # rule 0, OpenCV's cvtColor
    ch = capi.LAYOUT_CHANNELS[layout]
    rgb = np.stack([synth_frame(h, w, 5 * h + w + k) for k in range(3)], axis=-1)
    c32 = rgb.astype(np.uint32)
    gray = ((wb * c32[..., 2] + wg * c32[..., 1] + wr * c32[..., 0] + (1 << (shift - 1))) >> shift)
    want = oracle.gaussian(gray.astype(np.uint8), sigma)
    src = np.full((h, w, ch), 77, np.uint8)
    src[..., :3] = rgb[..., ::-1] if layout == capi.LAYOUT_BGR8 else rgb
    d_src, d_out = ctx.malloc(src.nbytes), ctx.malloc(h * w)
    try:
        ctx.h2d(d_src, src)
        ctx.dev_gaussian_u8_color(d_src, layout, sigma, h, w, 1, d_out)
        got = np.empty((h, w), np.uint8)
        ctx.d2h(got, d_out)
    finally:
        ctx.free(d_src)
        ctx.free(d_out)
    assert np.array_equal(got.astype(np.int16), want), (sigma, layout, h, w)


@pytest.mark.parametrize("layout", [capi.LAYOUT_BGR8, capi.LAYOUT_RGBA8])
@pytest.mark.parametrize("sigma", [1.0, 1.2])  # windows 7 and 9: the colour kernel shares the strip function
def test_colour_entry_point_border_waves(ctx, sigma, layout):
    ctx.set_option("gray_rule", 0)
    try:
        for h, seg in HEIGHTS:
            ctx.set_option("tune_gaussian_seg", seg)
            for w in WIDTHS:
                _colour_case(ctx, sigma, layout, h, w)
    finally:
        ctx.set_option("tune_gaussian_seg", 0)


def test_colour_entry_point_without_the_fma(ctx):
    """Switch off: the colour kernel's border waves take the general body and its interior waves the long division."""
    ctx.set_option("gray_rule", 0)
    ctx.set_option("gaussian_fma_div", 0)
    ctx.set_option("tune_gaussian_seg", 67)
    try:
        for w in (8, 964):
            _colour_case(ctx, 1.2, capi.LAYOUT_BGR8, 300, w)
    finally:
        ctx.set_option("tune_gaussian_seg", 0)
        ctx.set_option("gaussian_fma_div", 1)
