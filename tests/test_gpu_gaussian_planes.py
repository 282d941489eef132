"""The Gaussian kernels on planes whose quotients sit on integers (tests/gaussian_planes.py), bit for bit.

The division is pinned exhaustively elsewhere (test_gpu_numerics.py); this file pins what comes before it: the
separately rounded products, the ascending order of the adds and the border weights.  A one-ulp slip in any of them
changes an output pixel only where the quotient lies within one ulp of an integer, which a random image offers on
fewer than ten pixels per frame and a piecewise-constant one on tens of thousands (tests/test_gaussian_planes.py has
the counts, and shows that the oracle comparison made here fails for four such slips).

Every case sends the three flat batches (256 levels each; (24, 24), (7, 40), (40, 7)) and the four 300 x 964 mosaics
through dev_gaussian and dev_gaussian_u8 and compares both planes with the oracle.  There is no tolerance anywhere.
Where a kernel form has no u8 output (the generic kernels, the marching variants without the product table,
half-windows above 8) the test asserts that dev_gaussian_u8 refuses with CANNY_HIP_ERR_UNSUPPORTED; likewise the
colour entry point beyond window 9 (sigma 1.4), where the case then takes the route the pipeline takes: the
standalone conversion and the gray kernel.
"""
import numpy as np
import pytest

import gaussian_planes as gp
import oracle
from canny_edge_amd import capi

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 2
RULES = {0: (1868, 9617, 4899, 14), 1: (7471, 38470, 19595, 16)}  # (wb, wg, wr, shift): OpenCV, PIL
ALPHA = 77


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.Context(0) as c:
        yield c
        _defaults(c)


def _defaults(c):
    c.set_option("gaussian_path", 0)
    c.set_option("tune_gaussian_variant", 0)
    c.set_option("tune_gaussian_seg", 0)
    c.set_option("gaussian_fma_div", 1)
    c.set_option("gray_rule", 0)
    c.set_option("smoothed_u8", 1)


@pytest.fixture(scope="module")
def planes():
    return gp.designed()


class _Oracle:
    """The oracle's smoothed planes of every designed batch, computed once per sigma and left unchanged."""

    def __init__(self, planes):
        self.planes, self.cache = planes, {}

    def __call__(self, sigma):
        if sigma not in self.cache:
            self.cache[sigma] = {name: np.stack([oracle.gaussian(f, sigma) for f in batch])
                                 for name, batch in self.planes.items()}
            for a in self.cache[sigma].values():
                a.flags.writeable = False
        return self.cache[sigma]


@pytest.fixture(scope="module")
def smoothed(planes):
    return _Oracle(planes)


def _half_window(sigma):
    return len(oracle.gaussian_kernel(sigma)) // 2


def _compare(got, want, sigma, what, name):
    """Bit-exact comparison; the message names sigma, path and shape, the number of differing pixels, how many of
    them lie within the half-window of a frame border, and the first one."""
    got = got.astype(np.int16)
    if np.array_equal(got, want):
        return
    C = _half_window(sigma)
    diff = got != want
    near = int((diff & (gp.border_distance(want.shape[1:]) < C)).sum())
    f, r, c = (int(v) for v in np.argwhere(diff)[0])
    pytest.fail(f"sigma {sigma} (half-window {C}), {what}, {name} {want.shape}: {int(diff.sum())} pixels differ, {near} of "
                f"them within {C} of a frame border; first (frame, row, column, got, want) = "
                f"({f}, {r}, {c}, {int(got[f, r, c])}, {int(want[f, r, c])})")


def _run_planes(c, planes, want, sigma, what, u8_exists=True):
    """The designed batches through dev_gaussian and dev_gaussian_u8 against the oracle."""
    for name, batch in planes.items():
        n, h, w = batch.shape
        d_in, d_16, d_8 = c.malloc(batch.nbytes), c.malloc(batch.nbytes * 2), c.malloc(batch.nbytes)
        try:
            c.h2d(d_in, batch)
            c.dev_gaussian(d_in, sigma, h, w, n, d_16)
            s16 = np.empty(batch.shape, np.int16)
            c.d2h(s16, d_16)
            if u8_exists:
                c.dev_gaussian_u8(d_in, sigma, h, w, n, d_8)
                u8 = np.empty(batch.shape, np.uint8)
                c.d2h(u8, d_8)
            else:
                with pytest.raises(capi.CannyHipError) as ei:
                    c.dev_gaussian_u8(d_in, sigma, h, w, n, d_8)
                assert ei.value.status == ERR_UNSUPPORTED
        finally:
            c.synchronize()
            for p in (d_in, d_16, d_8):
                c.free(p)
        _compare(s16, want[name], sigma, what + ", s16 plane", name)
        if u8_exists:
            _compare(u8, want[name], sigma, what + ", u8 plane", name)


# ---- every kernel path ------------------------------------------------------------------------------------------------
# path 1 = generic two-pass, 2 = marching default (symmetric taps, systolic row pass, product table), 3 = LDS-ring
# kernel, 4 = symmetric taps multiplying and fetching products, 5 = product-fetching row pass with the table,
# 6 = systolic row pass that multiplies (the numbering of test_gaussian_paths); u8 output exists with the table only
PATH_NAMES = {1: "generic", 2: "march_default", 3: "march_lds_ring", 4: "march_sym_multiply", 5: "march_fetch_table",
              6: "march_systolic_multiply"}


@pytest.mark.parametrize("sigma", gp.HALF_WINDOW_SIGMAS)
@pytest.mark.parametrize("path", sorted(PATH_NAMES), ids=[PATH_NAMES[p] for p in sorted(PATH_NAMES)])
def test_every_kernel_path(ctx, planes, smoothed, path, sigma):
    ctx.set_option("gaussian_path", min(path, 2))
    ctx.set_option("tune_gaussian_variant", {3: 1, 4: 2, 5: 3, 6: 4}.get(path, 0))
    try:
        _run_planes(ctx, planes, smoothed(sigma), sigma, f"path {path} ({PATH_NAMES[path]})", u8_exists=path in (2, 5))
    finally:
        _defaults(ctx)


# ---- the default path: both quotient forms, one wave per frame column and separate top / interior / bottom waves ------
def _ascending_weight_bits(sigma):
    total = np.float32(0)
    for k in oracle.gaussian_kernel(sigma):
        total = np.float32(total + k)
    return int(total.view(np.uint32))


def test_default_path_sigmas_give_the_intended_weights():
    """Full-window weights 1, 1 + 2^-23, 1 + 2^-23, 1 - 5 * 2^-24 (in no row of the one-instruction table) and
    1 - 2^-24."""
    bits = [_ascending_weight_bits(s) for s in (1.0, 1.4, 2.0, gp.TABLE_MISS_SIGMA, 0.5)]
    assert bits == [0x3F800000, 0x3F800001, 0x3F800001, 0x3F7FFFFB, 0x3F7FFFFF], [hex(b) for b in bits]
    table = [int(np.float32(d).view(np.uint32)) for d, _ in capi.fma_div_table()]
    assert [b in table for b in bits] == [True, True, True, False, True]


@pytest.mark.parametrize("sigma", [1.0, 1.4, 2.0, gp.TABLE_MISS_SIGMA, 0.5])
@pytest.mark.parametrize("seg", [0, 67], ids=["auto_segments", "67_row_segments"])
@pytest.mark.parametrize("fma_div", [1, 0], ids=["fma_division", "long_division"])
def test_default_path(ctx, planes, smoothed, fma_div, seg, sigma):
    """With the one-instruction quotient the mosaics' waves run the four strip bodies that use it (both borders, column
    border only, row border only, interior); without it, or on the table miss, the general body and the interior
    long-division body: all five meet all 256 levels."""
    ctx.set_option("gaussian_fma_div", fma_div)
    ctx.set_option("tune_gaussian_seg", seg)
    try:
        _run_planes(ctx, planes, smoothed(sigma), sigma, f"default path, fma_div {fma_div}, seg {seg}")
    finally:
        _defaults(ctx)


# ---- generic kernels at windows wider than the cells ------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [4.0, 6.5])
def test_generic_kernels_at_large_windows(ctx, planes, smoothed, sigma):
    assert _half_window(sigma) > 8 and 2 * _half_window(sigma) + 1 > gp.CELL
    _run_planes(ctx, planes, smoothed(sigma), sigma, "automatic choice (generic kernels)", u8_exists=False)


# ---- colour entry point -----------------------------------------------------------------------------------------------
def _gray(rgb, rule):
    wb, wg, wr, s = RULES[rule]
    c = np.asarray(rgb).astype(np.uint32)
    return ((wb * c[..., 2] + wg * c[..., 1] + wr * c[..., 0] + (1 << (s - 1))) >> s).astype(np.uint8)


def _colour(batch, layout):
    """Gray planes [n, h, w] -> interleaved frames with B = G = R (and alpha 77)."""
    src = np.full(batch.shape + (capi.LAYOUT_CHANNELS[layout],), ALPHA, np.uint8)
    src[..., :3] = batch[..., None]
    return src


def test_equal_channels_give_the_level_itself():
    levels = np.arange(256, dtype=np.uint8)
    for rule in RULES:
        assert np.array_equal(_gray(np.stack([levels] * 3, -1), rule), levels), rule


@pytest.mark.parametrize("sigma", [1.0, 1.2, 1.4])
@pytest.mark.parametrize("rule", [0, 1], ids=["opencv_rule", "pil_rule"])
@pytest.mark.parametrize("layout", [capi.LAYOUT_BGR8, capi.LAYOUT_RGBA8], ids=["bgr8", "rgba8"])
def test_colour_entry_point(ctx, planes, smoothed, layout, rule, sigma):
    want = smoothed(sigma)
    fused = _half_window(sigma) <= 4  # the colour kernel exists up to window 9
    ctx.set_option("gray_rule", rule)
    try:
        for name, batch in planes.items():
            n, h, w = batch.shape
            src = _colour(batch, layout)
            d_src, d_gray, d_out = ctx.malloc(src.nbytes), ctx.malloc(batch.nbytes), ctx.malloc(batch.nbytes)
            try:
                ctx.h2d(d_src, src)
                if fused:
                    ctx.dev_gaussian_u8_color(d_src, layout, sigma, h, w, n, d_out)
                else:
                    with pytest.raises(capi.CannyHipError) as ei:
                        ctx.dev_gaussian_u8_color(d_src, layout, sigma, h, w, n, d_out)
                    assert ei.value.status == ERR_UNSUPPORTED
                    ctx.dev_to_gray(d_src, layout, h, w, n, d_gray)
                    ctx.dev_gaussian_u8(d_gray, sigma, h, w, n, d_out)
                got = np.empty(batch.shape, np.uint8)
                ctx.d2h(got, d_out)
            finally:
                ctx.synchronize()
                for p in (d_src, d_gray, d_out):
                    ctx.free(p)
            _compare(got, want[name], sigma, f"colour layout {layout}, gray_rule {rule}, "
                     f"{'fused' if fused else 'to_gray + gray kernel'}", name)
    finally:
        _defaults(ctx)


# ---- end to end -------------------------------------------------------------------------------------------------------
_edges = {}


def _oracle_canny(key, frames, sigma, lo, hi):
    if (key, sigma) not in _edges:
        _edges[key, sigma] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
        _edges[key, sigma].flags.writeable = False
    return _edges[key, sigma]


def _e2e_frames(planes, key):
    """"mosaic960": the mosaics' first 960 columns.  The fused Sobel+NMS+classify kernel, and with it the u8 smoothed
    plane and the colour Gaussian inside canny(), needs a width that is a multiple of 8; 964 is not, so the full
    mosaics take the s16 plane there whatever "smoothed_u8" says.  Both widths run."""
    return planes["mosaic"][:, :, :960] if key == "mosaic960" else planes[key]


@pytest.mark.parametrize("sigma", [1.0, 1.4, 2.0])
@pytest.mark.parametrize("u8", [1, 0], ids=["u8_smoothed_plane", "s16_smoothed_plane"])
def test_canny_end_to_end(ctx, planes, u8, sigma):
    """Thresholds (1, 2) on the flat frames: a single smoothed pixel that reads g - 1 instead of g (or g where the
    reference's float quotient truncates to g - 1) becomes an edge."""
    ctx.set_option("smoothed_u8", u8)
    try:
        for key, lo, hi in (("mosaic", 50, 150), ("mosaic960", 50, 150), ("flat24x24", 1, 2)):
            frames = _e2e_frames(planes, key)
            want = _oracle_canny(key, frames, sigma, lo, hi)
            got = ctx.canny_batch(frames, sigma, lo, hi)
            _compare(got, want, sigma, f"canny_batch ({lo}, {hi}), smoothed_u8 {u8}", key)
    finally:
        _defaults(ctx)


@pytest.mark.parametrize("key,fused", [("mosaic", 0), ("mosaic960", 1)])
def test_dev_canny_color_on_the_mosaics(ctx, planes, key, fused):
    """The full mosaics (the standalone conversion and the s16 plane: 964 is no multiple of 8) and their first 960
    columns (the colour Gaussian and the u8 plane)."""
    frames = _e2e_frames(planes, key)
    n, h, w = frames.shape
    want = _oracle_canny(key, frames, 1.0, 50, 150)
    src = _colour(frames, capi.LAYOUT_BGR8)
    d_src, d_out = ctx.malloc(src.nbytes), ctx.malloc(frames.nbytes * 2)
    try:
        ctx.h2d(d_src, src)
        ctx.dev_canny_color(d_src, capi.LAYOUT_BGR8, 1.0, 50, 150, h, w, n, d_out)
        got = np.empty(frames.shape, np.int16)
        ctx.d2h(got, d_out)
        assert ctx.get_option("last_canny_fused_gray") == fused
        assert ctx.get_option("last_canny_smoothed_u8") == fused
    finally:
        ctx.synchronize()
        ctx.free(d_src)
        ctx.free(d_out)
    _compare(got, want, 1.0, "dev_canny_color BGR8 (50, 150)", key)
