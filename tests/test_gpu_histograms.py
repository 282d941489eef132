"""The histogram and select kernels of the automatic thresholds, each on its own.

canny_hip_selftest_histogram launches hist_intensity_kernel / hist_gradient_kernel exactly as canny_hip_dev_canny_auto does,
on a plane the test designs; canny_hip_selftest_select launches thr_select_kernel on histograms the test designs.  Every
comparison is exact: whole [n][257] histograms against np.bincount of the plane (or of min(Sobel magnitude, 256)), pair
arrays against the numpy restatement of the rule and against the host export.  tests/test_gpu_auto_thresholds.py sees
only the selected pairs, which a few miscounted pixels away from the quantile crossing do not move; these tests do."""
import ctypes as C
import functools

import numpy as np
import pytest

import hist_rule as hr
from canny_edge_amd import capi

gpu = pytest.mark.gpu  # the tests that launch kernels; the checks of the designed cases themselves run anywhere

BINS = hr.BINS
POISON = 0xA5  # bytes behind the plane: a read past its end that is counted shows up in the histogram
GUARD = 0xDEADBEEF  # the histogram buffer before the call, and the row behind the last frame's after it


@pytest.fixture(scope="module")
def ctx(hip):
    with capi.Context(0) as c:
        yield c


class Buffers:
    """One plane buffer and one histogram buffer on the device, sized for the largest case of a test."""

    def __init__(self, ctx, max_px, max_frames):
        self.ctx = ctx
        self.d_plane = ctx.malloc(max_px * 2 + 64)
        self.d_hist = ctx.malloc((max_frames + 1) * BINS * 4)

    def histogram(self, planes, u8, kind):
        n, h, w = planes.shape
        body = planes if u8 else planes.astype(np.int16)
        host = np.concatenate([body.reshape(-1).view(np.uint8), np.full(64, POISON, np.uint8)])
        self.ctx.h2d(self.d_plane, host)
        self.ctx.h2d(self.d_hist, np.full((n + 1, BINS), GUARD, np.uint32))
        self.ctx.selftest_histogram(self.d_plane, u8, kind, h, w, n, self.d_hist)
        got = np.empty((n + 1, BINS), np.uint32)
        self.ctx.synchronize()
        self.ctx.d2h(got, self.d_hist)
        assert (got[n] == GUARD).all(), "the row behind the last frame's histogram was written"
        return got[:n]

    def free(self):
        self.ctx.synchronize()
        self.ctx.free(self.d_plane)
        self.ctx.free(self.d_hist)


def check_hist(got, want, px, what):
    assert want.dtype == np.uint32 and (want.sum(axis=1, dtype=np.uint64) == px).all(), what
    if not np.array_equal(got, want):
        f, b = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} bins differ, first frame {f} bin {b}: "
                             f"got {got[f, b]}, want {want[f, b]}")
    assert (got.sum(axis=1, dtype=np.uint64) == px).all(), what


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- intensity -----------------------------------------------------------------------------------------------------
INTENSITY_SHAPES = [(1, 1), (3, 5), (5, 5), (1, 17), (7, 17), (21, 27), (33, 31), (37, 53), (24, 23), (40, 62)]
FRAME_COUNTS = (1, 2, 3, 5, 8)
# n_frames = 256 caps the grid at ceil(kHistBlocks / 256) = 8 workgroups per frame; a pass of a lane's outer loop takes
# kHistGroups = 4 groups, so the 8 * 256 lanes cover 8192 groups = 131,072 pixels at once and a 401 x 403 frame (161,603
# pixels, % 16 = 3) sends every lane round again -- with the last pass partly past the frame's end.  Fewer frames would
# widen the grid and a proportionally larger frame would be needed: the batch cannot be made smaller than about
# kHistBlocks * 256 * kHistGroups * 16 pixels.  test_launch_arithmetic_of_the_large_cases asserts these figures from the
# constants in the source.
BIG_INTENSITY = (256, 401, 403)


def test_intensity_shapes_cover_every_residue():
    assert {h * w % 16 for h, w in INTENSITY_SHAPES} >= {0, 1, 7, 8, 9, 15}
    assert BIG_INTENSITY[1] * BIG_INTENSITY[2] % 16 != 0


def test_launch_arithmetic_of_the_large_cases():
    n, h, w = BIG_INTENSITY
    blocks, groups = hr.intensity_launch(h, w, n)
    assert blocks < -(-groups // (hr.BLOCK * hr.HIST_GROUPS)), "the grid is not capped"
    assert groups > blocks * hr.BLOCK * hr.HIST_GROUPS, "no lane runs its outer loop twice"
    n, h, w = BIG_GRADIENT
    blocks, tiles = hr.gradient_launch(h, w, n)
    assert -(-tiles // blocks) >= 3, "no workgroup walks three tiles"
    # the small cases, in contrast, have one workgroup per tile and one pass per lane
    for gh, gw in GRADIENT_SHAPES:
        assert hr.gradient_launch(gh, gw, 3)[0] == hr.gradient_launch(gh, gw, 3)[1]


def test_intensity_planes_are_what_they_claim():
    n, h, w = 3, 37, 53
    for index, make in enumerate(hr.INTENSITY_PLANES):
        planes, want = intensity_case(index, n, h, w)
        assert planes.shape == (n, h, w) and planes.dtype == np.uint8 and want.shape == (n, BINS), make.__name__
    groups = lambda name: by_name[name].reshape(-1)[:n * h * w // 16 * 16].reshape(-1, 16).astype(int)
    by_name = {make.__name__: intensity_case(i, n, h, w)[0] for i, make in enumerate(hr.INTENSITY_PLANES)}
    flat = groups("plane_flat_groups")
    assert (flat == flat[:, :1]).all() and (np.diff(flat[:, 0]) != 0).all()
    for e in range(16):
        g = groups("plane_one_differs_%d" % e)
        rest = np.delete(g, e, axis=1)
        assert (rest == rest[:, :1]).all() and (g[:, e] != rest[:, 0]).all(), e
    runs = by_name["plane_stretches_batch"].reshape(-1)
    assert (runs[:1024] == runs[0]).all() and runs[1024] != runs[0]
    same = by_name["plane_frames_pairwise_equal"]
    assert same[0, 0, 0] == same[1, 0, 0] != same[2, 0, 0] and (same[1] == same[1, 0, 0]).all()


@functools.lru_cache(maxsize=None)
def intensity_case(index, n, h, w):
    make = hr.INTENSITY_PLANES[index]
    planes = make(n, h, w, np.random.default_rng(1000 * index + 10 * n + h))
    return _frozen(planes, hr.intensity_hist(planes))


@gpu
@pytest.mark.parametrize("u8", [True, False], ids=["byte_plane", "short_plane"])
@pytest.mark.parametrize("shape", INTENSITY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_intensity_histogram_is_bincount(ctx, shape, u8):
    """Every designed plane at every frame count: pixel counts that are not multiples of 16 make frames start inside a
    16-pixel group (masked per pixel, never flat) and end the batch with a partial group (loaded element by element)."""
    h, w = shape
    buf = Buffers(ctx, max(FRAME_COUNTS) * h * w, max(FRAME_COUNTS))
    try:
        for n in FRAME_COUNTS:
            for index, make in enumerate(hr.INTENSITY_PLANES):
                planes, want = intensity_case(index, n, h, w)
                assert planes.shape == (n, h, w) and planes.dtype == np.uint8
                check_hist(buf.histogram(planes, u8, "median"), want, h * w, (make.__name__, n, shape, u8))
    finally:
        buf.free()


@pytest.fixture(scope="module")
def big_intensity():
    n, h, w = BIG_INTENSITY
    planes = hr.plane_mixed_frames(n, h, w, np.random.default_rng(77))
    return _frozen(planes, hr.intensity_hist(planes))


@gpu
@pytest.mark.parametrize("u8", [True, False], ids=["byte_plane", "short_plane"])
def test_intensity_histogram_lanes_iterate(ctx, big_intensity, u8):
    """The capped grid (see BIG_INTENSITY): every lane runs its outer loop twice, the second time partly past the frame."""
    planes, want = big_intensity
    n, h, w = planes.shape
    buf = Buffers(ctx, planes.size, n)
    try:
        check_hist(buf.histogram(planes, u8, "median"), want, h * w, ("mixed_frames", planes.shape, u8))
    finally:
        buf.free()


# ---- gradient ------------------------------------------------------------------------------------------------------
GRADIENT_SHAPES = [(1, 1), (1, 130), (70, 1), (33, 65), (70, 130), (2, 2), (31, 63), (32, 64), (33, 64), (32, 65),
                   (2, 130), (70, 2), (1, 64), (31, 1)]
# 130 x 200 is 4 x 5 = 20 tiles of 64 x 32; with 256 frames the grid is capped at 8 workgroups per frame, so workgroups
# 0..3 take three tiles each (t, t + 8, t + 16) through the register prefetch and the others two.
BIG_GRADIENT = (256, 130, 200)


def test_gradient_shapes_cover_the_tile_edges():
    assert {w for _, w in GRADIENT_SHAPES} == {1, 2, 63, 64, 65, 130}
    assert {h for h, _ in GRADIENT_SHAPES} == {1, 2, 31, 32, 33, 70}
    assert {(1, 1), (1, 130), (70, 1), (33, 65), (70, 130)} <= set(GRADIENT_SHAPES)
    assert hr.TILE_W == 64 and hr.TILE_H == 32  # the sizes above sit one below, on and one above these


@functools.lru_cache(maxsize=None)
def gradient_case(index, n, h, w):
    make = hr.GRADIENT_PLANES[index]
    planes = make(n, h, w, np.random.default_rng(2000 * index + 10 * n + h))
    return _frozen(planes, hr.gradient_hist(planes))


@gpu
@pytest.mark.parametrize("u8", [True, False], ids=["byte_plane", "short_plane"])
@pytest.mark.parametrize("shape", GRADIENT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gradient_histogram_is_bincount_of_sobel(ctx, shape, u8):
    h, w = shape
    buf = Buffers(ctx, 3 * h * w, 3)
    try:
        for n in (1, 3):
            for index, make in enumerate(hr.GRADIENT_PLANES):
                planes, want = gradient_case(index, n, h, w)
                check_hist(buf.histogram(planes, u8, "quantile"), want, h * w, (make.__name__, n, shape, u8))
    finally:
        buf.free()


def test_gradient_references_are_not_vacuous():
    """Full-range noise fills the clamp bin, low noise spreads over the low bins, the ramps put whole rows of a tile into
    one non-zero bin (one atomic for the wave).  A constant plane has no gradient anywhere under the reference's border
    rule -- every term is a difference of two pixels, and a dropped term drops both -- so its whole frame is bin 0, the
    wave-uniform path on every row, full or partial."""
    h, w = 70, 130
    by_name = {make.__name__: gradient_case(i, 1, h, w)[1][0] for i, make in enumerate(hr.GRADIENT_PLANES)}
    assert by_name["plane_noise"][256] > h * w // 2
    assert np.count_nonzero(by_name["plane_noise_low"][:120]) > 60 and by_name["plane_noise_low"][256] == 0
    for name in ("plane_const_1", "plane_const_128", "plane_const_255"):
        assert by_name[name][0] == h * w
    assert by_name["plane_ramp_x"][8] >= (h - 2) * (w - 2) and by_name["plane_ramp_y"][24] >= (h - 2) * (w - 2)
    for name in ("plane_step_64_32", "plane_step_37_13"):
        assert by_name[name][256] > 0 and by_name[name][0] > 0


@pytest.fixture(scope="module")
def big_gradient():
    n, h, w = BIG_GRADIENT
    planes = hr.plane_noise(n, h, w, np.random.default_rng(78))
    planes[1::4] = hr.plane_noise_low(n, h, w, np.random.default_rng(79))[1::4]
    planes[2::4] = hr.plane_ramp_y(n, h, w, None)[2::4]
    planes[3::4] = hr.plane_step(64, 32)(n, h, w, None)[3::4]
    return _frozen(planes, hr.gradient_hist(planes))


@gpu
@pytest.mark.parametrize("u8", [True, False], ids=["byte_plane", "short_plane"])
def test_gradient_histogram_blocks_walk_tiles(ctx, big_gradient, u8):
    """The capped grid (see BIG_GRADIENT): a workgroup counts three tiles, fetching the next while it counts."""
    planes, want = big_gradient
    n, h, w = planes.shape
    buf = Buffers(ctx, planes.size, n)
    try:
        check_hist(buf.histogram(planes, u8, "quantile"), want, h * w, ("mixed_frames", planes.shape, u8))
    finally:
        buf.free()


def test_numpy_sobel_restatement_matches_the_oracle():
    """The oracle refuses one-row and one-column frames, so those references come from hist_rule.np_sobel_magnitude; on
    every other shape and plane of this file the two must agree pixel for pixel."""
    for h, w in GRADIENT_SHAPES:
        if h < 2 or w < 2:
            continue
        for index in range(len(hr.GRADIENT_PLANES)):
            for p in gradient_case(index, 3, h, w)[0]:
                assert np.array_equal(hr.np_sobel_magnitude(p), hr.sobel_magnitude(p)), (h, w, index)


# ---- select --------------------------------------------------------------------------------------------------------
SELECT_PARAMS = (("median", 0.67, 1.33), ("quantile", 0.7, 0.9), ("median", 0.0, 5.0), ("median", 1.0, 1.0),
                 ("quantile", 1e-6, 1.0), ("quantile", 0.5, 0.5))
SELECT_HISTS = {
    # an empty histogram between two occupied ones: frames are independent
    "empty": lambda: np.stack([hr.hists_single_bin()[40], np.zeros(BINS, np.uint32), hr.hists_single_bin()[200]]),
    "single_bin": hr.hists_single_bin,
    "lane_boundaries": hr.hists_lane_boundaries,
    "random": hr.hists_random,
    "beyond_32_bits": hr.hists_beyond_32_bits,
}


@functools.lru_cache(maxsize=None)
def select_hists(name):
    return _frozen(np.ascontiguousarray(SELECT_HISTS[name](), dtype=np.uint32))[0]


def run_select(ctx, hists, rule, low, high):
    n = hists.shape[0]
    d_hist, d_pairs = ctx.malloc(hists.nbytes), ctx.malloc((n + 1) * 8)
    try:
        ctx.h2d(d_hist, hists)
        ctx.h2d(d_pairs, np.full((n + 1, 2), -7, np.int32))
        ctx.selftest_select(d_hist, n, rule, low, high, d_pairs)
        got = np.empty((n + 1, 2), np.int32)
        ctx.synchronize()
        ctx.d2h(got, d_pairs)
    finally:
        ctx.synchronize()
        ctx.free(d_hist)
        ctx.free(d_pairs)
    assert (got[n] == -7).all(), "the pair behind the last frame's was written"
    return got[:n]


@gpu
@pytest.mark.parametrize("rule,low,high", SELECT_PARAMS)
@pytest.mark.parametrize("name", list(SELECT_HISTS))
def test_select_matches_numpy_rule_and_host_export(ctx, name, rule, low, high):
    """The device prefix sum (5 bins per lane, then a 64-bit wave scan made of two 32-bit shuffles) against the numpy
    rule and the host export, frame by frame.

    beyond_32_bits: a real frame cannot hold 2^32 pixels (height * width is capped at 2^31 - 1), so no histogram the
    pipeline builds sums past the low word.  The case pins the scan's high word all the same: the kernel declares a
    64-bit cumulative count and computes it, and the host export accepts any 257 unsigned counts."""
    hists = select_hists(name)
    got = run_select(ctx, hists, rule, low, high)
    want = np.array([hr.np_rule(h, rule, low, high) for h in hists], np.int32)
    if not np.array_equal(got, want):
        f = int(np.argwhere((got != want).any(axis=1))[0, 0])
        raise AssertionError(f"{name} {rule} {low} {high}: {int((got != want).any(axis=1).sum())} frames differ, first "
                             f"{f}: got {tuple(got[f])}, want {tuple(want[f])}, bins {np.nonzero(hists[f])[0][:8]}")
    for f, h in enumerate(hists):
        if h.any():
            assert capi.auto_thresholds_from_histogram(h, rule, low, high) == tuple(want[f]), (name, f)
        else:  # the host export refuses an empty histogram; the kernel reports Q = 257, clamped like any other
            with pytest.raises(capi.CannyHipError):
                capi.auto_thresholds_from_histogram(h, rule, low, high)
    assert ((1 <= got[:, 0]) & (got[:, 0] <= got[:, 1]) & (got[:, 1] <= 255)).all()


# ---- argument checks -----------------------------------------------------------------------------------------------
@gpu
def test_selftest_histogram_rejects_bad_arguments(ctx):
    n, h, w = 2, 5, 5
    d_plane, d_hist = ctx.malloc(n * h * w), ctx.malloc(n * BINS * 4)
    try:
        ctx.h2d(d_plane, np.zeros(n * h * w, np.uint8))
        ctx.h2d(d_hist, np.full((n, BINS), GUARD, np.uint32))
        fn, P = ctx._L.canny_hip_selftest_histogram, C.c_void_p
        bad = [(None, P(d_plane), 1, 1, h, w, n, P(d_hist)), (ctx._h, None, 1, 1, h, w, n, P(d_hist)),
               (ctx._h, P(d_plane), 1, 1, h, w, n, None)]
        bad += [(ctx._h, P(d_plane), 1, kind, h, w, n, P(d_hist)) for kind in (0, 3, -1)]
        bad += [(ctx._h, P(d_plane), 1, 2, hh, ww, nn, P(d_hist))
                for hh, ww, nn in ((0, w, n), (h, 0, n), (h, w, 0), (-1, w, n), (h, -3, n), (h, w, -2))]
        for args in bad:
            assert fn(*args) == 1, args[2:7]  # CANNY_HIP_ERR_INVALID
        got = np.empty((n, BINS), np.uint32)
        ctx.synchronize()
        ctx.d2h(got, d_hist)
        assert (got == GUARD).all()
    finally:
        ctx.synchronize()
        ctx.free(d_plane)
        ctx.free(d_hist)


@gpu
def test_selftest_select_rejects_bad_arguments(ctx):
    n = 3
    d_hist, d_pairs = ctx.malloc(n * BINS * 4), ctx.malloc(n * 8)
    try:
        ctx.h2d(d_hist, np.ones((n, BINS), np.uint32))
        ctx.h2d(d_pairs, np.full((n, 2), -7, np.int32))
        fn, P = ctx._L.canny_hip_selftest_select, C.c_void_p
        bad = [(None, P(d_hist), n, 1, 0.67, 1.33, P(d_pairs)), (ctx._h, None, n, 1, 0.67, 1.33, P(d_pairs)),
               (ctx._h, P(d_hist), n, 1, 0.67, 1.33, None), (ctx._h, P(d_hist), 0, 1, 0.67, 1.33, P(d_pairs)),
               (ctx._h, P(d_hist), -1, 1, 0.67, 1.33, P(d_pairs))]
        bad += [(ctx._h, P(d_hist), n, rule, low, high, P(d_pairs))  # the parameter checks of canny_hip_dev_canny_auto
                for rule, low, high in ((0, 0.5, 1.0), (3, 0.5, 1.0), (1, -1.0, 1.0), (1, 2.0, 1.0), (2, 0.0, 0.5),
                                        (2, 0.5, 1.5), (2, 0.9, 0.5), (1, float("nan"), 1.0), (2, 0.5, float("nan")),
                                        (1, 0.5, float("inf")))]
        for args in bad:
            assert fn(*args) == 1, args[2:6]
        got = np.empty((n, 2), np.int32)
        ctx.synchronize()
        ctx.d2h(got, d_pairs)
        assert (got == -7).all()
    finally:
        ctx.synchronize()
        ctx.free(d_hist)
        ctx.free(d_pairs)
