"""CPU-only helpers for the histogram and select tests of the automatic thresholds: the numpy
restatement of the rule, the reference histograms (np.bincount of the plane, or of min(Sobel magnitude, 256)), the launch
arithmetic of canny_kernels.hip restated from its constants, and the designed planes and histograms the tests upload.
Everything here is plain numpy; no kernel is launched."""
import math
import os
import re

import numpy as np

import oracle

BINS = 257
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KERNELS = open(os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_kernels.hip")).read()


def _const(name):
    return int(re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, _KERNELS).group(1))


# the launch constants of the histogram kernels, read from the source so that a change there moves the designed cases
HIST_WAVES, HIST_BLOCKS, HIST_GROUPS = _const("kHistWaves"), _const("kHistBlocks"), _const("kHistGroups")
TILE_W, TILE_H = _const("HG_TW"), _const("HG_TH")
BLOCK = HIST_WAVES * 64


def blocks_per_frame(n_frames, units_per_frame):
    """hist_blocks_per_frame: about HIST_BLOCKS workgroups in all, at most one per unit of work, at least one."""
    return max(1, min(-(-HIST_BLOCKS // n_frames), units_per_frame))


def intensity_launch(h, w, n_frames):
    """(workgroups per frame, 16-pixel groups that can overlap one frame) of launch_hist_intensity.  One pass of a lane's
    outer loop takes HIST_GROUPS groups, so a lane iterates when the groups exceed blocks * BLOCK * HIST_GROUPS."""
    groups = h * w // 16 + 2
    lanes = -(-groups // HIST_GROUPS)
    return blocks_per_frame(n_frames, -(-lanes // BLOCK)), groups


def gradient_launch(h, w, n_frames):
    """(workgroups per frame, tiles per frame) of launch_hist_gradient."""
    tiles = -(-w // TILE_W) * -(-h // TILE_H)
    return blocks_per_frame(n_frames, tiles), tiles


# ---- the rule ------------------------------------------------------------------------------------------------------
def np_quantile(hist, q):
    """Inverted-CDF quantile: min { b : h[0] + ... + h[b] >= max(1, ceil(q * N)) }, q a float32 widened to double;
    257 when no bin reaches the count (N = 0)."""
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64))
    need = max(1, math.ceil(float(np.float32(q)) * float(int(cum[-1]))))
    return int(np.searchsorted(cum, need, side="left"))


def np_rule(hist, rule, low, high):
    if rule in ("median", 1):
        m = np_quantile(hist, 0.5)
        lo, hi = math.floor(float(np.float32(low)) * m), math.floor(float(np.float32(high)) * m)
    else:
        lo, hi = np_quantile(hist, low), np_quantile(hist, high)
    lo = min(max(lo, 1), 255)
    return lo, min(max(hi, lo), 255)


# ---- reference histograms ------------------------------------------------------------------------------------------
def intensity_hist(planes):
    """[n, h, w] planes in [0,255] -> [n, 257] uint32: bin = value (bin 256 stays empty)."""
    return np.stack([np.bincount(p.ravel(), minlength=BINS) for p in planes]).astype(np.uint32)


def np_sobel_magnitude(plane):
    """The reference's Sobel magnitude restated in numpy for any shape, 1 x 1 included: gx clamps the column index to
    the image and drops the rows outside it, gy clamps the row index and drops the columns outside it; floor(sqrt(gx^2 +
    gy^2)).  Integer arithmetic; the square root of an integer below 2^53 is correctly rounded, so its floor is exact."""
    p = np.asarray(plane, dtype=np.int64)
    h, w = p.shape
    cols, rows = np.arange(w), np.arange(h)
    d = p[:, np.minimum(cols + 1, w - 1)] - p[:, np.maximum(cols - 1, 0)]
    gx = 2 * d
    gx[:-1] += d[1:]
    gx[1:] += d[:-1]
    e = p[np.minimum(rows + 1, h - 1)] - p[np.maximum(rows - 1, 0)]
    gy = 2 * e
    gy[:, :-1] += e[:, 1:]
    gy[:, 1:] += e[:, :-1]
    return np.floor(np.sqrt((gx * gx + gy * gy).astype(np.float64))).astype(np.int64)


def sobel_magnitude(plane):
    """oracle.sobel's magnitude; the oracle refuses frames with fewer than two rows or columns (the reference reads out of
    bounds there), so those come from the numpy restatement, which the tests check against the oracle on every other
    shape."""
    h, w = plane.shape
    if h < 2 or w < 2:
        return np_sobel_magnitude(plane)
    return oracle.sobel(plane.astype(np.int16))[0].astype(np.int64)


def gradient_hist(planes):
    """[n, h, w] planes in [0,255] -> [n, 257] uint32: bin = min(Sobel magnitude, 256)."""
    return np.stack([np.bincount(np.minimum(sobel_magnitude(p), 256).ravel(), minlength=BINS)
                     for p in planes]).astype(np.uint32)


# ---- planes for the intensity histogram ----------------------------------------------------------------------------
# Each takes (n, h, w, rng) and returns [n, h, w] uint8.  `i` below is the pixel index in the whole batch: the kernel's
# 16-pixel groups are aligned to the batch's first pixel, so a frame of h * w % 16 != 0 pixels starts inside a group.
def _batch_index(n, h, w):
    return np.arange(n * h * w, dtype=np.int64)


def _shape(flat, n, h, w):
    return np.ascontiguousarray(flat.reshape(n, h, w).astype(np.uint8))


def plane_noise(n, h, w, rng):
    return rng.integers(0, 256, (n, h, w), dtype=np.uint8)


def plane_ramp(n, h, w, rng):
    """A slow ramp: a step of 1 every 23 pixels, so some groups are flat, their neighbours in the wave one apart."""
    return _shape((_batch_index(n, h, w) // 23 + 3) % 256, n, h, w)


def plane_const(value):
    def make(n, h, w, rng):
        return np.full((n, h, w), value, np.uint8)
    make.__name__ = "plane_const_%d" % value
    return make


def plane_frames_differ(n, h, w, rng):
    """Constant frames, each with a value of its own."""
    return _shape(np.repeat((np.arange(n) * 37 + 5) % 256, h * w), n, h, w)


def plane_frames_pairwise_equal(n, h, w, rng):
    """Constant frames: frames 2k and 2k + 1 share a value, the next pair has another."""
    return _shape(np.repeat((np.arange(n) // 2 * 50 + 7) % 256, h * w), n, h, w)


def plane_flat_groups(n, h, w, rng):
    """Every aligned 16-pixel group is flat, with a value that differs from lane to lane."""
    return _shape((_batch_index(n, h, w) // 16 * 7 + 1) % 256, n, h, w)


def plane_stretches_batch(n, h, w, rng):
    """Stretches of 1024 equal pixels (a wave's 64 groups), aligned to the batch's first pixel."""
    return _shape((_batch_index(n, h, w) // 1024 * 41 + 2) % 256, n, h, w)


def plane_stretches_frame(n, h, w, rng):
    """The same stretches counted from each frame's first pixel: aligned to a wave only where the frame starts on a
    group."""
    i = _batch_index(n, h, w)
    return _shape((i % (h * w) // 1024 * 41 + i // (h * w) * 3 + 9) % 256, n, h, w)


def plane_one_differs(e):
    """Groups of 15 equal pixels and a different one at position e."""
    def make(n, h, w, rng):
        i = _batch_index(n, h, w)
        g = i // 16
        base = (g * 5 + 11) % 256
        return _shape(np.where(i % 16 == e, (base + 1 + g % 200) % 256, base), n, h, w)
    make.__name__ = "plane_one_differs_%d" % e
    return make


INTENSITY_PLANES = ([plane_noise, plane_ramp, plane_const(0), plane_const(1), plane_const(255), plane_frames_differ,
                     plane_frames_pairwise_equal, plane_flat_groups, plane_stretches_batch, plane_stretches_frame]
                    + [plane_one_differs(e) for e in range(16)])


def plane_mixed_frames(n, h, w, rng):
    """A large batch whose frames take turns: noise, the ramp, stretches from the frame's start, a constant."""
    out = plane_noise(n, h, w, rng)
    i = np.arange(h * w, dtype=np.int32)
    out[1::4] = (((i // 23 + 3) & 255).astype(np.uint8)).reshape(h, w)
    out[2::4] = (((i // 1024 * 41 + 9) & 255).astype(np.uint8)).reshape(h, w)
    out[3::4] = ((np.arange(3, n, 4) // 8 * 50 + 7) & 255).astype(np.uint8)[:, None, None]
    return out


# ---- planes for the gradient histogram -----------------------------------------------------------------------------
def plane_noise_low(n, h, w, rng):
    return rng.integers(0, 21, (n, h, w), dtype=np.uint8)


def plane_ramp_x(n, h, w, rng):
    return np.ascontiguousarray(np.broadcast_to((np.arange(w) % 256).astype(np.uint8), (n, h, w)))


def plane_ramp_y(n, h, w, rng):
    return np.ascontiguousarray(np.broadcast_to((np.arange(h) * 3 % 256).astype(np.uint8)[:, None], (n, h, w)))


def plane_step(col, row):
    """10 left of column `col` and above row `row`, 200 elsewhere: one vertical and one horizontal step edge."""
    def make(n, h, w, rng):
        p = np.full((n, h, w), 200, np.uint8)
        p[:, :row, :col] = 10
        return p
    make.__name__ = "plane_step_%d_%d" % (col, row)
    return make


GRADIENT_PLANES = [plane_noise, plane_noise_low, plane_const(1), plane_const(128), plane_const(255), plane_ramp_x,
                   plane_ramp_y, plane_step(64, 32), plane_step(37, 13)]


# ---- histograms for the select kernel ------------------------------------------------------------------------------
def random_hist(rng):
    """The generator kinds of tests/test_auto_thresholds_rule.py."""
    kind = rng.integers(0, 5)
    h = np.zeros(BINS, np.uint32)
    if kind == 0:  # dense
        h[:] = rng.integers(0, 1000, BINS)
    elif kind == 1:  # a few occupied bins
        idx = rng.integers(0, BINS, rng.integers(1, 6))
        h[idx] = rng.integers(1, 10**6, idx.size)
    elif kind == 2:  # an image-like intensity histogram
        v = np.clip(rng.normal(rng.uniform(0, 255), rng.uniform(1, 60), rng.integers(1, 5000)), 0, 255).astype(int)
        h[:256] = np.bincount(v, minlength=256)
    elif kind == 3:  # a gradient-like histogram: mass near 0, a long tail, clamped at 256
        v = np.minimum(rng.exponential(rng.uniform(1, 200), rng.integers(1, 5000)).astype(int), 256)
        h[:] = np.bincount(v, minlength=BINS)
    else:  # large counts (a 4K frame has 8.3 M pixels)
        h[:] = rng.integers(0, 2**24, BINS)
    if h.sum() == 0:
        h[rng.integers(0, BINS)] = 1
    return h


def hists_single_bin():
    """257 histograms: all mass in bin b, for every b."""
    return (np.eye(BINS, dtype=np.uint32) * 1000).astype(np.uint32)


def hists_lane_boundaries():
    """Equal mass in bins 5l + 4 and 5l + 5: the last bin one lane of the select kernel owns and the next lane's first."""
    lanes = np.arange((BINS - 1) // 5)
    h = np.zeros((lanes.size, BINS), np.uint32)
    h[lanes, 5 * lanes + 4] = 77
    h[lanes, 5 * lanes + 5] = 77
    return h


def hists_random(count=300, seed=401):
    rng = np.random.default_rng(seed)
    return np.stack([random_hist(rng) for _ in range(count)])


def hists_beyond_32_bits():
    """Totals above 2^32, which only the high word of the kernel's 64-bit scan can carry."""
    rng = np.random.default_rng(402)
    full = np.full(BINS, 2**32 - 1, np.uint32)
    half = np.full(BINS, 2**31, np.uint32)
    sparse = np.zeros(BINS, np.uint32)
    sparse[::7] = 2**31
    # the running sum first reaches 2^32 inside lane 3's bins (15 .. 19): 16 bins of 2^28 - 1 stay below, bin 16 crosses
    carry_mid = np.full(BINS, 2**28 - 1, np.uint32)
    # ... and between two neighbouring bins of one lane (lane 24 owns 120 .. 124), with a light tail
    carry_lane = np.zeros(BINS, np.uint32)
    carry_lane[[122, 123, 200]] = 2**32 - 1, 2**32 - 1, 3
    noise = rng.integers(0, 2**32, BINS, dtype=np.uint64).astype(np.uint32)
    hs = np.stack([full, half, sparse, carry_mid, carry_lane, noise])
    assert (hs.astype(np.uint64).sum(axis=1) > 2**32).all()
    return hs
