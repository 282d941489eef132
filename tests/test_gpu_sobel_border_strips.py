"""The fused Sobel+NMS+classify kernel at the image borders: widths, heights and segment lengths at which its border
strips can go wrong.

The kernel canny() runs gives each lane 8 adjacent pixels and each wave a strip of 62 lanes = 496 columns (plus one
halo lane on either side); its launches have width % 8 == 0, so a lane lies wholly inside or wholly outside the image
and the first / last strip of a frame handle columns 0 and W-1 with per-lane constants.  Where those lanes sit depends
on the width:

* W = 496 k: column W-1 is pixel 7 of a strip's LAST owner lane, the first outside lane is that strip's halo lane;
* W = 496 k + 8: column W-1 is pixel 7 of a new strip's FIRST owner lane, the first outside lane is its second;
* W = 8, 16: the whole frame is one or two lanes between the two outside lanes;
* W = 488, 504, 1000: the last lane sits one lane to either side of those.

Rows: a segment's march starts two rows above its first row and runs a whole number of three-row trips, so segments
of 8, 33 and 64 rows over heights around the segment and tile sizes (and of two or three rows) exercise the warm-up
steps, the last step, the rounded-up steps and the rows outside the image.

Every case is dev_canny bit for bit against the oracle, with the packed-i16 kernel (tune_sobel_variant=1, which has
none of the border code under test) as a second witness.  sigma = 0.05 leaves the frames as they are, so what the
Sobel+NMS kernel sees is what the test built.
"""
import numpy as np
import pytest

import oracle
import sobel_planes as sp

pytestmark = pytest.mark.gpu

SIGMA = 0.05
WIDTHS = [8, 16, 488, 496, 504, 512, 992, 1000]
HEIGHTS = [2, 3, 5, 63, 64, 65, 67, 130]
SEGS = [8, 33, 64]
THRESHOLDS = [(50, 150), (1, 2), (255, 255)]


def _noise(h, w, seed):
    """High-contrast noise: half of the pixels at 0 / 255, the rest uniform, so that the gradients at the four borders
    are large and of every sign."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w), dtype=np.uint8)
    hard = rng.random((h, w)) < 0.5
    f[hard] = np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)[hard]
    return f


def _frame_only(h, w, seed):
    """Bright pixels in columns 0 and W-1 and rows 0 and H-1 only (random values there, zero inside)."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w), np.uint8)
    f[:, 0] = rng.integers(128, 256, h)
    f[:, w - 1] = rng.integers(128, 256, h)
    f[0, :] = rng.integers(128, 256, w)
    f[h - 1, :] = rng.integers(128, 256, w)
    return f


def _plane_corner(h, w, which):
    """A corner of plane 0 of the adversarial planes of sobel_planes.py, whose four border bands are filled: 0 = top
    left (left and top bands), 1 = top right (right and top bands), 2 = bottom left (left and bottom bands).  The
    bands' chosen gradients sit on the crop's own border."""
    plane = sp.build()["planes"][0]
    ph, pw = plane.shape
    if which == 0:
        return np.ascontiguousarray(plane[:h, :w])
    if which == 1:
        return np.ascontiguousarray(plane[:h, pw - w:])
    return np.ascontiguousarray(plane[ph - h:, :w])


def _frames(h, w):
    """Six frames per shape; a case takes one to three of them."""
    return np.stack([_noise(h, w, 1000 * h + w), _frame_only(h, w, 7 * h + w), _plane_corner(h, w, 0),
                     _plane_corner(h, w, 1), _plane_corner(h, w, 2), _noise(h, w, 31 * h + 3 * w + 1)])


_want = {}


def _oracle(frames, h, w, k, lo, hi):
    key = (h, w, k, lo, hi)
    if key not in _want:
        _want[key] = oracle.canny(frames[k], SIGMA, lo, hi)
    return _want[key]


def _report(got, want):
    bad = np.argwhere(got != want)
    return len(bad), [(*b.tolist(), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:6]]


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.set_option("tune_sobel_variant", 0)  # process-wide
    c.close()


class _Dev:
    """Device buffers for the largest batch of the module."""

    def __init__(self, c, nbytes):
        self.c = c
        self.d_in, self.d_out, self.d_thr = c.malloc(nbytes), c.malloc(2 * nbytes), c.malloc(64)

    def free(self):
        for p in (self.d_in, self.d_out, self.d_thr):
            self.c.free(p)


@pytest.fixture(scope="module")
def dev(ctx):
    d = _Dev(ctx, 3 * max(HEIGHTS) * max(WIDTHS))
    yield d
    d.free()


def _run(ctx, dev, batch, lo, hi, seg, u8, variant, pairs=None):
    n, h, w = batch.shape
    ctx.set_option("tune_sobel_variant", variant)
    ctx.set_option("tune_sobel_seg", seg)
    ctx.set_option("smoothed_u8", u8)
    ctx.set_option("fuse_classify", 1)
    try:
        ctx.h2d(dev.d_in, batch)
        if pairs is None:
            ctx.dev_canny(dev.d_in, SIGMA, lo, hi, h, w, n, dev.d_out)
        else:
            ctx.h2d(dev.d_thr, np.ascontiguousarray(pairs, np.int32))
            ctx.dev_canny_thresholds(dev.d_in, SIGMA, dev.d_thr, h, w, n, dev.d_out)
        assert ctx.get_option("last_canny_smoothed_u8") == u8  # the fused kernel ran, on the plane asked for
        got = np.empty((n, h, w), np.int16)
        ctx.d2h(got, dev.d_out)
    finally:
        ctx.set_option("tune_sobel_variant", 0)
        ctx.set_option("tune_sobel_seg", 0)
        ctx.set_option("smoothed_u8", 1)
    return got


@pytest.mark.parametrize("u8", [1, 0], ids=["u8_smoothed_plane", "s16_smoothed_plane"])
@pytest.mark.parametrize("w", WIDTHS)
def test_border_strips_against_oracle(ctx, dev, w, u8):
    """Every height x segment length x threshold pair at one width, all six frame kinds each time: in calls of one,
    two and three frames, and which kinds share a call rotates from case to case."""
    case = 0
    for h in HEIGHTS:
        frames = _frames(h, w)
        for seg in SEGS:
            for lo, hi in THRESHOLDS:
                order = [(case + i) % len(frames) for i in range(len(frames))]
                case += 1
                for pick in (order[:1], order[1:3], order[3:]):
                    batch = np.ascontiguousarray(frames[pick])
                    want = np.stack([_oracle(frames, h, w, k, lo, hi) for k in pick])
                    got = _run(ctx, dev, batch, lo, hi, seg, u8, 0)
                    assert np.array_equal(got, want), (w, h, seg, lo, hi, u8, pick, _report(got, want))
                    witness = _run(ctx, dev, batch, lo, hi, seg, u8, 1)
                    assert np.array_equal(witness, want), ("packed", w, h, seg, lo, hi, u8, pick,
                                                           _report(witness, want))


@pytest.mark.parametrize("u8", [1, 0], ids=["u8_smoothed_plane", "s16_smoothed_plane"])
def test_border_strips_per_frame_pairs(ctx, dev, u8):
    """Explicit per-frame pairs (the kernel's THR body): three frames, three pairs, every width."""
    pairs = np.array(THRESHOLDS, np.int32)
    for i, w in enumerate(WIDTHS):
        for h in (HEIGHTS[i % len(HEIGHTS)], 67, 130):
            frames = _frames(h, w)
            pick = [(i + j) % len(frames) for j in range(3)]
            batch = np.ascontiguousarray(frames[pick])
            want = np.stack([_oracle(frames, h, w, k, int(lo), int(hi)) for k, (lo, hi) in zip(pick, pairs)])
            for seg in SEGS:
                got = _run(ctx, dev, batch, 0, 0, seg, u8, 0, pairs)
                assert np.array_equal(got, want), (w, h, seg, u8, pick, _report(got, want))
                witness = _run(ctx, dev, batch, 0, 0, seg, u8, 1, pairs)
                assert np.array_equal(witness, want), ("packed", w, h, seg, u8, pick, _report(witness, want))


def test_border_frames_have_border_edges():
    """The inputs do what they are for: the oracle keeps edge pixels in columns 0 and W-1 and rows 0 and H-1 of the
    noise and border-only frames, and at 130 rows the plane corners carry kept pixels on the borders whose bands they
    hold."""
    for w in WIDTHS:
        frames = _frames(130, w)
        for k in (0, 1):
            e = _oracle(frames, 130, w, k, 1, 2)
            assert e[:, 0].any() and e[:, w - 1].any() and e[0].any() and e[129].any(), (w, k)
        tl, tr, bl = (_oracle(frames, 130, w, k, 1, 2) for k in (2, 3, 4))
        assert tl[:, 0].any() and tl[0].any() and tr[:, w - 1].any() and tr[0].any() and bl[:, 0].any() and bl[129].any(), w
