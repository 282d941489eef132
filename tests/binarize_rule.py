"""The binarization rule of include/canny_hip.h in numpy and Python ints: what the host C++
(canny_binarize_host.cpp) and the kernels (canny_binarize.hip) are compared with, byte for byte.  Not a test module.

The window sum S comes from a summed-area table of the edge-padded frame -- unlike the host (column sums per row) and the
kernels (direct sums; vertical running sums and a prefix sum per row).  cond exists in both forms of the header: `cond_mean`
with the rounded mean, `cond_nodiv` without a division.  Otsu runs on Python ints, which have no width to overflow."""
import numpy as np

FIXED, OTSU, ADAPTIVE_MEAN = 0, 1, 2
METHODS = (FIXED, OTSU, ADAPTIVE_MEAN)
MAX_EXTENT = 255
OTSU_MAX_PIXELS = 1 << 26


def pack(px):
    """bool [..., w] -> bytes [..., ceil(w / 8)], rows MSB-first, pad bits 0."""
    return np.packbits(np.asarray(px, bool), axis=-1)


def unpack(bits, w):
    return np.unpackbits(np.asarray(bits, np.uint8), axis=-1)[..., :w].astype(bool)


def window_sums(frame, kw, kh, border="edge"):
    """S of every pixel of one frame [h, w] as int64: the kw x kh window centred on it, coordinates clamped to the frame
    (border 'edge'); 'zero' and 'reflect' exist for the mutants of the sensitivity tests only."""
    a = np.asarray(frame).astype(np.int64)
    ax, ay = kw // 2, kh // 2
    if border == "zero":
        p = np.pad(a, ((ay, ay), (ax, ax)), mode="constant")
    else:
        p = np.pad(a, ((ay, ay), (ax, ax)), mode=border)      # 'edge' is BORDER_REPLICATE; 'reflect' is BORDER_REFLECT_101
    sat = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    sat[1:, 1:] = p.cumsum(0).cumsum(1)
    h, w = a.shape
    return sat[kh:kh + h, kw:kw + w] - sat[:h, kw:kw + w] - sat[kh:kh + h, :w] + sat[:h, :w]


def cond_mean(v, S, A, c):
    """v > m - c with m = (2 S + A) // (2 A), the mean rounded half up."""
    return np.asarray(v, np.int64) > (2 * S + A) // (2 * A) - c


def cond_nodiv(v, S, A, c):
    """The division-free form: 2 S < A (2 (v + c) - 1)."""
    return 2 * S < A * (2 * (np.asarray(v, np.int64) + c) - 1)


def otsu_scores(hist):
    """score(t) for t = 0..255 as Python ints."""
    hist = [int(x) for x in hist]
    assert len(hist) == 256
    N, S = sum(hist), sum(i * x for i, x in enumerate(hist))
    w0 = s0 = 0
    scores = []
    for t in range(256):
        w0 += hist[t]
        s0 += t * hist[t]
        w1, s1 = N - w0, S - s0
        d = w1 * s0 - s1 * w0
        scores.append(0 if w0 * w1 == 0 else d * d // (w0 * w1))
    return scores


def otsu(hist):
    """The smallest t with the largest score."""
    scores = otsu_scores(hist)
    return scores.index(max(scores))


def histogram(frame):
    return np.bincount(np.asarray(frame, np.uint8).ravel(), minlength=256)


def binarize(imgs, method, thr_or_c=0, kw=3, kh=None, invert=0, form=cond_nodiv):
    """imgs uint8 [n, h, w] -> (bits uint8 [n, h, ceil(w / 8)], counts int64 [n], thresholds int32 [n])."""
    a = np.asarray(imgs, np.uint8)
    assert a.ndim == 3 and method in METHODS and invert in (0, 1)
    kh = kw if kh is None else kh
    n, h, w = a.shape
    px = np.zeros((n, h, w), bool)
    thr = np.zeros(n, np.int32)
    for f in range(n):
        if method == ADAPTIVE_MEAN:
            assert kw % 2 == 1 and kh % 2 == 1 and 3 <= kw <= MAX_EXTENT and 3 <= kh <= MAX_EXTENT and -255 <= thr_or_c <= 255
            cond = form(a[f], window_sums(a[f], kw, kh), kw * kh, thr_or_c)
            thr[f] = thr_or_c
        else:
            assert method == OTSU or -1 <= thr_or_c <= 255
            thr[f] = otsu(histogram(a[f])) if method == OTSU else thr_or_c
            cond = a[f].astype(np.int64) > int(thr[f])
        px[f] = cond != bool(invert)
    return pack(px), px.reshape(n, -1).sum(1).astype(np.int64), thr


def unit_frames(n, h, w, seed):
    """Frames whose values are {b, b + 1} at random, b per frame: with c = 1 and a 3 x 3 window one unit of S decides bits."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 255, n)
    return (base[:, None, None] + (rng.random((n, h, w)) < 0.5)).astype(np.uint8)


def blobs_on_a_ramp(h=96, w=160):
    """One frame: dark blobs (-40 grey levels, 7 x 7 and larger, 9 pixels apart at least) on a brightness ramp from 40 to
    215 from left to right, with single dark pixels of noise -> (frame uint8 [h, w], the number of blobs).  Chosen so that the
    adaptive mean with a 31 x 31 window and c = 10, opened by 3 x 3, has exactly one component per blob, and Otsu's global
    threshold -- which cuts the ramp itself -- has not."""
    ramp = (40 + (np.arange(w) * 175) // (w - 1)).astype(np.int64)
    a = np.tile(ramp, (h, 1))
    boxes = [(8, 10, 7, 7), (10, 40, 9, 11), (30, 75, 8, 8), (12, 110, 11, 9), (50, 20, 9, 9), (60, 140, 7, 10),
             (70, 60, 10, 8), (45, 105, 7, 7), (78, 100, 9, 12)]
    for y, x, bh, bw in boxes:
        a[y:y + bh, x:x + bw] -= 40
    for y, x in ((3, 70), (40, 5), (55, 90), (88, 30), (25, 150), (90, 150)):   # noise: one pixel each, far from the blobs
        a[y, x] -= 40
    return a.astype(np.uint8), len(boxes)
