"""The temporal-fusion rule of include/canny_hip.h restated in numpy and plain Python ints: the judge of
the host C++ (csrc/canny_fuse_host.cpp) and of the kernels (csrc/canny_fuse.hip).  `fuse` and `change_mask` work on whole
stacks with a sort along the time axis; `fuse_pixel` is the same rule for one pixel in Python ints."""
import numpy as np

MEAN, MEDIAN, MIN, MAX = 0, 1, 2, 3
OPS = (MEAN, MEDIAN, MIN, MAX)
MAX_GROUP = 255
MEAN_ROW = 255 * 255 + 1


def row_bytes(w):
    return (w + 7) // 8


def pack_bits(plane_bool):
    """bool [..., w] -> bit maps uint8 [..., ceil(w / 8)], rows MSB-first, pad bits 0."""
    return np.packbits(np.asarray(plane_bool, bool), axis=-1)


def unpack_bits(bits, w):
    """bit maps -> bool [..., w]; the pad bits are dropped, whatever they hold."""
    return np.unpackbits(np.asarray(bits, np.uint8), axis=-1)[..., :w].astype(bool)


def n_groups(n_frames, group_len, group_step):
    return (n_frames - group_len) // group_step + 1


def mean_of(s, c):
    """Python ints: the rounded mean of c samples with sum s."""
    return (2 * s + c) // (2 * c)


def fuse_pixel(values, op, fill=0, min_count=1):
    """values: the VALID samples of one pixel's window (Python ints) -> (result, count)."""
    c = len(values)
    if c < min_count:
        return fill, c
    v = sorted(values)
    if op == MEAN:
        return mean_of(sum(v), c), c
    return (v[(c - 1) >> 1] if op == MEDIAN else (v[0] if op == MIN else v[c - 1])), c


def fuse(frames, valid_bits, group_len, group_step, op, fill=0, min_count=1):
    """frames uint8 [n, h, w], valid_bits uint8 [n, h, ceil(w / 8)] or None -> (fused uint8 [g, h, w], count uint8 [g, h, w])."""
    frames = np.asarray(frames, np.uint8)
    n, h, w = frames.shape
    assert 1 <= group_len <= min(n, MAX_GROUP) and group_step >= 1 and op in OPS and 0 <= fill <= 255 and 1 <= min_count <= 255
    valid = np.ones((n, h, w), bool) if valid_bits is None else unpack_bits(valid_bits, w)
    g = n_groups(n, group_len, group_step)
    fused, count = np.zeros((g, h, w), np.uint8), np.zeros((g, h, w), np.uint8)
    for k in range(g):
        sl = slice(k * group_step, k * group_step + group_len)
        S, V = frames[sl].astype(np.int64), valid[sl]
        c = V.sum(0).astype(np.int64)
        srt = np.sort(np.where(V, S, 256), axis=0)            # the invalid samples behind every valid one
        if op == MEAN:
            s = np.where(V, S, 0).sum(0)
            out = (2 * s + c) // (2 * np.maximum(c, 1))
        else:
            rank = ((c - 1) >> 1) if op == MEDIAN else (np.zeros_like(c) if op == MIN else c - 1)
            out = np.take_along_axis(srt, np.maximum(rank, 0)[None], axis=0)[0]
        fused[k] = np.where(c < min_count, fill, out).astype(np.uint8)
        count[k] = c.astype(np.uint8)
    return fused, count


def change_mask(frames, valid_bits, background, bg_count, frames_per_background, thr, min_count=1):
    """-> (mask bit maps uint8 [n, h, ceil(w / 8)] with pad bits 0, changed int64 [n])."""
    frames = np.asarray(frames, np.uint8)
    n, h, w = frames.shape
    assert frames_per_background >= 1 and 0 <= thr <= 255 and 1 <= min_count <= 255
    background = np.asarray(background, np.uint8).reshape(-1, h, w)
    assert len(background) == -(-n // frames_per_background)
    which = np.arange(n) // frames_per_background
    on = np.abs(frames.astype(np.int64) - background[which].astype(np.int64)) > thr
    if valid_bits is not None:
        on &= unpack_bits(valid_bits, w)
    if bg_count is not None:
        on &= np.asarray(bg_count, np.uint8).reshape(-1, h, w)[which] >= min_count
    return pack_bits(on), on.reshape(n, -1).sum(1).astype(np.int64)


def mean_table():
    """What canny_hip_selftest_fuse_mean must return: uint8 [255, MEAN_ROW], row c - 1, cell s <= 255 c; the rest 0."""
    t = np.zeros((255, MEAN_ROW), np.uint8)
    for c in range(1, 256):
        s = np.arange(255 * c + 1, dtype=np.int64)
        t[c - 1, :len(s)] = (2 * s + c) // (2 * c)
    return t


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 67, 257)
HEIGHTS = (1, 2, 15, 16, 17, 33)
GROUP_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 255)
VALID = ("null", "ones", "zeros", "half", "sparse", "single", "dirty")
VALUES = ("random", "extremes", "ties", "constant", "ascending", "descending")


def values(kind, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if kind == "extremes":
        return (rng.integers(0, 2, (n, h, w)) * 255).astype(np.uint8)
    if kind == "ties":
        return rng.integers(7, 9, (n, h, w), dtype=np.uint8)
    if kind == "constant":
        return np.full((n, h, w), 93, np.uint8)
    ramp = (np.arange(n) * 3 + 1) % 256
    ramp = ramp if kind == "ascending" else ramp[::-1]
    return np.broadcast_to(ramp.astype(np.uint8)[:, None, None], (n, h, w)).copy()


def valid_bits(kind, n, h, w, seed):
    """None or bit maps uint8 [n, h, ceil(w / 8)]."""
    rng = np.random.default_rng(seed + 7)
    if kind == "null":
        return None
    if kind == "ones":
        return np.full((n, h, row_bytes(w)), 0xFF, np.uint8)          # pad bits set too
    if kind == "zeros":
        return np.zeros((n, h, row_bytes(w)), np.uint8)
    if kind == "single":
        v = np.zeros((n, h, w), bool)
        v[min(1, n - 1)] = True
        return pack_bits(v)
    bits = pack_bits(rng.random((n, h, w)) < (0.05 if kind == "sparse" else 0.5))
    if kind == "dirty" and w % 8:
        bits[..., -1] |= (1 << (8 - w % 8)) - 1                           # every pad bit 1
    return bits


def moving_object(h=40, w=70, seed=31):
    """Three copies of a random background in 0..199 with a 6 x 9 patch raised by 50 at three disjoint places, one per frame."""
    bg = np.random.default_rng(seed).integers(0, 200, (h, w), dtype=np.uint8)
    frames, patch = np.stack([bg] * 3), np.zeros((3, h, w), bool)
    for f, (y, x) in enumerate(((3, 5), (20, 30), (31, 58))):
        patch[f, y:y + 6, x:x + 9] = True
    frames[patch] += 50
    return bg, frames, patch
