"""The image pyramid rule of include/canny_hip.h in numpy: pyrDown, pyrUp, whole pyramids and the layout
of a pyramid's one buffer.  Every axis is a small integer matrix built from the rule's own words (fold; the even and odd
outputs of pyrUp), so that a plane goes through `D_h @ plane @ D_w.T` in int64 -- on purpose unlike the host rule (pixel by
pixel) and the kernels (separated, packed 16-bit halves)."""
import numpy as np

TAPS = (1, 4, 6, 4, 1)
MAX_LEVELS = 15
ALIGN = 256


def fold(p, n):
    """reflect-101: cv::BORDER_DEFAULT, scipy mode='mirror'."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def down_matrix(n):
    """int64 [(n + 1) // 2, n]: the weights of the source samples in every output sample of pyrDown along an axis of n."""
    m = np.zeros(((n + 1) // 2, n), np.int64)
    for o in range(m.shape[0]):
        for j, k in enumerate(TAPS):
            m[o, fold(2 * o + j - 2, n)] += k
    return m


def up_matrix(n, on):
    """int64 [on, n], on in (2 n - 1, 2 n): the weights of pyrUp along an axis; s[-1] := s[min(1, n - 1)], s[n] := s[n - 1]."""
    assert on in (2 * n - 1, 2 * n) and on >= 1
    at = lambda x: min(1, n - 1) if x < 0 else min(x, n - 1)
    m = np.zeros((on, n), np.int64)
    for o in range(on):
        x = o // 2
        if o % 2 == 0:
            for xx, k in ((x - 1, 1), (x, 6), (x + 1, 1)):
                m[o, at(xx)] += k
        else:
            for xx in (x, x + 1):
                m[o, at(xx)] += 4
    return m


def _planes(a):
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3
    return a.astype(np.int64)


def pyr_down(planes):
    """uint8 [n, h, w] -> uint8 [n, (h + 1) // 2, (w + 1) // 2]."""
    a = _planes(planes)
    s = down_matrix(a.shape[1]) @ a @ down_matrix(a.shape[2]).T      # one axis after the other
    assert s.max(initial=0) <= 255 * 256
    return ((s + 128) >> 8).astype(np.uint8)


def pyr_up(planes, oh, ow):
    """uint8 [n, h, w] -> uint8 [n, oh, ow]."""
    a = _planes(planes)
    s = up_matrix(a.shape[1], oh) @ a @ up_matrix(a.shape[2], ow).T
    assert s.max(initial=0) <= 255 * 64
    return ((s + 32) >> 6).astype(np.uint8)


def max_levels(h, w):
    """ceil(log2(max(h, w))): the level at which the plane is 1 x 1 for the first time."""
    return min((max(h, w) - 1).bit_length(), MAX_LEVELS)


def pyramid(planes, levels):
    """The levels 1..levels as a list of uint8 arrays."""
    assert 1 <= levels <= max_levels(*planes.shape[1:])
    out = []
    for _ in range(levels):
        planes = pyr_down(planes)
        out.append(planes)
    return out


def layout(n, h, w, levels):
    """([(h_l, w_l, off_l, bytes_l)] for l = 1..levels, total_bytes)."""
    rows, off, total = [], 0, 0
    for _ in range(levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        rows.append((h, w, off, n * h * w))
        total = off + n * h * w
        off = -(-total // ALIGN) * ALIGN
    return rows, total


def pack(levels, n, h, w, fill):
    """The levels laid out in one buffer of total_bytes, the pads holding `fill`."""
    rows, total = layout(n, h, w, len(levels))
    buf = np.full(total, fill, np.uint8)
    for lv, (hl, wl, off, nbytes) in zip(levels, rows):
        assert lv.shape == (n, hl, wl)
        buf[off:off + nbytes] = lv.reshape(-1)
    return buf


def named_planes(n, h, w, seed):
    """Frames that exercise the rule: flat, random, a 0 / 255 checkerboard; -> uint8 [n, h, w], frame f of kind f % 3."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    kinds = (lambda: np.full((h, w), int(rng.integers(0, 256)), np.uint8),
             lambda: rng.integers(0, 256, (h, w), dtype=np.uint8),
             lambda: (((yy + xx) & 1) * 255).astype(np.uint8))
    return np.stack([kinds[f % 3]() for f in range(n)])
