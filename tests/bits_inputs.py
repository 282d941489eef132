"""Packed bit maps as a caller may hand them to the dev_*_bits entry points (include/canny_hip.h: rows MSB-first and padded
to bytes, any byte address, the padding bits of a row ignored whatever they hold), for tests/test_gpu_bits_inputs.py.

Two halves.  The first needs numpy only: masks designed so that a reader that trusts a pad bit changes the answer, the pad
variants of a packed map, and the widened data of the CPU control (the pad columns counted as pixels).  The second puts a
map into one larger device allocation -- `shift` filler bytes, the map, at least 64 filler bytes -- so that every over-read
and every read from a rounded-down address lands in filler of the same allocation, never outside it, and checks afterwards
that nothing of it was written."""
import numpy as np

SHIFTS = (0, 1, 3, 7)                 # the address modulo 2, 4 and 8 takes odd residues
PADS = ("clean", "ones", "random")
TAIL = 64                             # filler bytes behind the map, at least
# n x h x w: the smallest shapes at which word, byte and frame boundaries move
SHAPES = [(3, 37, 69),     # row_bytes 9; the second 64-pixel word holds 5 pixels and 3 pad bits; h * row_bytes is odd
          (2, 33, 129),    # row_bytes 17; the third word holds one pixel and seven pad bits
          (2, 50, 63),     # one word, one pad bit
          (2, 9, 2),       # six pad bits, a single partial byte
          (2, 40, 64)]     # no pad bits, shift only: separates an address slip from a pad slip
SHAPE_IDS = [f"{n}x{h}x{w}" for n, h, w in SHAPES]


def row_bytes(w):
    return (w + 7) // 8


def pad_bits(w):
    return 8 * row_bytes(w) - w


def placements(w):
    """(shift, filler byte, pad setting) of every call of one case: all shifts under all pad settings in 0xFF filler, and
    once in 0x00 filler.  A width without pad bits has one pad setting."""
    pads = PADS if pad_bits(w) else PADS[:1]
    return [(s, 0xFF, p) for p in pads for s in SHIFTS] + [(3, 0x00, pads[-1])]


def packed(masks, pad, seed=0):
    """np.packbits(masks, axis=-1) with only the pad bits changed: left clean, all set, or random (then column w is set
    where the map's last column is, so that whatever the draw a pad bit lengthens every run that ends there)."""
    masks = np.asarray(masks, bool)
    bits = np.packbits(masks, axis=-1)
    k = pad_bits(masks.shape[-1])
    if pad == "clean" or not k:
        return bits
    pm = np.uint8((1 << k) - 1)
    if pad == "ones":
        bits[..., -1] |= pm
    else:
        assert pad == "random"
        r = np.random.default_rng(1000 + seed).integers(0, 256, bits.shape[:-1], dtype=np.uint8) & pm
        r.reshape(-1)[::3] &= np.uint8(pm >> 1)            # column w clear in every third row ...
        r |= masks[..., -1].astype(np.uint8) << (k - 1)     # ... and set where it continues a run that ends on column w - 1
        bits[..., -1] |= r
    return bits


def widened(bits):
    """The map a reader sees that counts the pad columns as pixels: bool [..., 8 * row_bytes]."""
    return np.unpackbits(bits, axis=-1).astype(bool)


def widened_plane(plane, w8):
    """A plane [..., h, w] continued to w8 columns by edge replication."""
    extra = w8 - plane.shape[-1]
    return np.pad(plane, [(0, 0)] * (plane.ndim - 1) + [(0, extra)], mode="edge") if extra else plane


def yx(indices, width):
    """Pixel indices r * width + c as (r, c) pairs: the form in which results at two widths can be compared."""
    a = np.asarray(indices).astype(np.int64)
    return np.stack([a // width, a % width], axis=-1)


def differ(a, b):
    """Whether two tuples of arrays differ in at least one member (another shape is a difference)."""
    assert len(a) == len(b)
    return any(np.shape(x) != np.shape(y) or not np.array_equal(x, y) for x, y in zip(a, b))


# ---- masks ------------------------------------------------------------------------------------------------------------
def _texture(n, h, w, seed):
    """Random texture at densities around 0.05 and 0.3, frame by frame in turn."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random((h, w)) < (0.05, 0.3, 0.1)[f % 3] for f in range(n)])


def _right_border(m):
    """Rows where column w - 1 is clear (the first and the last) whatever the texture put there."""
    m[:, 0, -1] = m[:, -1, -1] = False
    return m


def line_masks(n, h, w, seed=1):
    """Texture, a vertical line on column w - 1 over rows 1 .. h - 2 (a full phantom column beside it outvotes it), a
    horizontal line through the middle that ends on column w - 1 (a set pad bit lengthens its run) and a diagonal that
    ends in the last column."""
    m = _texture(n, h, w, seed)
    m[:, 1:h - 1, w - 1] = True
    m[:, h // 2, :] = True
    d = min(h, w)
    for f in range(n):
        i = np.arange(d - f)
        m[f, h - 1 - i - f, w - d + i + f] = True     # rises to (h - d, w - 1); it starts one step further on per frame
    return _right_border(m)


def ring(h, w, cx, cy, r, a0=0.0, a1=360.0):
    """The pixels within half a pixel of the circle (cx, cy, r) between the angles a0 and a1 (degrees)."""
    yy, xx = np.mgrid[:h, :w]
    d = np.hypot(xx - cx, yy - cy)
    ang = np.degrees(np.arctan2(yy - cy, xx - cx)) % 360.0
    return (np.abs(d - r) <= 0.5) & (ang >= a0) & (ang <= a1)


def circle_of(h, w):
    """(cx, cy, r) of the designed circle: it touches the right border in column w - 1."""
    r = max(1, min(12, (h - 3) // 2, w - 1))
    return w - 1 - r, h // 2, r


def circle_masks(n, h, w, seed=2):
    """Texture and an arc (the right three quarters of the circle in the odd frames, all of it in the even ones) whose
    circle touches the right border."""
    m = _texture(n, h, w, seed)
    cx, cy, r = circle_of(h, w)
    for f in range(n):
        m[f] |= ring(h, w, cx, cy, r) if f % 2 == 0 else (ring(h, w, cx, cy, r, 0, 135) | ring(h, w, cx, cy, r, 225, 360))
    m[:, cy, w - 1] = True
    return _right_border(m)


def blob_masks(n, h, w, seed=3):
    """Texture, a box outline whose right side lies on column w - 1 (a set pad bit beside it joins the component, moves a
    hull and a polygon vertex) and single pixels on column w - 1 further down."""
    m = _texture(n, h, w, seed)
    a, b = h // 5, max(h // 5 + 2, h // 2)
    x0 = max(0, w - 1 - min(w - 1, 9))
    m[:, a, x0:] = m[:, b, x0:] = True
    m[:, a:b + 1, w - 1] = m[:, a:b + 1, x0] = True
    m[:, b + 2:h - 1:3, w - 1] = True
    return _right_border(m)


def chamfer_templates(h, w):
    """The template list of a shape: rings where they fit, a few points where the frame is only two columns wide."""
    import chamfer_rule
    if min(h, w) < 9:
        return [np.array([[0, 0]], np.int16), np.array([[0, 0], [0, 1], [-1, 2]], np.int16)]
    return [chamfer_rule.ring_template(3), np.array([[0, 0], [2, 1], [-3, 4], [5, -2], [-1, -4]], np.int16),
            chamfer_rule.ring_template(5)]


def chamfer_masks(n, h, w, seed=4):
    """Texture and one template (the first ring, or the three points of a two-column frame) drawn with its bounding box
    touching the right border: the best match (score 0) lies there."""
    rng = np.random.default_rng(seed)
    m = np.stack([rng.random((h, w)) < (0.05, 0.02, 0.3)[f % 3] for f in range(n)])
    tpl = chamfer_templates(h, w)[0 if min(h, w) >= 9 else 1].astype(np.int64)
    ax, ay = w - 1 - int(tpl[:, 0].max()), h // 2 - int(tpl[:, 1].max()) // 2
    m[:, max(ay - 5, 0):ay + 6, max(w - 10, 0):] = False    # the drawn template stands alone
    m[:, ay + tpl[:, 1], ax + tpl[:, 0]] = True
    return _right_border(m)


def planes_for(masks, dtype, seed=5):
    """Planes [n, h, w] for the fit stages: a blurred step along every mask pixel's neighbourhood plus noise, so that the
    edgels of the map's pixels have gradients in every direction; uint8, or int16 over a range that needs 16 bits."""
    n, h, w = masks.shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = 90.0 + 70.0 * np.sin(xx / 3.1) * np.cos(yy / 4.3) + 40.0 * (xx > (w * 3) // 4)
    p = np.clip(base[None] + rng.integers(-12, 13, (n, h, w)) + 30 * masks, 0, 255)
    if dtype == np.uint8:
        return p.astype(np.uint8)
    return (p.astype(np.int32) * 37 - 4000).astype(np.int16)


# ---- placement on the device ---------------------------------------------------------------------------------------------
class Placed:
    """A packed map inside one device allocation: `shift` filler bytes, the map, TAIL or more filler bytes (the total a
    multiple of 16).  ptr = base + shift.  unchanged() downloads the whole allocation and compares it with the upload."""

    def __init__(self, ctx, bits, shift, filler):
        bits = np.ascontiguousarray(bits, np.uint8)
        total = -(-(shift + bits.size + TAIL) // 16) * 16
        self.host = np.full(total, filler, np.uint8)
        self.host[shift:shift + bits.size] = bits.reshape(-1)
        self.ctx, self.shift, self.size = ctx, shift, bits.size
        self.base = ctx.malloc(total)
        ctx.h2d(self.base, self.host)
        self.ptr = self.base + shift

    def unchanged(self, what):
        got = np.empty_like(self.host)
        self.ctx.d2h(got, self.base)
        a, b = self.shift, self.shift + self.size
        assert np.array_equal(got[:a], self.host[:a]), f"{what}: the filler in front of the map was written"
        assert np.array_equal(got[a:b], self.host[a:b]), f"{what}: the caller's map was written"
        assert np.array_equal(got[b:], self.host[b:]), f"{what}: the filler behind the map was written"

    def free(self):
        self.ctx.free(self.base)


class Outputs:
    """Device output arrays of one call, pre-filled with a sentinel byte pattern and followed by guard words; raw() gives
    every byte back, the guards included, so that one comparison covers the payload, the unused slots and the guards."""
    FILL, GUARD = 0xA5, 64

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, {}

    def add(self, key, count, dtype):
        nbytes = int(count) * np.dtype(dtype).itemsize + self.GUARD
        p = self.ctx.malloc(nbytes)
        self.bufs[key] = (p, nbytes)
        return p

    def up(self, key, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        if a.nbytes:
            self.ctx.h2d(p, a)
        self.bufs["in:" + key] = (p, 0)
        return p

    def refill(self):
        for p, nbytes in self.bufs.values():
            if nbytes:
                self.ctx.h2d(p, np.full(nbytes, self.FILL, np.uint8))

    def raw(self):
        out = {}
        for key, (p, nbytes) in self.bufs.items():
            if nbytes:
                out[key] = np.empty(nbytes, np.uint8)
                self.ctx.d2h(out[key], p)
        return out

    def free(self):
        for p, _ in self.bufs.values():
            self.ctx.free(p)
        self.bufs = {}


def expected_bytes(count, dtype, payload):
    """What Outputs.raw() must hold for an output of `count` elements whose first elements are `payload` (flattened) and
    whose remaining slots and guard are untouched."""
    nbytes = int(count) * np.dtype(dtype).itemsize + Outputs.GUARD
    out = np.full(nbytes, Outputs.FILL, np.uint8)
    p = np.ascontiguousarray(payload).astype(dtype, copy=False).reshape(-1)
    assert p.size <= count
    out[:p.nbytes] = p.view(np.uint8)
    return out


def put(buf, dtype, at, payload):
    """Overwrite elements [at, at + len) of an expected_bytes() buffer."""
    p = np.ascontiguousarray(payload).astype(dtype, copy=False).reshape(-1)
    a = int(at) * np.dtype(dtype).itemsize
    buf[a:a + p.nbytes] = p.view(np.uint8)
