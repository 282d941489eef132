"""The nine loads of a hysteresis tile, in every combination, and the tile geometry at frame borders.

load_tile() (canny_kernels.hip) reads a tile's own word and up to eight halo words, each under its own condition, and takes
their bits out behind the last load; the tile's frame, row and column come from reciprocals (canny_tile_div.h) or, for the
second tile of a sweep-0 wave, from the first tile's.  The maps here make every neighbour count on its own:

  a "centre" tile and a subset of its eight neighbours.  Each neighbour of the subset holds ONE strong pixel, the pixel that
  touches the centre tile (an edge pixel for the four sides, the corner pixel for the four corners); in the centre tile a
  run of weak pixels leads from the pixel next to it to a marker pixel.  Nothing else is strong, the runs of different
  neighbours keep two pixels apart, so a marker is set exactly when its own neighbour's halo word was read, and read right.

Frame m of a batch takes subset m; neighbours that do not exist (the centre tile lies on the frame's border) are left out,
which is what the geometry has to get right there.  The oracle's maps are the reference, equality is exact, and before
anything runs on the device the oracle alone must give the sharp answer: marker k set if and only if neighbour k is in
the subset.

Routes.  The entry points that take a candidate plane are dev_hysteresis (a batch) and hysteresis() (one frame); both run
sweep 0 and then the batch-wide queue, whatever hysteresis_tail says (the option is set both ways all the same: it must not
matter).  The per-frame queues and the tail kernel are reached through canny() only, from an image; they share load_tile()
and process_tile_with() with the routes here and are driven by tests/test_gpu_hyst_push_path.py.
"""
import numpy as np
import pytest

import hyst_maps as hm
import oracle

pytestmark = pytest.mark.gpu

T = hm.T
DIRS = hm.PUSH_DIRS   # up, down, left, right, then the four corners
SENTINEL = 0x5A5A
GUARD = 256


def _chain(th, tw, d):
    """Tile-local pixels of the weak run for the neighbour in direction d, from the border inwards; the last is the marker."""
    r = min(th, tw) // 4
    a, b = tw // 2, th // 2
    dy, dx = d
    ys = [b] * r if dy == 0 else [i if dy < 0 else th - 1 - i for i in range(r)]
    xs = [a] * r if dx == 0 else [i if dx < 0 else tw - 1 - i for i in range(r)]
    return list(zip(ys, xs))


def halo_frame(shape, centre, subset):
    """-> (frame, {k: marker pixel} for the neighbours of `subset` that exist).  subset: bit k = DIRS[k]."""
    h, w = shape
    cy, cx = centre
    oy, ox = cy * T, cx * T
    th, tw = min(T, h - oy), min(T, w - ox)
    tiles_y, tiles_x = -(-h // T), -(-w // T)
    frame = np.zeros(shape, np.int16)
    markers = {}
    for k, (dy, dx) in enumerate(DIRS):
        if not (subset >> k) & 1 or not (0 <= cy + dy < tiles_y and 0 <= cx + dx < tiles_x):
            continue
        chain = _chain(th, tw, (dy, dx))
        for y, x in chain:
            frame[oy + y, ox + x] = hm.WEAK
        y0, x0 = chain[0]
        frame[oy + y0 + dy, ox + x0 + dx] = hm.STRONG   # across the border, in the neighbour tile
        markers[k] = (oy + chain[-1][0], ox + chain[-1][1])
    return frame, markers


class _Batch:
    def __init__(self, shape, centre, subsets=range(256)):
        built = [halo_frame(shape, centre, m) for m in subsets]
        self.cand = np.stack([f for f, _ in built])
        self.want = np.stack([oracle.hysteresis(f, hm.LO, hm.HI) for f in self.cand])
        # the oracle alone is sharp: a marker is set exactly where its neighbour is in the subset (and exists)
        all_markers = halo_frame(shape, centre, 255)[1]
        assert all_markers, "the centre tile has no neighbour at all"
        for m, (_, markers), want in zip(subsets, built, self.want):
            for k, p in all_markers.items():
                assert (want[p] != 0) == (k in markers), f"subset {m}: marker of neighbour {k} at {p}"
            if not markers:
                assert not want.any(), f"subset {m}: nothing is strong next to a weak pixel"
        self.full = len(all_markers)
        for a in (self.cand, self.want):
            a.flags.writeable = False


_memo = {}


def _batch(shape, centre, subsets=None):
    key = (shape, centre, None if subsets is None else tuple(subsets))
    if key not in _memo:
        _memo[key] = _Batch(shape, centre, range(256) if subsets is None else subsets)
    return _memo[key]


def _dev(ctx, cand):
    n, h, w = cand.shape
    buf = np.concatenate([np.ascontiguousarray(cand, np.int16).ravel(), np.full(GUARD, SENTINEL, np.int16)])
    d = ctx.malloc(buf.nbytes)
    try:
        ctx.h2d(d, buf)
        ctx.dev_hysteresis(d, h, w, n, hm.LO, hm.HI)
        ctx.synchronize()
        out = np.empty_like(buf)
        ctx.d2h(out, d)
    finally:
        ctx.free(d)
    assert (out[n * h * w:] == SENTINEL).all(), "dev_hysteresis wrote behind its frames"
    return out[:n * h * w].reshape(n, h, w)


def _same(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    if bad.size:
        f = int(bad[0])
        ys, xs = np.nonzero(got[f] != want[f])
        raise AssertionError(f"{what}: {bad.size} of {len(got)} frames differ from the oracle, first frame {f} in {ys.size} "
                             f"pixels, first ({ys[0]}, {xs[0]}): got {got[f][ys[0], xs[0]]}, want {want[f][ys[0], xs[0]]}")


@pytest.fixture(scope="module", params=(1, 0), ids=("tail", "no_tail"))
def ctx(hip, request):
    with hip.Context(0) as c:
        c.set_option("hysteresis_tail", request.param)
        yield c


# ---- all eight neighbours at once, every subset -----------------------------------------------------------------------
def test_every_subset_of_the_eight_neighbours_as_one_batch(ctx):
    """256 frames of 3 x 3 whole tiles, the centre tile in the middle: every combination of the loads, left + right, left +
    both left corners and none among them."""
    b = _batch((192, 192), (1, 1))
    assert b.full == 8
    _same(_dev(ctx, b.cand), b.want, "192 x 192, every subset, one batch")


def test_every_subset_of_the_eight_neighbours_frame_by_frame(ctx):
    b = _batch((192, 192), (1, 1))
    got = np.stack([ctx.hysteresis(f, hm.LO, hm.HI) for f in b.cand])
    _same(got, b.want, "192 x 192, every subset, single frames")


# ---- ragged tiles and frame borders -----------------------------------------------------------------------------------
RAGGED = (136, 200)   # 3 x 4 tiles; the last tile row is 8 pixels high, the last tile column 8 pixels wide
CENTRES = ((1, 1), (0, 0), (0, 3), (2, 0), (2, 3), (0, 1), (2, 2), (1, 0), (1, 3))


@pytest.mark.parametrize("centre", CENTRES, ids=lambda c: f"tile{c[0]}_{c[1]}")
def test_ragged_frame_with_the_centre_on_every_border(ctx, centre):
    """The centre role in the first and the last tile row and column (8-pixel tiles among them): the neighbours that do
    not exist are not read, the others are.  As one batch of 256 and, for a sample, as single frames."""
    b = _batch(RAGGED, centre)
    cy, cx = centre
    assert b.full == [8, 5, 3][(cy in (0, 2)) + (cx in (0, 3))]   # neighbours inside the frame
    _same(_dev(ctx, b.cand), b.want, f"{RAGGED}, centre {centre}, one batch")
    pick = (0, 255, 0x0F, 0xF0, 0x55, 0xAA, 0x3C, 0xC3)
    got = np.stack([ctx.hysteresis(b.cand[m], hm.LO, hm.HI) for m in pick])
    _same(got, b.want[list(pick)], f"{RAGGED}, centre {centre}, single frames")


def test_wave_of_sweep_0_straddles_the_end_of_a_tile_row(ctx):
    """A frame of 3 x 3 tiles: sweep 0 gives a wave two consecutive tiles, so tiles (0,2) | (1,0), and in the next frame
    of a batch (2,2) | next frame's (0,0), share a wave -- every tile takes the centre role in turn, with all the neighbours
    it has, in a batch of three frames whose tile count (27) is odd: the last wave of sweep 0 has one tile."""
    for centre in [(y, x) for y in range(3) for x in range(3)]:
        one = _batch((192, 192), centre, subsets=(255,))
        for n in (1, 3):   # 9 and 27 tiles: both odd
            cand = np.repeat(one.cand, n, axis=0)
            _same(_dev(ctx, cand), np.repeat(one.want, n, axis=0), f"192 x 192, centre {centre}, {n} frames")


def test_odd_tile_count_with_every_subset(ctx):
    """255 frames of 3 x 3 tiles: 2295 tiles, an odd number, and from frame 1 on a frame's first tile is the SECOND tile
    of its wave in every other frame."""
    b = _batch((192, 192), (1, 1))
    _same(_dev(ctx, b.cand[1:]), b.want[1:], "192 x 192, subsets 1..255")
