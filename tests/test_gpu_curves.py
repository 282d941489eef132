"""Edge curves on the GPU (canny_hip_dev_canny_curves / canny_hip_dev_curves_bits / canny_hip_canny_curves): the edge map
linked into ordered chains -- every edge pixel once, in order along its curve, curves split at junctions -- CSR-shaped on
two levels over the batch, like the contour chains.

Reference: oracle.canny per frame -> the plain-Python rule of tests/curves_rule.py.  Everything is integers, equality is
exact.  offsets, point_offsets, chain_offsets, points and records are checked separately so that a failure names which.
Every output buffer is pre-filled with a pattern and followed by guard words."""
import numpy as np
import pytest

import components_rule as cr
import curves_rule as rule
import edgels_rule as er
import oracle
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

GUARD32 = np.int32(0x5A5A5A5A)
N_GUARD = 64
OFF_FILL = np.uint64(0xEEEEEEEEEEEEEEEE)
SHAPES = [(37, 53), (9, 2), (2, 9), (64, 8), (120, 1001), (270, 480)]
MIN_LENGTHS = [1, 3, 10]

_cache = {}


def _frames(n, h, w, seed0):
    return np.stack([synth_frame(h, w, seed0 + i) for i in range(n)])


def _oracle_maps(frames, sigma, lo, hi, key):
    k = ("maps", key, frames.shape, sigma, lo, hi)
    if k not in _cache:
        _cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _cache[k]


def _want(maps, min_length, key):
    """rule.csr of the maps, computed once per (key, min_length) and shared."""
    k = ("csr", key, maps.shape, min_length)
    if k not in _cache:
        _cache[k] = rule.csr(maps, min_length)
    return _cache[k]


class _Dev:
    """Device buffers of one curves call.  source: frames uint8 [n, h, w] (the canny route) or, with bits=True, packed
    bit maps [n, h, ceil(w / 8)] placed `shift` bytes into their allocation."""

    def __init__(self, ctx, source, capacity, point_capacity, h=None, w=None, bits=False, shift=0, records=True, chain=True,
                 points=True, edges=False):
        self.ctx, self.capacity, self.point_capacity, self.bits = ctx, int(capacity), int(point_capacity), bits
        self.n = source.shape[0]
        self.h, self.w = (h, w) if bits else source.shape[1:]
        self.npx = self.n * self.h * self.w
        self.ptrs = []
        self.d_src = self._malloc(source.nbytes + shift + 16) + shift
        ctx.h2d(self.d_src, source)
        self.d_rec = self._filled(np.full((self.capacity + N_GUARD) * 4, GUARD32, np.int32)) if records else 0
        self.d_chain = self._filled(np.full(self.capacity + 1 + N_GUARD, OFF_FILL, np.uint64)) if chain else 0
        self.d_points = self._filled(np.full(self.point_capacity + N_GUARD, GUARD32, np.int32)) if points else 0
        self.d_off = self._filled(np.full(self.n + 1, OFF_FILL, np.uint64))
        self.d_poff = self._filled(np.full(self.n + 1, OFF_FILL, np.uint64))
        self.d_edges = self._filled(np.full(self.npx, 0x5A5A, np.int16)) if edges else 0

    def _malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def _filled(self, a):
        p = self._malloc(a.nbytes)
        self.ctx.h2d(p, a)
        return p

    def run(self, min_length, sigma=None, lo=None, hi=None):
        cap = self.capacity if self.d_chain else 0
        pcap = self.point_capacity if self.d_points else 0
        if self.bits:
            self.ctx.dev_curves_bits(self.d_src, self.h, self.w, self.n, min_length, self.d_rec, cap, self.d_off,
                                     self.d_chain, self.d_points, pcap, self.d_poff)
        else:
            self.ctx.dev_canny_curves(self.d_src, sigma, lo, hi, self.h, self.w, self.n, min_length, self.d_rec, cap,
                                      self.d_off, self.d_chain, self.d_points, pcap, self.d_poff, self.d_edges)

    def get(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        self.ctx.d2h(out, ptr)
        return out

    def raw(self):
        """Every output buffer, guards included, as bytes (for the run-to-run comparison)."""
        out = [self.get(self.d_off, self.n + 1, np.uint64), self.get(self.d_poff, self.n + 1, np.uint64)]
        if self.d_rec:
            out.append(self.get(self.d_rec, (self.capacity + N_GUARD) * 4, np.int32))
        if self.d_chain:
            out.append(self.get(self.d_chain, self.capacity + 1 + N_GUARD, np.uint64))
        if self.d_points:
            out.append(self.get(self.d_points, self.point_capacity + N_GUARD, np.int32))
        return tuple(a.tobytes() for a in out)

    def edges(self):
        return self.get(self.d_edges, self.npx, np.int16).reshape(self.n, self.h, self.w)

    def check(self, want, what):
        """want = rule.csr(...): every output that exists against it, each named."""
        w_rec, w_off, w_chain, w_points, w_poff = want
        got = self.get(self.d_off, self.n + 1, np.uint64)
        assert np.array_equal(got, w_off), f"{what}: offsets are not the true counts"
        got = self.get(self.d_poff, self.n + 1, np.uint64)
        assert np.array_equal(got, w_poff), f"{what}: point_offsets are not the true counts"
        K = int(w_off[-1])
        fit = min(K, self.capacity) if self.d_chain else 0
        if self.d_chain:
            got = self.get(self.d_chain, self.capacity + 1 + N_GUARD, np.uint64)
            assert np.array_equal(got[:fit + 1], w_chain[:fit + 1]), f"{what}: chain_offsets differ"
            assert np.all(got[fit + 1:] == OFF_FILL), f"{what}: written past the chain offsets that exist"
            for f in range(self.n + 1):
                if int(w_off[f]) <= fit:
                    assert got[int(w_off[f])] == w_poff[f], f"{what}: point_offsets[{f}] != chain_offsets[offsets[{f}]]"
        if self.d_points:
            got = self.get(self.d_points, self.point_capacity + N_GUARD, np.int32)
            pfit = min(self.point_capacity, int(w_chain[fit]))
            assert np.array_equal(got[:pfit], w_points[:pfit]), f"{what}: points differ"
            assert np.all(got[pfit:] == GUARD32), f"{what}: written past the points that fit"
        if self.d_rec:
            got = self.get(self.d_rec, (self.capacity + N_GUARD) * 4, np.int32)
            assert np.array_equal(got[:fit * 4].reshape(fit, 4), w_rec[:fit]), f"{what}: records differ"
            assert np.all(got[fit * 4:] == GUARD32), f"{what}: written past the records that fit"

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_bits_call(ctx, masks, min_length, what, want=None, shift=0, pad_ones=False, capacity=None, point_capacity=None,
                     **outs):
    n, h, w = masks.shape
    bits = np.packbits(masks, axis=-1)
    if pad_ones and w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want = rule.csr(masks, min_length) if want is None else want
    cap = want[0].shape[0] if capacity is None else capacity
    pcap = want[3].size if point_capacity is None else point_capacity
    with _Dev(ctx, bits, cap, pcap, h=h, w=w, bits=True, shift=shift, **outs) as d:
        d.run(min_length)
        d.check(want, what)
    return want


# ---- the canny route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_length", MIN_LENGTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_curves_match_the_rule_on_the_oracles_maps(hip, shape, min_length):
    h, w = shape
    frames = _frames(3, h, w, 300 + h + w)
    maps = _oracle_maps(frames, 1.4, 50, 150, "main")
    want = _want(maps, min_length, "main")
    what = f"{shape} min_length={min_length}"
    with hip.Context(0) as ctx:
        for edges in (True, False):
            with _Dev(ctx, frames, want[0].shape[0], want[3].size, edges=edges) as d:
                d.run(min_length, 1.4, 50, 150)
                d.check(want, f"{what} d_edges={edges}")
                if edges:
                    assert np.array_equal(d.edges(), maps), f"{what}: the s16 map differs from the oracle"


# ---- the bits route --------------------------------------------------------------------------------------------------------
def _stacked():
    """The designed and the random maps as one batch of 70 x 72 frames, each map in the top-left corner of its frame (the
    1 x 70 and 70 x 1 maps keep their line; frames that are one pixel wide or high have a test of their own)."""
    if "stacked" not in _cache:
        maps = dict(rule.designed_maps())
        maps.update(rule.random_maps(seeds=(0,)))
        _cache["stacked"] = (list(maps), np.stack([rule.embed(m, 70, 72) for m in maps.values()]))
    return _cache["stacked"]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_designed_and_random_maps_through_the_bits_route(hip, order):
    names, masks = _stacked()
    if order == "reversed":
        names, masks = names[::-1], masks[::-1]
    with hip.Context(0) as ctx:
        for min_length in MIN_LENGTHS:
            want = _check_bits_call(ctx, masks, min_length, f"stacked {order} min_length={min_length}", pad_ones=True)
            if min_length == 1:
                counts = dict(zip(names, np.diff(want[1]).astype(int)))
                assert counts["square_ring"] == counts["diamond_ring"] == counts["sawtooth_ring"] == 1
                assert counts["plus"] == counts["x"] == 4 and counts["t"] == 3 and counts["figure_eight"] == 2
                flags = want[0][:, rule.FLAGS]
                assert (flags & rule.CLOSED).any() and (flags & rule.ISOLATED).any() and (flags & rule.END_JUNCTION).any()


def test_frames_one_pixel_wide_or_high(hip):
    with hip.Context(0) as ctx:
        for h, w in ((1, 1), (1, 70), (70, 1), (1, 130), (9, 2)):
            rng = np.random.default_rng(h * 1000 + w)
            masks = np.stack([np.ones((h, w), bool), rng.random((h, w)) < 0.6, rng.random((h, w)) < 0.3])
            for min_length in (1, 3):
                _check_bits_call(ctx, masks, min_length, f"{h}x{w} min_length={min_length}", pad_ones=True)


def test_directed_masks_through_the_bits_route(hip):
    with hip.Context(0) as ctx:
        for h, w in ((64, 72), (9, 2), (130, 200)):
            named = cr.directed_masks(h, w)
            masks = np.stack(list(named.values()))
            _check_bits_call(ctx, masks, 1, f"directed {h}x{w}: {list(named)}", pad_ones=True)


def test_lines_that_cross_the_64_column_chunks(hip):
    def lines(h, w):
        m = np.zeros((4, h, w), bool)
        m[0, h // 2, :] = True                                  # one straight line through every chunk
        m[1, h // 2, 3:w - 3] = True
        m[1, :, w // 2] = True                                  # ... crossed by another: a junction
        for i in range(min(h, w)):                              # a diagonal, and a zigzag over the chunk border
            m[2, i, i] = True
        for x in range(w):
            m[3, (h // 2 + (x & 1)) % h, x] = True
        return m

    with hip.Context(0) as ctx:
        for h, w in ((3, 200), (200, 3), (5, 129), (3, 4230)):   # the last: more than 64 chunks a row
            for min_length in (1, 10):
                _check_bits_call(ctx, lines(h, w), min_length, f"lines {h}x{w} min_length={min_length}", pad_ones=True)


def test_frames_never_see_each_other(hip):
    h, w = 6, 70
    masks = np.zeros((3, h, w), bool)
    masks[0, h - 1, 2:60] = True          # a line on the last row of one frame ...
    masks[1, 0, 3:61] = True              # ... above a line on the first row of the next
    masks[1, h - 1, :] = True
    masks[2, 0, ::2] = True
    with hip.Context(0) as ctx:
        want = _check_bits_call(ctx, masks, 1, "frame isolation")
        assert np.diff(want[1]).tolist() == [1, 2, 35] and want[0][0, rule.POINTS] == 58


@pytest.mark.parametrize("density", [0.05, 0.35, 0.9])
def test_random_masks_at_odd_byte_addresses(hip, density):
    with hip.Context(0) as ctx:
        for h, w in ((37, 53), (66, 129)):
            masks = np.random.default_rng(17 * h + w).random((3, h, w)) < density
            for min_length in (1, 3):
                want = rule.csr(masks, min_length)
                for shift in (1, 3):   # an odd byte address, padding bits set
                    _check_bits_call(ctx, masks, min_length, f"({h},{w}) density={density} min_length={min_length} "
                                     f"shift={shift}", want=want, shift=shift, pad_ones=True)


def test_the_long_single_curve(hip):
    m = cr.serpentine(256, 256)[None]
    with hip.Context(0) as ctx:
        want = _check_bits_call(ctx, m, 1, "serpentine(256, 256)")
        assert want[0].shape[0] == 1 and want[3].size == int(m.sum())


# ---- capacities and options ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_length", [1, 4])
def test_capacities_bound_the_writes_never_the_counts(hip, min_length):
    frames = _frames(3, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150, "capacity")
    want = _want(maps, min_length, "capacity")
    w_chain = want[2]
    K, P = want[0].shape[0], want[3].size
    assert K > 8 and P > K
    j = int(np.argmax(np.diff(w_chain)))
    mid = int(w_chain[j]) + int(w_chain[j + 1] - w_chain[j]) // 2
    assert w_chain[j] < mid < w_chain[j + 1], "lands inside a chain"
    with hip.Context(0) as ctx:
        for cap, pcap in ((K, P), (K // 2, P // 2), (K - 1, P), (1, P), (0, P), (K, mid), (K, 1), (K, 0), (K - 1, mid),
                          (K + 9, P + 9)):
            with _Dev(ctx, frames, cap, pcap) as d:   # capacity 0 WITH real buffers: nothing may be written to them
                d.run(min_length, 1.4, 50, 150)
                d.check(want, f"capacity={cap} point_capacity={pcap}")
        with _Dev(ctx, frames, K, P, records=False) as d:
            d.run(min_length, 1.4, 50, 150)
            d.check(want, "records NULL")
        with _Dev(ctx, frames, 0, 0, records=False, chain=False, points=False) as d:
            d.run(min_length, 1.4, 50, 150)
            d.check(want, "counts only")
        # the designed maps hold closed curves and junctions: a chain cut midway, half the records
        names, masks = _stacked()
        sw = rule.csr(masks, min_length)
        _check_bits_call(ctx, masks, min_length, "bits, halved", want=sw, capacity=sw[0].shape[0] // 2,
                         point_capacity=sw[3].size // 2)
        _check_bits_call(ctx, masks, min_length, "bits, a chain cut", want=sw, point_capacity=sw[3].size // 3)
        _check_bits_call(ctx, masks, min_length, "bits, counts only", want=sw, capacity=0, point_capacity=0,
                         records=False, chain=False, points=False)
        # a capacity without its buffer is an argument error, and nothing is written
        for kw in (dict(chain=False), dict(points=False)):
            with _Dev(ctx, frames, K, P, **kw) as d:
                with pytest.raises(hip.CannyHipError) as ei:
                    ctx.dev_canny_curves(d.d_src, 1.4, 50, 150, d.h, d.w, d.n, min_length, d.d_rec, K, d.d_off, d.d_chain,
                                         d.d_points, P, d.d_poff, 0)
                assert ei.value.status == 1
                ctx.synchronize()
                assert np.all(d.get(d.d_off, d.n + 1, np.uint64) == OFF_FILL)
                assert np.all(d.get(d.d_poff, d.n + 1, np.uint64) == OFF_FILL)
                assert np.all(d.get(d.d_rec, (K + N_GUARD) * 4, np.int32) == GUARD32)


def test_max_val_above_255_follows_the_map(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300, "hi300")
    assert not maps.any(), "the oracle's map is all zero for max_val = 300"
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 64, 64, edges=True) as d:
            d.run(1, 1.0, 50, 300)
            d.check(rule.csr(maps, 1), "max_val=300")
            assert np.array_equal(d.edges(), maps)
        r, off, chain, pts, poff = ctx.canny_curves(frames, 1.0, 50, 300)
        assert r.shape == (0, 4) and not off.any() and not poff.any() and pts.size == 0 and chain.tolist() == [0]


def test_a_rejected_call_writes_nothing(hip):
    frames = _frames(2, 64, 64, 9)
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 256, 1024, edges=True) as d:
            before = d.raw()
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1, 1.0, 300, 100)
            assert ei.value.status == 5   # CANNY_HIP_ERR_DOMAIN, dev_canny's own
            ctx.synchronize()
            assert d.raw() == before and np.all(d.edges() == 0x5A5A)


# ---- determinism, the host form, a long-lived context ----------------------------------------------------------------------
def test_same_bytes_on_every_run_and_the_host_form(hip):
    frames = _frames(4, 270, 480, 77)
    maps = _oracle_maps(frames, 1.4, 50, 150, "determinism")
    want = _want(maps, 2, "determinism")
    K, P = want[0].shape[0], want[3].size
    names, masks = _stacked()
    sw = rule.csr(masks, 1)
    with hip.Context(0) as ctx:
        runs, bit_runs = [], []
        for k in range(3):
            if k == 2:   # an unrelated call on the context in between
                ctx.canny_points(_frames(2, 96, 256, 1), 1.4, 50, 150)
            with _Dev(ctx, frames, K, P) as d:
                d.run(2, 1.4, 50, 150)
                if k == 0:
                    d.check(want, "first run")
                runs.append(d.raw())
            with _Dev(ctx, np.packbits(masks, axis=-1), sw[0].shape[0], sw[3].size, h=70, w=72, bits=True) as d:
                d.run(1)
                bit_runs.append(d.raw())
        assert runs[0] == runs[1] == runs[2] and bit_runs[0] == bit_runs[1] == bit_runs[2]
        # the host form equals the device form (= the rule)
        r, off, chain, pts, poff = ctx.canny_curves(frames, 1.4, 50, 150, min_length=2)
        assert np.array_equal(off, want[1]) and np.array_equal(poff, want[4]), "canny_curves: the counts"
        assert np.array_equal(r, want[0]), "canny_curves: records"
        assert np.array_equal(chain, want[2]), "canny_curves: chain_offsets"
        assert pts.dtype == np.int32 and np.array_equal(pts, want[3]), "canny_curves: points"
        cut = P // 2
        r, off, chain, pts, poff = ctx.canny_curves(frames, 1.4, 50, 150, min_length=2, want_records=False, capacity=K - 1,
                                                    point_capacity=cut)
        assert r is None and np.array_equal(off, want[1]) and np.array_equal(poff, want[4])
        assert np.array_equal(chain, want[2][:K]) and np.array_equal(pts, want[3][:min(cut, int(want[2][K - 1]))])


def test_a_long_lived_context_with_dirty_workspaces(hip):
    """The row sums live in the workspaces of the contours' and the components' scans: a curves call after calls of
    another shape that left them dirty, and a components call after the curves call, each still exact."""
    import contours_rule
    big, small = _frames(2, 120, 1001, 40), _frames(3, 37, 53, 50)
    big_maps = _oracle_maps(big, 1.4, 50, 150, "dirty-big")
    small_maps = _oracle_maps(small, 1.4, 50, 150, "dirty-small")
    with hip.Context(0) as ctx:
        s, off, chain, pts, poff = ctx.canny_contours(big, 1.4, 50, 150, min_area=1)
        w = contours_rule.csr(big_maps, 1)
        assert np.array_equal(off, w[1]) and np.array_equal(pts, w[3]), "contours before"
        ctx.canny_components(big, 1.4, 50, 150, min_area=3)
        want = rule.csr(small_maps, 1)
        with _Dev(ctx, small, want[0].shape[0], want[3].size) as d:
            d.run(1, 1.4, 50, 150)
            d.check(want, "curves after contours / components of another shape")
        labels, kept, stats, offsets = ctx.canny_components(big, 1.4, 50, 150, min_area=2, want_kept=True)
        w_labels, w_stats, w_off = cr.csr(big_maps, 2)
        assert np.array_equal(offsets, w_off) and np.array_equal(stats, w_stats), "components after curves: records"
        assert np.array_equal(labels, w_labels), "components after curves: labels"
        s, off, chain, pts, poff = ctx.canny_contours(small, 1.4, 50, 150, min_area=1)
        w = contours_rule.csr(small_maps, 1)
        assert np.array_equal(off, w[1]) and np.array_equal(chain, w[2]) and np.array_equal(pts, w[3]), "contours after"
        want = rule.csr(big_maps, 3)
        with _Dev(ctx, big, want[0].shape[0], want[3].size) as d:
            d.run(3, 1.4, 50, 150)
            d.check(want, "curves of the larger shape afterwards")


def test_curves_call_after_an_unflushed_stream_call(hip):
    h, w = 96, 256
    streamed, mine = _frames(5, h, w, 1200), _frames(3, h, w, 1300)
    streamed_maps = _oracle_maps(streamed, 1.4, 50, 150, "streamed")
    maps = _oracle_maps(mine, 1.4, 50, 150, "mine")
    want = rule.csr(maps, 2)
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", 0)
        d_in, d_map = ctx.malloc(streamed.nbytes), ctx.malloc(streamed.nbytes * 2)
        try:
            ctx.h2d(d_in, streamed)
            got = np.empty(streamed.shape, np.int16)
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_bits_call(ctx, maps != 0, 2, "bits form after a streamed call", want=want)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map"
        finally:
            ctx.free(d_in)
            ctx.free(d_map)


# ---- past the cap of the row grid ------------------------------------------------------------------------------------------
def test_curves_past_the_row_cap(hip):
    """More than 65 536 x 4 image rows: the plan query says that a wave takes a second trip.  Narrow frames, five distinct
    maps in a cycle whose length does not divide a trip; once with room for everything, once with capacities that end
    inside the second trip."""
    n, h, w, cycle = 65003, 7, 8, 5
    p = hip.curves_plan(n, h, w)
    per_trip = p.grid * p.per_group
    assert p.trips >= 2 and p.units == n * h and p.units % per_trip != 0 and per_trip % (cycle * h) != 0, p
    rng = np.random.default_rng(7)
    distinct = np.stack([np.zeros((h, w), bool), np.ones((h, w), bool), rng.random((h, w)) < 0.25,
                         rng.random((h, w)) < 0.45, rule.embed(rule.designed_maps()["square_ring"], h, w)])
    idx = np.arange(n) % cycle
    per = [rule.curves(m, 1) for m in distinct]
    counts = np.array([r.shape[0] for r, _ in per])
    lens = [np.array([c.size for c in cs], np.int64) for _, cs in per]
    pts = [np.concatenate(cs) if cs else np.zeros(0, np.int32) for _, cs in per]
    w_off = np.concatenate([[0], np.cumsum(counts[idx])]).astype(np.uint64)
    w_rec = np.concatenate([per[k][0] for k in idx])
    w_chain = np.concatenate([[0], np.cumsum(np.concatenate([lens[k] for k in idx]))]).astype(np.uint64)
    w_points = np.concatenate([pts[k] for k in idx])
    w_poff = w_chain[w_off.astype(np.int64)]
    want = (w_rec, w_off, w_chain, w_points, w_poff)
    K, P = w_rec.shape[0], w_points.size
    r1 = int(w_off[per_trip // h + 1])     # the records of the frames that the first trip touches
    cap, pcap = (r1 + K) // 2, (int(w_chain[r1]) + P) // 2
    assert r1 < cap < K and int(w_chain[r1]) < pcap < P
    bits = np.packbits(distinct, axis=-1)[idx]
    with hip.Context(0) as ctx:
        for c, pc in ((K, P), (cap, pcap)):
            with _Dev(ctx, bits, c, pc, h=h, w=w, bits=True) as d:
                d.run(1)
                d.check(want, f"past the cap, capacities {c} of {K}, {pc} of {P}")


# ---- composition -----------------------------------------------------------------------------------------------------------
def test_the_curve_points_feed_the_edgels_at_call(hip):
    h, w, sigma = 120, 200, 1.4
    frames = _frames(3, h, w, 11)
    maps = _oracle_maps(frames, sigma, 50, 150, "edgels")
    want = rule.csr(maps, 3)
    K, P = want[0].shape[0], want[3].size
    assert P > 100
    planes = [oracle.gaussian(f, sigma) for f in frames]
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, K, P) as d:
            d.run(3, sigma, 50, 150)
            d.check(want, "curves before edgels_at")
            d_edgels = d._filled(np.full((P + N_GUARD) * 4, GUARD32, np.int32))
            ctx.dev_edgels_at(0, False, h, w, 3, d.d_points, d.d_poff, d_edgels, P)   # the context's smoothed plane
            got = d.get(d_edgels, (P + N_GUARD) * 4, np.int32)
            assert np.all(got[P * 4:] == GUARD32)
            poff = want[4].astype(np.int64)
            w_edgels = np.concatenate([er.edgels_at(planes[f], want[3][poff[f]:poff[f + 1]].astype(np.uint32))
                                       for f in range(3)])
            assert np.array_equal(got[:P * 4].reshape(P, 4).view(np.uint32), w_edgels.view(np.uint32)), \
                "edgels along the curves differ from the rule"


def test_parts_are_timed_and_the_stages_are_unaffected(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150, "timed")
    want = rule.csr(maps, 1)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)
        with _Dev(ctx, frames, want[0].shape[0], want[3].size) as d:
            d.run(1, 1.4, 50, 150)
            d.check(want, "profiled")
        for part in range(2):
            ms, launches = ctx.curves_profile_get(part)
            assert launches == 1 and ms > 0.0, hip.CURVE_PARTS[part]
        for stage in range(9):
            assert ctx.profile_get(stage)[1] == 0
        assert ctx.contours_profile_get(0)[1] == 0 and ctx.components_profile_get(0)[1] == 0
