"""Outer contour chains on the GPU (canny_hip_dev_canny_contours / canny_hip_dev_contours_bits /
canny_hip_canny_contours): for every kept component of the finished edge map the ordered list of its outer border pixels,
CSR-shaped on two levels over the batch.

Reference: oracle.canny per frame -> the plain-Python rule of tests/contours_rule.py.  Everything is integers, equality is
exact.  offsets, point_offsets, chain_offsets, points and stats are checked separately so that a failure names which.
Every output buffer is pre-filled with a pattern and followed by guard words."""
import os
import subprocess

import numpy as np
import pytest

import components_rule as cr
import contours_rule as rule
import oracle
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = np.int32(0x5A5A5A5A)
N_GUARD = 64
OFF_FILL = np.uint64(0xEEEEEEEEEEEEEEEE)
SHAPES = [(270, 480), (37, 53), (9, 2), (2, 9), (64, 8), (120, 1001), (130, 4096)]
MIN_AREAS = [1, 5, 20]

_cache = {}


def _frames(n, h, w, seed0):
    return np.stack([synth_frame(h, w, seed0 + i) for i in range(n)])


def _oracle_maps(frames, sigma, lo, hi, key):
    k = ("maps", key, frames.shape, sigma, lo, hi)
    if k not in _cache:
        _cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _cache[k]


def _want(maps, min_area, key):
    """rule.csr of the maps, computed once per (key, min_area) and shared."""
    k = ("csr", key, maps.shape, min_area)
    if k not in _cache:
        _cache[k] = rule.csr(maps, min_area)
    return _cache[k]


class _Dev:
    """Device buffers of one contours call.  source: frames uint8 [n, h, w] (the canny route) or, with bits=True, packed
    bit maps [n, h, ceil(w / 8)] placed `shift` bytes into their allocation."""

    def __init__(self, ctx, source, capacity, point_capacity, h=None, w=None, bits=False, shift=0, stats=True, chain=True,
                 points=True, edges=False):
        self.ctx, self.capacity, self.point_capacity, self.bits = ctx, int(capacity), int(point_capacity), bits
        self.n = source.shape[0]
        self.h, self.w = (h, w) if bits else source.shape[1:]
        self.npx = self.n * self.h * self.w
        self.ptrs = []
        self.d_src = self._malloc(source.nbytes + shift + 16) + shift
        ctx.h2d(self.d_src, source)
        self.d_stats = self._filled(np.full((self.capacity + N_GUARD) * 6, GUARD32, np.int32)) if stats else 0
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

    def run(self, min_area, sigma=None, lo=None, hi=None):
        cap = self.capacity if self.d_chain else 0
        pcap = self.point_capacity if self.d_points else 0
        if self.bits:
            self.ctx.dev_contours_bits(self.d_src, self.h, self.w, self.n, min_area, self.d_stats, cap, self.d_off,
                                       self.d_chain, self.d_points, pcap, self.d_poff)
        else:
            self.ctx.dev_canny_contours(self.d_src, sigma, lo, hi, self.h, self.w, self.n, min_area, self.d_stats, cap,
                                        self.d_off, self.d_chain, self.d_points, pcap, self.d_poff, self.d_edges)

    def get(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        self.ctx.d2h(out, ptr)
        return out

    def raw(self):
        """Every output buffer, guards included, as bytes (for the run-to-run comparison)."""
        out = [self.get(self.d_off, self.n + 1, np.uint64), self.get(self.d_poff, self.n + 1, np.uint64)]
        if self.d_stats:
            out.append(self.get(self.d_stats, (self.capacity + N_GUARD) * 6, np.int32))
        if self.d_chain:
            out.append(self.get(self.d_chain, self.capacity + 1 + N_GUARD, np.uint64))
        if self.d_points:
            out.append(self.get(self.d_points, self.point_capacity + N_GUARD, np.int32))
        return tuple(a.tobytes() for a in out)

    def edges(self):
        return self.get(self.d_edges, self.npx, np.int16).reshape(self.n, self.h, self.w)

    def check(self, want, what):
        """want = rule.csr(...): every output that exists against it, each named."""
        w_stats, w_off, w_chain, w_points, w_poff = want
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
        if self.d_stats:
            got = self.get(self.d_stats, (self.capacity + N_GUARD) * 6, np.int32)
            assert np.array_equal(got[:fit * 6].reshape(fit, 6), w_stats[:fit]), f"{what}: stats differ"
            assert np.all(got[fit * 6:] == GUARD32), f"{what}: written past the records that fit"

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_bits_call(ctx, masks, min_area, what, want=None, shift=0, pad_ones=False, capacity=None, point_capacity=None,
                     **outs):
    n, h, w = masks.shape
    bits = np.packbits(masks, axis=-1)
    if pad_ones and w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want = rule.csr(masks, min_area) if want is None else want
    cap = want[0].shape[0] if capacity is None else capacity
    pcap = want[3].size if point_capacity is None else point_capacity
    with _Dev(ctx, bits, cap, pcap, h=h, w=w, bits=True, shift=shift, **outs) as d:
        d.run(min_area)
        d.check(want, what)
    return want


@pytest.mark.parametrize("min_area", MIN_AREAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_contours_match_the_rule_on_the_oracles_maps(hip, shape, min_area):
    h, w = shape
    frames = _frames(3, h, w, 300 + h + w)
    maps = _oracle_maps(frames, 1.4, 50, 150, "main")
    want = _want(maps, min_area, "main")
    what = f"{shape} min_area={min_area}"
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, want[0].shape[0], want[3].size, edges=True) as d:
            d.run(min_area, 1.4, 50, 150)
            d.check(want, what)
            assert np.array_equal(d.edges(), maps), f"{what}: the s16 map differs from the oracle"
            # the record CSR is the components calls' own
            d_off = d._filled(np.full(d.n + 1, OFF_FILL, np.uint64))
            ctx.dev_canny_components(d.d_src, 1.4, 50, 150, h, w, d.n, min_area, 0, 0, 0, 0, d_off, 0)
            assert np.array_equal(d.get(d_off, d.n + 1, np.uint64), want[1]), f"{what}: offsets of dev_canny_components"


def test_directed_masks_through_the_bits_route(hip):
    h, w = 130, 200   # the staircase and the diagonal pair cross the four-tile corner at 64
    named = cr.directed_masks(h, w)
    masks = np.stack(list(named.values()))
    with hip.Context(0) as ctx:
        for min_area in (1, 2):
            want = _check_bits_call(ctx, masks, min_area, f"directed min_area={min_area}: {list(named)}", pad_ones=True)
            if min_area == 1:
                counts = dict(zip(named, np.diff(want[1]).astype(int)))
                lengths = dict(zip(named, np.diff(want[4]).astype(int)))
                assert counts["all_set"] == 1 and lengths["all_set"] == 2 * (h + w) - 4
                assert counts["checkerboard"] == lengths["checkerboard"] == ((h + 1) // 2) * ((w + 1) // 2)
                assert counts["staircase"] == counts["diagonal_pair"] == counts["serpentine"] == counts["spiral"] == 1
                assert lengths["diagonal_pair"] == 2 and lengths["all_clear"] == 0


def test_the_long_single_trace(hip):
    m = cr.serpentine(256, 256)[None]
    with hip.Context(0) as ctx:
        want = _check_bits_call(ctx, m, 1, "serpentine(256, 256)")
        assert want[0].shape[0] == 1 and want[3].size == 65535


@pytest.mark.parametrize("density", [0.05, 0.4, 0.9])
def test_random_masks_through_the_bits_route(hip, density):
    with hip.Context(0) as ctx:
        for h, w in ((37, 63), (66, 129), (50, 77)):
            masks = np.random.default_rng(17 * h + w).random((3, h, w)) < density
            for min_area in (1, 5):
                want = rule.csr(masks, min_area)
                for shift in (1, 3):   # an odd byte address, padding bits set
                    _check_bits_call(ctx, masks, min_area, f"({h},{w}) density={density} min_area={min_area} shift={shift}",
                                     want=want, shift=shift, pad_ones=True)


@pytest.mark.parametrize("min_area", [1, 4])
def test_capacities_bound_the_writes_never_the_counts(hip, min_area):
    frames = _frames(3, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150, "capacity")
    want = _want(maps, min_area, "capacity")
    w_chain = want[2]
    K, P = want[0].shape[0], want[3].size
    assert K > 8 and P > K
    j = int(np.argmax(np.diff(w_chain)))
    mid = int(w_chain[j]) + int(w_chain[j + 1] - w_chain[j]) // 2
    assert w_chain[j] < mid < w_chain[j + 1], "lands inside a chain"
    with hip.Context(0) as ctx:
        for cap, pcap in ((K - 1, P), (1, P), (0, P), (K, mid), (K, 1), (K, 0), (K - 1, mid), (K + 9, P + 9)):
            with _Dev(ctx, frames, cap, pcap) as d:   # capacity 0 WITH real buffers: nothing may be written to them
                d.run(min_area, 1.4, 50, 150)
                d.check(want, f"capacity={cap} point_capacity={pcap}")
        with _Dev(ctx, frames, K, P, stats=False) as d:
            d.run(min_area, 1.4, 50, 150)
            d.check(want, "stats NULL")
        with _Dev(ctx, frames, 0, 0, stats=False, chain=False, points=False) as d:
            d.run(min_area, 1.4, 50, 150)
            d.check(want, "counts only")
        _check_bits_call(ctx, maps != 0, min_area, "bits, mid-chain", want=want, capacity=K - 1, point_capacity=mid)
        _check_bits_call(ctx, maps != 0, min_area, "bits, counts only", want=want, capacity=0, point_capacity=0,
                         stats=False, chain=False, points=False)
        # a capacity without its buffer is an argument error, and nothing is written
        for kw in (dict(chain=False), dict(points=False)):
            with _Dev(ctx, frames, K, P, **kw) as d:
                with pytest.raises(hip.CannyHipError) as ei:
                    ctx.dev_canny_contours(d.d_src, 1.4, 50, 150, d.h, d.w, d.n, min_area, d.d_stats, K, d.d_off, d.d_chain,
                                           d.d_points, P, d.d_poff, 0)
                assert ei.value.status == 1
                ctx.synchronize()
                assert np.all(d.get(d.d_off, d.n + 1, np.uint64) == OFF_FILL)
                assert np.all(d.get(d.d_poff, d.n + 1, np.uint64) == OFF_FILL)
                assert np.all(d.get(d.d_stats, (K + N_GUARD) * 6, np.int32) == GUARD32)


def test_max_val_above_255_follows_the_map(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300, "hi300")
    assert not maps.any(), "the oracle's map is all zero for max_val = 300"
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 64, 64, edges=True) as d:
            d.run(1, 1.0, 50, 300)
            d.check(rule.csr(maps, 1), "max_val=300")
            assert np.array_equal(d.edges(), maps)
        s, off, chain, pts, poff = ctx.canny_contours(frames, 1.0, 50, 300)
        assert s.shape == (0, 6) and not off.any() and not poff.any() and pts.size == 0 and chain.tolist() == [0]


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


def test_same_bytes_on_every_run_and_the_host_form(hip):
    frames = _frames(4, 270, 480, 77)
    maps = _oracle_maps(frames, 1.4, 50, 150, "determinism")
    want = _want(maps, 2, "determinism")
    K, P = want[0].shape[0], want[3].size
    with hip.Context(0) as ctx:
        runs = []
        for k in range(3):
            if k == 2:   # an unrelated call on the context in between
                ctx.canny_points(_frames(2, 96, 256, 1), 1.4, 50, 150)
            with _Dev(ctx, frames, K, P) as d:
                d.run(2, 1.4, 50, 150)
                if k == 0:
                    d.check(want, "first run")
                runs.append(d.raw())
        assert runs[0] == runs[1] == runs[2]
        # the host form equals the device form (= the rule)
        s, off, chain, pts, poff = ctx.canny_contours(frames, 1.4, 50, 150, min_area=2)
        assert np.array_equal(off, want[1]) and np.array_equal(poff, want[4]), "canny_contours: the counts"
        assert np.array_equal(s, want[0]), "canny_contours: stats"
        assert np.array_equal(chain, want[2]), "canny_contours: chain_offsets"
        assert pts.dtype == np.int32 and np.array_equal(pts, want[3]), "canny_contours: points"
        cut = P // 2
        s, off, chain, pts, poff = ctx.canny_contours(frames, 1.4, 50, 150, min_area=2, want_stats=False, capacity=K - 1,
                                                      point_capacity=cut)
        assert s is None and np.array_equal(off, want[1]) and np.array_equal(poff, want[4])
        assert np.array_equal(chain, want[2][:K]) and np.array_equal(pts, want[3][:min(cut, int(want[2][K - 1]))])
        # the workspaces are shared: a components call on the same context afterwards still equals its rule
        labels, kept, stats, offsets = ctx.canny_components(frames, 1.4, 50, 150, min_area=2, want_kept=True)
        w_labels, w_stats, w_off = cr.csr(maps, 2)
        assert np.array_equal(offsets, w_off) and np.array_equal(stats, w_stats), "components after contours: records"
        assert np.array_equal(labels, w_labels) and np.array_equal(kept, np.where(w_labels != 0, 255, 0)), "... planes"


def test_contours_call_after_an_unflushed_stream_call(hip):
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
            with _Dev(ctx, mine, want[0].shape[0], want[3].size) as d:
                d.run(2, 1.4, 50, 150)
                d.check(want, "after a streamed call")
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map"
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_bits_call(ctx, maps != 0, 2, "bits form after a streamed call", want=want)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map (2)"
        finally:
            ctx.free(d_in)
            ctx.free(d_map)


def test_cli_writes_the_contours(hip, tmp_path):
    h, w = 64, 72
    frame = synth_frame(h, w, 4)
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + frame.tobytes())
    edges = oracle.canny(frame, 1.4, 50, 150)
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    for extra, min_area in (([], 1), (["-m", "4"], 4)):
        out = tmp_path / f"out{min_area}"
        out.mkdir()
        r = subprocess.run([exe, "1.4", "50", "150", "-i", str(src), "-o", str(out), "-t"] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        stats, chains = rule.contours(edges, min_area)
        assert len(chains) > 0
        lines = (out / "canny_contours.txt").read_text().splitlines()
        assert len(lines) == len(chains)
        for k, (ln, ch) in enumerate(zip(lines, chains), 1):
            t = [int(v) for v in ln.split()]
            assert t[0] == k and t[1] == ch.size and len(t) == 2 + 2 * ch.size, f"contour {k}"
            assert t[2::2] == (ch % w).tolist() and t[3::2] == (ch // w).tolist(), f"contour {k}: x y pairs"


def test_parts_are_timed_and_the_stages_are_unaffected(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150, "timed")
    want = rule.csr(maps, 1)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 0b1111 << 22)
        with _Dev(ctx, frames, want[0].shape[0], want[3].size) as d:
            d.run(1, 1.4, 50, 150)
            d.check(want, "profiled")
        for part in range(4):
            ms, launches = ctx.contours_profile_get(part)
            assert launches == 1 and ms > 0.0, hip.CONTOUR_PARTS[part]
        for stage in range(9):
            assert ctx.profile_get(stage)[1] == 0
        assert ctx.components_profile_get(0)[1] == 0 and ctx.hough_profile_get(0)[1] == 0
