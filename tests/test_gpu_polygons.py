"""Polygon approximation of the contour chains on the GPU (canny_hip_dev_canny_polygons / canny_hip_dev_polygons_bits /
canny_hip_dev_polygons_chains / canny_hip_canny_polygons): for every stored chain the vertices Douglas-Peucker keeps, with
the length, twice the area and the convexity of the polygon, CSR-shaped over the records.

Reference: oracle.canny per frame -> the contour rule of tests/contours_rule.py -> the plain-Python rule of
tests/polygons_rule.py.  Everything is integers, equality is exact.  vertex_offsets, vertices and measures are checked
separately so that a failure names which; so are the contours outputs the call passes through.  Every output buffer is
pre-filled with a pattern and followed by guard words."""
import os
import subprocess

import numpy as np
import pytest

import components_rule as cr
import contours_rule
import oracle
import polygons_rule as rule
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD32 = np.int32(0x5A5A5A5A)
GUARD64 = np.int64(0x5A5A5A5A5A5A5A5A)
OFF_FILL = np.uint64(0xEEEEEEEEEEEEEEEE)
N_GUARD = 64
SHAPES = [(37, 53), (9, 2), (2, 9), (120, 1001), (270, 480)]
MIN_AREAS = [1, 5]
TOLERANCES = [(0, 0), (256, 0), (0, 1311), (384, 655), (1 << 24, 0)]

_cache = {}


def _frames(n, h, w, seed0):
    return np.stack([synth_frame(h, w, seed0 + i) for i in range(n)])


def _oracle_maps(frames, sigma, lo, hi):
    k = ("maps", frames.shape, frames.tobytes()[:64], sigma, lo, hi)
    if k not in _cache:
        _cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _cache[k]


def _want_chains(maps, min_area, key):
    """contours_rule.csr of the maps, computed once per (key, min_area) and shared, never changed."""
    k = ("csr", key, maps.shape, min_area)
    if k not in _cache:
        _cache[k] = contours_rule.csr(maps, min_area)
    return _cache[k]


def _want_polygons(want_ct, capacity, point_capacity, width, tol, key=None):
    """polygons_rule.csr of the records that a call with these capacities stores."""
    fit = min(want_ct[0].shape[0], capacity)
    k = ("pg", key, fit, point_capacity, width, tol)
    if key is None or k not in _cache:
        res = rule.csr(want_ct[2][:fit + 1], want_ct[3], point_capacity, width, *tol)
        if key is None:
            return res
        _cache[k] = res
    return _cache[k]


class _Dev:
    """Device buffers of one polygons call.  source: frames uint8 [n, h, w] (the canny route) or, with bits=True, packed
    bit maps [n, h, ceil(w / 8)]."""

    def __init__(self, ctx, source, capacity, point_capacity, vertex_capacity, h=None, w=None, bits=False, measures=True,
                 vertices=True):
        self.ctx, self.bits = ctx, bits
        self.capacity, self.point_capacity, self.vertex_capacity = int(capacity), int(point_capacity), int(vertex_capacity)
        self.n = source.shape[0]
        self.h, self.w = (h, w) if bits else source.shape[1:]
        self.ptrs = []
        self.d_src = self._malloc(source.nbytes + 16)
        ctx.h2d(self.d_src, source)
        self.d_off = self._filled(np.full(self.n + 1, OFF_FILL, np.uint64))
        self.d_poff = self._filled(np.full(self.n + 1, OFF_FILL, np.uint64))
        self.d_chain = self._filled(np.full(self.capacity + 1 + N_GUARD, OFF_FILL, np.uint64))
        self.d_points = self._filled(np.full(self.point_capacity + N_GUARD, GUARD32, np.int32))
        self.d_voff = self._filled(np.full(self.capacity + 1 + N_GUARD, OFF_FILL, np.uint64))
        self.d_verts = self._filled(np.full(self.vertex_capacity + N_GUARD, GUARD32, np.int32)) if vertices else 0
        self.d_meas = self._filled(np.full((self.capacity + N_GUARD) * 4, GUARD64, np.int64)) if measures else 0

    def _malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def _filled(self, a):
        p = self._malloc(a.nbytes)
        self.ctx.h2d(p, a)
        return p

    def run(self, min_area, tol, sigma=None, lo=None, hi=None):
        vcap = self.vertex_capacity if self.d_verts else 0
        if self.bits:
            self.ctx.dev_polygons_bits(self.d_src, self.h, self.w, self.n, min_area, 0, self.capacity, self.d_off,
                                       self.d_chain, self.d_points, self.point_capacity, self.d_poff, tol[0], tol[1],
                                       self.d_voff, self.d_verts, vcap, self.d_meas)
        else:
            self.ctx.dev_canny_polygons(self.d_src, sigma, lo, hi, self.h, self.w, self.n, min_area, 0, self.capacity,
                                        self.d_off, self.d_chain, self.d_points, self.point_capacity, self.d_poff, tol[0],
                                        tol[1], self.d_voff, self.d_verts, vcap, self.d_meas)

    def get(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        self.ctx.d2h(out, ptr)
        return out

    def polygon_outputs(self):
        """(vertex_offsets, vertices or None, measures or None), guards included."""
        return (self.get(self.d_voff, self.capacity + 1 + N_GUARD, np.uint64),
                self.get(self.d_verts, self.vertex_capacity + N_GUARD, np.int32) if self.d_verts else None,
                self.get(self.d_meas, (self.capacity + N_GUARD) * 4, np.int64) if self.d_meas else None)

    def raw(self):
        out = [self.get(self.d_off, self.n + 1, np.uint64), self.get(self.d_poff, self.n + 1, np.uint64),
               self.get(self.d_chain, self.capacity + 1 + N_GUARD, np.uint64),
               self.get(self.d_points, self.point_capacity + N_GUARD, np.int32)]
        out += [a for a in self.polygon_outputs() if a is not None]
        return tuple(a.tobytes() for a in out)

    def check(self, want_ct, want_pg, what):
        """want_ct = contours_rule.csr(...), want_pg = polygons_rule.csr(...) of the stored records: every output named."""
        _, w_off, w_chain, w_points, w_poff = want_ct
        w_voff, w_verts, w_meas = want_pg
        fit = min(int(w_off[-1]), self.capacity)
        assert np.array_equal(self.get(self.d_off, self.n + 1, np.uint64), w_off), f"{what}: offsets"
        assert np.array_equal(self.get(self.d_poff, self.n + 1, np.uint64), w_poff), f"{what}: point_offsets"
        got = self.get(self.d_chain, self.capacity + 1 + N_GUARD, np.uint64)
        assert np.array_equal(got[:fit + 1], w_chain[:fit + 1]), f"{what}: chain_offsets"
        assert np.all(got[fit + 1:] == OFF_FILL), f"{what}: written past the chain offsets that exist"
        got = self.get(self.d_points, self.point_capacity + N_GUARD, np.int32)
        pfit = min(self.point_capacity, int(w_chain[fit]))
        assert np.array_equal(got[:pfit], w_points[:pfit]), f"{what}: points"
        assert np.all(got[pfit:] == GUARD32), f"{what}: written past the points that fit"
        check_polygon_outputs(self.polygon_outputs(), fit, self.vertex_capacity, want_pg, what)

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_polygon_outputs(outputs, fit, vertex_capacity, want_pg, what):
    voff, verts, meas = outputs
    w_voff, w_verts, w_meas = want_pg
    assert w_voff.size == fit + 1
    assert np.array_equal(voff[:fit + 1], w_voff), f"{what}: vertex_offsets differ"
    assert np.all(voff[fit + 1:] == OFF_FILL), f"{what}: written past the vertex offsets that exist"
    if verts is not None:
        vfit = min(vertex_capacity, w_verts.size)
        assert np.array_equal(verts[:vfit], w_verts[:vfit]), f"{what}: vertices differ"
        assert np.all(verts[vfit:] == GUARD32), f"{what}: written past the vertices that fit"
    if meas is not None:
        got = meas[:4 * fit].reshape(fit, 4)
        for col, name in enumerate(("vertices", "length_q8", "area2", "convex")):
            assert np.array_equal(got[:, col], w_meas[:, col]), f"{what}: measures[{name}] differ"
        assert np.all(meas[4 * fit:] == GUARD64), f"{what}: written past the measures that exist"


# ---- the canny route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", MIN_AREAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_polygons_match_the_rule_on_the_oracles_maps(hip, shape, min_area):
    h, w = shape
    frames = _frames(3, h, w, 300 + h + w)
    maps = _oracle_maps(frames, 1.4, 50, 150)
    want_ct = _want_chains(maps, min_area, "main")
    K, P = want_ct[0].shape[0], want_ct[3].size
    with hip.Context(0) as ctx:
        for tol in TOLERANCES:
            what = f"{shape} min_area={min_area} tol={tol}"
            want_pg = _want_polygons(want_ct, K, P, w, tol, key=("main", shape, min_area))
            with _Dev(ctx, frames, K, P, P) as d:
                d.run(min_area, tol, 1.4, 50, 150)
                d.check(want_ct, want_pg, what)
            if tol[0] >= 1 << 24 and K:
                assert int(want_pg[2][:, 0].max()) <= 2, "eps = 2^24 leaves the anchors"


# ---- designed maps on both sides of the 64-point boundary -----------------------------------------------------------------
def _designed():
    """name -> (mask, the chain length it is there for).  Every mask is 70 wide."""
    out = {}
    for n_px, n_chain in ((2, 2), (32, 62), (33, 64), (34, 66)):
        m = np.zeros((5, 70), bool)
        m[2, 3:3 + n_px] = True
        out[f"line{n_px}"] = (m, n_chain)
    m = np.zeros((5, 70), bool)
    m[1, 7] = True
    out["dot"] = (m, 1)
    m = np.zeros((12, 70), bool)
    m[1:10, 2:5] = True
    m[7:10, 2:11] = True
    out["l_block"] = (m, None)
    s = np.zeros((66, 70), bool)
    s[1:65, 3:67] = cr.serpentine(64, 64)
    out["serpentine"] = (s, None)
    return out


def test_designed_chains_around_the_64_point_boundary(hip):
    named = _designed()
    for name, (m, n_chain) in named.items():
        _, chains = contours_rule.contours(m)
        assert len(chains) == 1, name
        if n_chain is not None:
            assert chains[0].size == n_chain, name
    assert named["l_block"][0].any() and contours_rule.contours(named["l_block"][0])[1][0].size % 2 == 1, "an odd length"
    assert contours_rule.contours(named["serpentine"][0])[1][0].size > 4000
    # all in one frame, stacked with a blank row between them: short and long records alternate within one launch
    order = ["line2", "serpentine", "line32", "dot", "line33", "l_block", "line34"]
    one = np.concatenate([np.pad(named[k][0], ((0, 1), (0, 0))) for k in order])
    h = max(named[k][0].shape[0] for k in order)
    separate = np.stack([np.pad(named[k][0], ((0, h - named[k][0].shape[0]), (0, 0))) for k in order])
    with hip.Context(0) as ctx:
        for masks, label in ((one[None], "one frame"), (separate, "separate frames")):
            want_ct = contours_rule.csr(masks, 1)
            K, P = want_ct[0].shape[0], want_ct[3].size
            assert K == len(order)
            lengths = np.diff(want_ct[2]).astype(int)
            assert {1, 2, 62, 64, 66} <= set(lengths.tolist())
            bits = np.packbits(masks, axis=-1)
            for tol in TOLERANCES + [(181, 0), (512, 0)]:
                want_pg = rule.csr(want_ct[2], want_ct[3], P, masks.shape[2], *tol)
                with _Dev(ctx, bits, K, P, P, h=masks.shape[1], w=masks.shape[2], bits=True) as d:
                    d.run(1, tol)
                    d.check(want_ct, want_pg, f"designed, {label}, tol={tol}")
                if tol == (0, 0):
                    by_len = dict(zip(lengths.tolist(), want_pg[2].tolist()))
                    assert by_len[1][0] == 1 and by_len[2][0] == 2 and by_len[64][0] == 2 and by_len[66][0] == 2
                    assert int(want_pg[2][:, 0].max()) > 100, "the serpentine keeps its turning points"


# ---- hand-made chains, uploaded directly ----------------------------------------------------------------------------------
def _zigzag(n, width, growing):
    """n points (i, 200 +- amplitude): the amplitude grows (or, mirrored, shrinks) along the chain, so the farthest point of
    a run lies next to the run's end (or its start) and the descent is as deep as the chain is long."""
    i = np.arange(n)
    amp = i if growing else n - 1 - i
    return ((200 + np.where(i % 2 == 1, amp, -amp)) * width + i).astype(np.int32)


def _run_chains(ctx, chains, width, height, tol, capacity=None, point_capacity=None, vertex_capacity=None, measures=True,
                vertices=True, n_frames=1):
    """dev_polygons_chains on chains uploaded as a contours call would have left them -> the outputs with their guards."""
    K = len(chains)
    co = np.zeros(K + 1, np.uint64)
    co[1:] = np.cumsum([len(c) for c in chains], dtype=np.uint64)
    pts = np.concatenate(chains).astype(np.int32)
    cap = K if capacity is None else capacity
    pcap = pts.size if point_capacity is None else point_capacity
    vcap = pts.size if vertex_capacity is None else vertex_capacity
    offsets = np.zeros(n_frames + 1, np.uint64)
    offsets[1:] = K
    bufs = [offsets, np.concatenate([co[:min(K, cap) + 1], np.full(max(0, cap - K) + N_GUARD, OFF_FILL, np.uint64)]),
            np.concatenate([pts[:pcap], np.full(N_GUARD, GUARD32, np.int32)]),
            np.full(cap + 1 + N_GUARD, OFF_FILL, np.uint64), np.full(vcap + N_GUARD, GUARD32, np.int32),
            np.full((cap + N_GUARD) * 4, GUARD64, np.int64)]
    ptrs = []
    try:
        for b in bufs:
            ptrs.append(ctx.malloc(max(b.nbytes, 16)))
            ctx.h2d(ptrs[-1], b)
        ctx.dev_polygons_chains(ptrs[0], n_frames, cap, ptrs[1], ptrs[2], pcap, width, height, tol[0], tol[1], ptrs[3],
                                ptrs[4] if vertices else 0, vcap if vertices else 0, ptrs[5] if measures else 0)
        for b, p in zip(bufs[3:], ptrs[3:]):
            ctx.d2h(b, p)
        for b, p in zip([a.copy() for a in bufs[:3]], ptrs[:3]):   # the inputs are read-only
            got = np.empty_like(b)
            ctx.d2h(got, p)
            assert np.array_equal(got, b), "dev_polygons_chains changed its input"
    finally:
        for p in ptrs:
            ctx.free(p)
    fit = min(K, cap)
    want = rule.csr(co[:fit + 1], pts, pcap, width, *tol)
    return (bufs[3], bufs[4] if vertices else None, bufs[5] if measures else None), fit, vcap, want


@pytest.mark.parametrize("growing", [True, False], ids=["farthest_at_the_end", "farthest_at_the_start"])
@pytest.mark.parametrize("tol", [(0, 0), (256, 0), (2560, 0), (0, 1311), (25600, 0)], ids=lambda t: f"eps{t[0]}_ratio{t[1]}")
def test_hand_made_zigzags_reach_the_strided_paths_bookkeeping(hip, growing, tol):
    width, height = 512, 512
    square = np.array([10 * width + 10, 10 * width + 30, 30 * width + 30, 30 * width + 10], np.int32)
    chains = [_zigzag(200, width, growing), square, _zigzag(65, width, not growing), _zigzag(64, width, growing),
              np.array([7], np.int32), _zigzag(129, width, growing)]
    with hip.Context(0) as ctx:
        outputs, fit, vcap, want = _run_chains(ctx, chains, width, height, tol)
        check_polygon_outputs(outputs, fit, vcap, want, f"zig-zags growing={growing} tol={tol}")
        if tol == (0, 0):
            assert want[2][0, 0] == 200 and want[2][1].tolist() == [4, 256 * 4, 2 * 400, 1], "nothing is collinear; the square: 4 axis steps"


# ---- capacities, absent outputs, determinism ------------------------------------------------------------------------------
def test_capacities_bound_the_writes_never_the_counts(hip):
    frames = _frames(3, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150)
    want_ct = _want_chains(maps, 1, "capacity")
    w_chain = want_ct[2]
    K, P = want_ct[0].shape[0], want_ct[3].size
    w = frames.shape[2]
    tol = (256, 655)
    full = _want_polygons(want_ct, K, P, w, tol)
    V = int(full[0][-1])
    assert K > 8 and V > K
    first1 = int(want_ct[1][1])                      # the first record of frame 1
    j = first1 + int(np.argmax(np.diff(w_chain[first1:int(want_ct[1][2]) + 1])))
    mid = int(w_chain[j]) + int(w_chain[j + 1] - w_chain[j]) // 2
    assert w_chain[j] < mid < w_chain[j + 1] and want_ct[1][1] <= j < want_ct[1][2], "cuts a chain in the middle of frame 1"
    jv = int(np.argmax(np.diff(full[0])))
    vmid = int(full[0][jv]) + 1
    assert full[0][jv] < vmid < full[0][jv + 1], "cuts a polygon"
    with hip.Context(0) as ctx:
        for cap, pcap, vcap in ((K, P, V), (K - 1, P, V), (1, P, V), (0, P, V), (K, mid, V), (K, 0, V), (K, P, 0),
                                (K, P, vmid), (K - 1, mid, vmid), (K + 9, P + 9, V + 9)):
            want_pg = _want_polygons(want_ct, cap, pcap, w, tol)
            what = f"capacity={cap} point_capacity={pcap} vertex_capacity={vcap}"
            if pcap == mid:
                assert want_pg[2][min(j, len(want_pg[2]) - 1)].tolist() == [-1, 0, 0, 0] or cap <= j
            seen = []
            for outs in (dict(), dict(measures=False), dict(vertices=False), dict(measures=False, vertices=False)):
                with _Dev(ctx, frames, cap, pcap, vcap, **outs) as d:
                    d.run(1, tol, 1.4, 50, 150)
                    d.check(want_ct, want_pg, f"{what} {outs}")
                    voff, verts, meas = d.polygon_outputs()
                    seen.append((voff.tobytes(), None if verts is None else verts.tobytes(),
                                 None if meas is None else meas.tobytes()))
            assert len({s[0] for s in seen}) == 1, f"{what}: vertex_offsets depend on which outputs are absent"
            assert seen[0][1] == seen[1][1] and seen[0][2] == seen[2][2], f"{what}: an output depends on the others"


def test_same_bytes_on_every_run_and_the_other_calls_still_equal_their_rules(hip):
    frames = _frames(4, 270, 480, 77)
    maps = _oracle_maps(frames, 1.4, 50, 150)
    want_ct = _want_chains(maps, 2, "determinism")
    K, P = want_ct[0].shape[0], want_ct[3].size
    tol = (128, 1311)
    want_pg = _want_polygons(want_ct, K, P, 480, tol)
    with hip.Context(0) as ctx:
        runs = []
        for k in range(3):
            with _Dev(ctx, frames, K, P, P) as d:
                d.run(2, tol, 1.4, 50, 150)
                if k == 0:
                    d.check(want_ct, want_pg, "first run")
                runs.append(d.raw())
        assert runs[0] == runs[1] == runs[2]
        # the host form: the chains stay on the device unless asked for
        polygons, measures, offsets, extra = ctx.canny_polygons(frames, 1.4, 50, 150, min_area=2, epsilon=0.5, ratio=0.02)
        assert np.array_equal(offsets, want_ct[1]) and np.array_equal(extra["point_offsets"], want_ct[4])
        assert np.array_equal(extra["vertex_offsets"], want_pg[0]), "canny_polygons: vertex_offsets"
        assert np.array_equal(extra["vertices"], want_pg[1]), "canny_polygons: vertices"
        assert np.array_equal(measures, want_pg[2]), "canny_polygons: measures"
        assert np.array_equal(extra["chain_offsets"], want_ct[2]) and "points" not in extra
        assert len(polygons) == K and all(p.size == m[0] for p, m in zip(polygons, measures))
        _, _, _, extra = ctx.canny_polygons(frames, 1.4, 50, 150, min_area=2, epsilon=0.5, ratio=0.02, want_stats=True,
                                            want_points=True)
        assert np.array_equal(extra["points"], want_ct[3]) and np.array_equal(extra["stats"], want_ct[0])
        assert np.array_equal(extra["vertices"], want_pg[1])
        # the workspaces are shared: a contours and a components call on the same context afterwards equal their rules
        s, off, chain, pts, poff = ctx.canny_contours(frames, 1.4, 50, 150, min_area=2)
        assert np.array_equal(off, want_ct[1]) and np.array_equal(poff, want_ct[4]) and np.array_equal(s, want_ct[0])
        assert np.array_equal(chain, want_ct[2]) and np.array_equal(pts, want_ct[3]), "contours after polygons"
        labels, kept, stats, offsets = ctx.canny_components(frames, 1.4, 50, 150, min_area=2, want_kept=True)
        w_labels, w_stats, w_off = cr.csr(maps, 2)
        assert np.array_equal(offsets, w_off) and np.array_equal(stats, w_stats), "components after polygons: records"
        assert np.array_equal(labels, w_labels), "components after polygons: labels"


def test_max_val_above_255_gives_all_zeros(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300)
    assert not maps.any()
    want_ct = contours_rule.csr(maps, 1)
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 64, 64, 64) as d:
            d.run(1, (256, 0), 1.0, 50, 300)
            d.check(want_ct, rule.csr(want_ct[2], want_ct[3], 64, 256, 256, 0), "max_val=300")
        polygons, measures, offsets, extra = ctx.canny_polygons(frames, 1.0, 50, 300, epsilon=1.0)
        assert polygons == [] and measures.shape == (0, 4) and not offsets.any() and extra["vertex_offsets"].tolist() == [0]


def test_argument_errors_return_their_statuses_and_write_nothing(hip):
    frames = _frames(2, 64, 64, 9)
    tall = np.zeros((1, 32769, 1), np.uint8)           # packed bits of a 32769 x 2 map: a height above 32768
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 256, 4096, 4096) as d:
            before = d.raw()
            base = dict(d_img=d.d_src, sigma=1.4, min_val=50, max_val=150, h=64, w=64, n=2, min_area=1, d_stats=0,
                        capacity=256, d_offsets=d.d_off, d_chain_offsets=d.d_chain, d_points=d.d_points,
                        point_capacity=4096, d_point_offsets=d.d_poff, epsilon_q8=256, ratio_q16=0,
                        d_vertex_offsets=d.d_voff, d_vertices=d.d_verts, vertex_capacity=4096, d_measures=d.d_meas)
            for change, status in ((dict(ratio_q16=65536), 1), (dict(d_vertex_offsets=0), 1), (dict(d_vertices=0), 1),
                                   (dict(d_chain_offsets=0), 1), (dict(d_points=0), 1), (dict(d_offsets=0), 1),
                                   (dict(d_point_offsets=0), 1), (dict(d_img=0), 1), (dict(min_val=300, max_val=100), 5)):
                with pytest.raises(hip.CannyHipError) as ei:
                    ctx.dev_canny_polygons(**{**base, **change})
                assert ei.value.status == status, change
                ctx.synchronize()
                assert d.raw() == before, f"{change}: a rejected call wrote something"
            for change, status in ((dict(ratio_q16=65536), 1), (dict(d_vertex_offsets=0), 1), (dict(d_offsets=0), 1),
                                   (dict(d_chain_offsets=0), 1), (dict(n=0), 1), (dict(w=32769), 2), (dict(h=32769), 2)):
                args = dict(d_offsets=d.d_off, n=2, capacity=256, d_chain_offsets=d.d_chain, d_points=d.d_points,
                            point_capacity=4096, w=64, h=64, epsilon_q8=0, ratio_q16=0, d_vertex_offsets=d.d_voff,
                            d_vertices=d.d_verts, vertex_capacity=4096, d_measures=d.d_meas)
                with pytest.raises(hip.CannyHipError) as ei:
                    ctx.dev_polygons_chains(**{**args, **change})
                assert ei.value.status == status, change
                ctx.synchronize()
                assert d.raw() == before, f"{change}: a rejected call wrote something"
        with _Dev(ctx, tall, 8, 64, 64, h=32769, w=2, bits=True) as d:
            before = d.raw()
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1, (0, 0))
            assert ei.value.status == 2
            ctx.synchronize()
            assert d.raw() == before


def test_parts_are_timed_and_the_contours_parts_are_unaffected(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150)
    want_ct = contours_rule.csr(maps, 1)
    K, P = want_ct[0].shape[0], want_ct[3].size
    want_pg = rule.csr(want_ct[2], want_ct[3], P, 256, 256, 0)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        for mask, counted in ((1 << 30, (1, 1, 1)), (0b1111 << 22, (0, 0, 0))):
            ctx.profile_reset()
            ctx.set_option("profile_stage_mask", mask)
            with _Dev(ctx, frames, K, P, P) as d:
                d.run(1, (256, 0), 1.4, 50, 150)
                d.check(want_ct, want_pg, "profiled")
            for part in range(3):
                ms, launches = ctx.polygons_profile_get(part)
                assert launches == counted[part] and (ms > 0.0) == bool(counted[part]), hip.POLYGON_PARTS[part]
            for stage in range(9):
                assert ctx.profile_get(stage)[1] == 0
            assert ctx.contours_profile_get(0)[1] == (0 if counted[0] else 1) and ctx.hough_circles_profile_get(3)[1] == 0


def test_cli_writes_the_polygons(hip, tmp_path):
    h, w = 64, 72
    frame = synth_frame(h, w, 4)
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + frame.tobytes())
    edges = oracle.canny(frame, 1.4, 50, 150)
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    for value, tol, extra, min_area in (("1.5,0.02", (384, 1311), [], 1), ("0", (0, 0), ["-m", "4"], 4)):
        out = tmp_path / f"out{min_area}"
        out.mkdir()
        r = subprocess.run([exe, "1.4", "50", "150", "-i", str(src), "-o", str(out), "-t", "-y", value] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        _, chains = contours_rule.contours(edges, min_area)
        assert len(chains) > 0
        assert len((out / "canny_contours.txt").read_text().splitlines()) == len(chains), "-t still writes its file"
        lines = (out / "canny_polygons.txt").read_text().splitlines()
        assert len(lines) == len(chains)
        for k, (ln, ch) in enumerate(zip(lines, chains), 1):
            pos, measures = rule.polygon(ch, w, *tol)
            t = [int(v) for v in ln.split()]
            assert t[:2] == [0, k] and t[2:6] == [int(v) for v in measures], f"polygon {k}: frame record and measures"
            assert t[6::2] == [int(ch[i]) % w for i in pos] and t[7::2] == [int(ch[i]) // w for i in pos], f"polygon {k}"
