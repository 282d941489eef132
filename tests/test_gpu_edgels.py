"""Sub-pixel edgels on the GPU (canny_hip_dev_canny_edgels, canny_hip_dev_edgels_at, canny_hip_canny_edgels,
canny_hip_dev_edgels_arith) against tests/edgels_rule.py applied to the oracle's smoothed plane and
the oracle's map.  Every comparison is exact equality on whole arrays; every output buffer is sentinel-filled with guard
words behind it."""
import math
import os
import subprocess

import numpy as np
import pytest

import edgels_rule as er
import oracle
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
SIGMA, LO, HI = 1.4, 50, 150


class _Bufs:
    """Sentinel-filled device arrays of uint32 words with guard words behind them."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.words = ctx, [], {}

    def filled(self, words):
        p = self.ctx.malloc(4 * (words + N_GUARD))
        self.ptrs.append(p)
        self.words[p] = words
        self.refill(p)
        return p

    def refill(self, p):
        self.ctx.h2d(p, np.full(self.words[p] + N_GUARD, SENT, np.uint32))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def get(self, p, what=""):
        out = np.empty(self.words[p] + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[self.words[p]:] == SENT).all(), f"guard words overwritten {what}"
        return out[:self.words[p]]

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


_REF = {}


def reference(h, w):
    """(frames, maps, smoothed planes, records per frame, indices per frame) of the three synth frames of a shape; computed
    once, never modified."""
    if (h, w) not in _REF:
        frames = np.stack([synth_frame(h, w, s) for s in (1, 2, 3)])
        maps = np.stack([oracle.canny(f, SIGMA, LO, HI) for f in frames])
        planes = [oracle.gaussian(f, SIGMA) for f in frames]
        idx = [np.flatnonzero(m.reshape(-1)).astype(np.uint32) for m in maps]
        rec = [er.edgels_at(p, i) for p, i in zip(planes, idx)]
        for a in (frames, maps, *planes, *idx, *rec):
            a.setflags(write=False)
        _REF[(h, w)] = (frames, maps, planes, rec, idx)
    return _REF[(h, w)]


def csr(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)


def run_edgels(ctx, b, d_img, n, h, w, capacity, with_points=True, with_edges=True, lo=LO, hi=HI):
    """One guarded dev_canny_edgels call -> (records uint32 [capacity, 4], offsets, points or None, edges or None)."""
    d_rec, d_off = b.filled(4 * capacity), b.filled(2 * (n + 1))
    d_pts = b.filled(capacity) if with_points else 0
    d_edges = b.filled(n * h * w // 2 + 1) if with_edges else 0
    ctx.dev_canny_edgels(d_img, SIGMA, lo, hi, h, w, n, d_rec if capacity else 0, capacity, d_off, d_edges=d_edges,
                         d_points=d_pts if capacity else 0)
    rec = b.get(d_rec, "behind the records").reshape(capacity, 4)
    off = b.get(d_off, "behind the offsets").view(np.uint64)
    pts = b.get(d_pts, "behind the points") if with_points else None
    edges = b.get(d_edges).view(np.int16)[:n * h * w].reshape(n, h, w) if with_edges else None
    return rec, off, pts, edges


# ---- routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("h,w", [(70, 128), (70, 77)], ids=["70x128", "70x77"])
def test_behind_dev_canny_equals_the_rule_on_the_oracles_planes(hip, h, w, u8, fuse, tail):
    frames, maps, planes, want_rec, want_idx = reference(h, w)
    want = np.concatenate(want_rec).view(np.uint32)
    total = len(want)
    assert total > 100 and (er.unpack(want.view(np.int32))[6]).sum() > total // 4
    with hip.Context(0) as ctx:
        ctx.set_option("smoothed_u8", u8)
        ctx.set_option("fuse_classify", fuse)
        ctx.set_option("hysteresis_tail", tail)
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        rec, off, pts, edges = run_edgels(ctx, b, d_img, 3, h, w, total + 5)
        # the byte plane exists only between the two marching kernels of the fused route (which needs width % 8 == 0)
        assert ctx.get_option("last_canny_smoothed_u8") == (1 if u8 and fuse and w % 8 == 0 else 0)
        assert np.array_equal(edges, maps), "d_edges differs from the oracle's map"
        assert np.array_equal(off, csr(want_idx))
        assert np.array_equal(pts[:total], np.concatenate(want_idx)) and (pts[total:] == SENT).all()
        bad = np.flatnonzero((rec[:total] != want).any(axis=1))
        assert bad.size == 0, f"{bad.size} of {total} records differ, first {bad[0]}: {rec[bad[0]]} != {want[bad[0]]}"
        assert (rec[total:] == SENT).all(), "records past the count were written"
        # without d_edges and d_points: the same records
        rec2, off2, _, _ = run_edgels(ctx, b, d_img, 3, h, w, total, with_points=False, with_edges=False)
        assert np.array_equal(rec2, want) and np.array_equal(off2, off)
        b.free()


def test_capacity_and_the_map_rule(hip):
    h, w = 70, 128
    frames, maps, planes, want_rec, want_idx = reference(h, w)
    want, want_pts, want_off = np.concatenate(want_rec).view(np.uint32), np.concatenate(want_idx), csr(want_idx)
    total = len(want)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        for cap in (0, total, total - 1, 1):  # counts only, exact, one short, one record
            rec, off, pts, _ = run_edgels(ctx, b, d_img, 3, h, w, cap, with_edges=False)
            assert np.array_equal(off, want_off), f"capacity {cap}: the offsets are not the true counts"
            assert np.array_equal(rec, want[:cap]) and np.array_equal(pts, want_pts[:cap]), f"capacity {cap}"
        # max_val > 255 empties every map
        rec, off, pts, _ = run_edgels(ctx, b, d_img, 3, h, w, 16, with_edges=False, hi=300)
        assert not off.any() and (rec == SENT).all() and (pts == SENT).all()
        # statuses: nothing is written
        d_rec, d_off = b.filled(64), b.filled(8)
        for kw, status in ((dict(d_edgels=0, capacity=4), 1), (dict(d_edgels=d_rec + 4, capacity=4), 1),
                           (dict(d_offsets=0), 1), (dict(d_img=0), 1), (dict(lo=300), 5), (dict(h=1), 2)):  # min_val > 255 >= max_val: DOMAIN
            a = dict(d_img=d_img, lo=LO, h=h, d_edgels=d_rec, capacity=4, d_offsets=d_off)
            a.update(kw)
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_canny_edgels(a["d_img"], SIGMA, a["lo"], HI, a["h"], w, 3, a["d_edgels"], a["capacity"], a["d_offsets"])
            assert ei.value.status == status, kw
            assert (b.get(d_rec) == SENT).all() and (b.get(d_off) == SENT).all(), kw
        b.free()


def test_same_bytes_on_every_run_on_a_context_with_dirty_workspaces(hip):
    """A long-lived context that has run other analysis calls on other shapes first: their workspaces (row prefixes, planes)
    hold whatever those left."""
    h, w = 70, 128
    frames, maps, planes, want_rec, want_idx = reference(h, w)
    want = np.concatenate(want_rec).view(np.uint32)
    other = np.stack([synth_frame(96, 200, s) for s in (5, 6, 7, 8)])
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        ctx.canny_hough_circles(other, SIGMA, LO, HI, 5, 30, threshold=15, support_threshold=10, min_dist=8, centres_max=32)
        ctx.canny_contours(other, SIGMA, LO, HI)
        ctx.canny_edgels(other, 1.0, 20, 60)
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        ctx.profile_enable(True)
        ctx.profile_reset()
        runs = []
        for _ in range(3):
            rec, off, pts, _ = run_edgels(ctx, b, d_img, 3, h, w, len(want), with_edges=False)
            runs.append((rec.tobytes(), off.tobytes(), pts.tobytes()))
        assert runs[0] == runs[1] == runs[2] and runs[0][0] == want.tobytes()
        for part in (hip.EDGEL_PART_LAYOUT, hip.EDGEL_PART_REFINE):
            ms, launches = ctx.edgels_profile_get(part)
            assert launches == 3 and ms > 0.0
        assert ctx.polygons_profile_get(0)[1] == 0  # other features' slots are untouched
        ctx.profile_enable(False)
        with pytest.raises(hip.CannyHipError):
            ctx.edgels_profile_get(2)
        b.free()


def test_host_buffer_form_equals_the_device_form(hip):
    h, w = 70, 128
    frames, maps, planes, want_rec, want_idx = reference(h, w)
    want = np.concatenate(want_rec)
    with hip.Context(0) as ctx:
        rec, off, pts = ctx.canny_edgels(frames, SIGMA, LO, HI, want_points=True)
        assert np.array_equal(rec, want) and np.array_equal(off, csr(want_idx)) and np.array_equal(pts, np.concatenate(want_idx))
        rec, off = ctx.canny_edgels(frames, SIGMA, LO, HI, capacity=7)
        assert np.array_equal(rec, want[:7]) and np.array_equal(off, csr(want_idx))
        rec, off = ctx.canny_edgels(frames[0], SIGMA, LO, HI, capacity=0)
        assert rec.shape == (0, 4) and off[1] == len(want_idx[0])
        x, y = hip.edgels_xy(want)
        assert np.all(np.abs(x - np.concatenate(want_idx) % w) <= 0.5) and np.all(np.abs(y - np.concatenate(want_idx) // w) <= 0.5)


# ---- the rule at listed pixels ------------------------------------------------------------------------------------------
def run_at(ctx, b, planes, lists, capacity=None, d_plane=None):
    """dev_edgels_at on a batch of equally shaped planes (or the context's plane with d_plane = 0) -> records [capacity, 4]."""
    n, h, w = len(lists), planes[0].shape[0], planes[0].shape[1]
    flat = np.concatenate(lists).astype(np.uint32) if sum(len(l) for l in lists) else np.zeros(0, np.uint32)
    capacity = len(flat) if capacity is None else capacity
    if d_plane is None:
        d_plane = b.upload(np.stack(planes))
    d_pts, d_off, d_rec = b.upload(flat), b.upload(csr(lists)), b.filled(4 * capacity)
    ctx.dev_edgels_at(d_plane, planes[0].dtype == np.uint8, h, w, n, d_pts, d_off, d_rec, capacity)
    return b.get(d_rec, "behind the records").reshape(capacity, 4)


def beyond(h, w):
    return np.array([h * w, h * w + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_at_designed_planes_and_lists(hip, dtype):
    rng = np.random.default_rng(3)
    full = np.iinfo(dtype)
    tie = np.tile(np.array([0, 0, 10, 20, 30, 30, 30, 30], dtype), (6, 1))
    ramp = np.tile((10 * np.arange(8)).astype(dtype), (6, 1))
    every68 = np.concatenate([np.arange(48, dtype=np.uint32), beyond(6, 8)])
    designed = ([np.full((6, 8), 77, dtype), ramp, tie, rng.integers(full.min, full.max + 1, (6, 8)).astype(dtype)],
                [every68, every68[::-1], every68, np.zeros(0, np.uint32)])
    big = [rng.integers(full.min, full.max + 1, (37, 53)).astype(dtype) for _ in range(3)]
    mixed = rng.integers(0, 37 * 53, 700).astype(np.uint32)
    mixed[::9] = rng.integers(37 * 53, 2 ** 32, mixed[::9].size, dtype=np.uint64).astype(np.uint32)
    random = (big, [np.concatenate([np.arange(37 * 53, dtype=np.uint32), beyond(37, 53)]), np.zeros(0, np.uint32), mixed])
    thin = [([rng.integers(full.min, full.max + 1, s).astype(dtype) for _ in range(2)],
             [np.concatenate([np.arange(s[0] * s[1], dtype=np.uint32), beyond(*s)])] * 2) for s in ((2, 2), (2, 70), (70, 2))]
    yy, xx = np.mgrid[0:9, 0:11]
    border = np.flatnonzero(((yy == 0) | (yy == 8) | (xx == 0) | (xx == 10)).reshape(-1))
    borders = ([rng.integers(full.min, full.max + 1, (9, 11)).astype(dtype)], [border])
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for planes, lists in (designed, random, borders, *thin):
            want = np.concatenate([er.edgels_at(p, l) for p, l in zip(planes, lists)]).view(np.uint32)
            got = run_at(ctx, b, planes, lists)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"{planes[0].shape}: {bad.size} records differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
            assert np.array_equal(got.view(np.int32), np.concatenate(
                [hip.edgels_from_plane(p, l) for p, l in zip(planes, lists)])), "the host function differs"
            short = run_at(ctx, b, planes, lists, capacity=max(1, len(want) - 3))
            assert np.array_equal(short, want[:len(short)])
        invalid = hip.edgels_flags(run_at(ctx, b, *designed).view(np.int32))[2]
        assert invalid.sum() == 15
        b.free()


def test_at_the_chain_points_of_the_contours_on_the_contexts_plane(hip):
    h, w = 70, 128
    frames, maps, planes, _, _ = reference(h, w)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        d_plain, d_off = b.filled(4 * 16), b.filled(8)
        # a fresh context has no plane to offer: INVALID, nothing written
        for _ in range(2):
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_edgels_at(0, False, h, w, 3, b.upload(np.zeros(16, np.uint32)),
                                  b.upload(np.array([0, 5, 10, 16], np.uint64)), d_plain, 16)
            assert ei.value.status == 1 and (b.get(d_plain) == SENT).all()
            ctx.canny_points(frames[:2], SIGMA, LO, HI)  # ... and neither has one that ran another shape
        cap, pcap = 3 * h * w, 8 * 3 * h * w
        d_offsets, d_chain, d_pts, d_poff = b.filled(8), b.filled(2 * (cap + 1)), b.filled(pcap), b.filled(8)
        ctx.dev_canny_contours(d_img, SIGMA, LO, HI, h, w, 3, 1, 0, cap, d_offsets, d_chain, d_pts, pcap, d_poff)
        poff = b.get(d_poff).view(np.uint64)
        n_pts = int(poff[3])
        assert 300 < n_pts <= pcap
        d_rec = b.filled(4 * n_pts)
        ctx.dev_edgels_at(0, False, h, w, 3, d_pts, d_poff, d_rec, n_pts)
        got = b.get(d_rec).reshape(n_pts, 4)
        pts = b.get(d_pts)[:n_pts]
        want = np.concatenate([er.edgels_at(planes[f], pts[int(poff[f]):int(poff[f + 1])]) for f in range(3)]).view(np.uint32)
        assert np.array_equal(got, want)
        assert not hip.edgels_flags(got.view(np.int32))[2].any()
        # another shape on the same context, then the old shape again: INVALID, nothing written
        ctx.canny_points(frames[:, :64, :64].copy(), SIGMA, LO, HI)
        b.refill(d_rec)
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.dev_edgels_at(0, False, h, w, 3, d_pts, d_poff, d_rec, n_pts)
        assert ei.value.status == 1 and (b.get(d_rec) == SENT).all()
        b.free()


# ---- past the grid cap ----------------------------------------------------------------------------------------------------
def test_rows_past_the_grid_cap(hip):
    """4097 frames of 256 x 8 are 1,048,832 image rows, more than 16 * 65536: some wave takes a second row.  All frames are
    flat but a few at both ends of the batch, which hold a bright blob."""
    n, h, w = 4097, 256, 8
    assert hip.launch_plan("points_rows", n, h, w).trips == 2
    blob = np.full((h, w), 30, np.uint8)
    blob[100:141, 2:6] = 220
    blob2 = np.full((h, w), 200, np.uint8)
    blob2[7:250, 0:4] = 20
    frames = np.full((n, h, w), 30, np.uint8)
    where = {0: blob, 1: blob2, 4090: blob, 4095: blob2, 4096: blob}
    idx = [np.zeros(0, np.uint32)] * n
    rec = [np.zeros((0, 4), np.int32)] * n
    assert not oracle.canny(frames[2], SIGMA, LO, HI).any()
    for f, img in where.items():
        frames[f] = img
        idx[f] = np.flatnonzero(oracle.canny(img, SIGMA, LO, HI).reshape(-1)).astype(np.uint32)
        rec[f] = er.edgels_at(oracle.gaussian(img, SIGMA), idx[f])
    want, want_off = np.concatenate(rec).view(np.uint32), csr(idx)
    assert len(want) > 300
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        got, off, pts, _ = run_edgels(ctx, b, d_img, n, h, w, len(want) + 3, with_edges=False)
        assert np.array_equal(off, want_off)
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == SENT).all()
        assert np.array_equal(pts[:len(want)], np.concatenate(idx))
        b.free()


def test_at_past_the_grid_cap(hip):
    h, w = 16, 16
    rng = np.random.default_rng(8)
    planes = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(3)]
    per_trip = hip.edgels_plan(3, h, w, 1).grid * hip.edgels_plan(3, h, w, 1).per_group
    lists = [rng.integers(0, h * w + 20, per_trip * 3 + 5).astype(np.uint32), np.zeros(0, np.uint32),
             rng.integers(0, h * w, per_trip + 1).astype(np.uint32)]
    assert hip.edgels_plan(3, h, w, len(lists[0])).trips == 4 and hip.edgels_plan(3, h, w, len(lists[2])).trips == 2
    want = np.concatenate([er.edgels_at(p, l) for p, l in zip(planes, lists)]).view(np.uint32)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        assert np.array_equal(run_at(ctx, b, planes, lists), want)
        b.free()


# ---- the device arithmetic ------------------------------------------------------------------------------------------------
def test_device_arithmetic_on_the_whole_sobel_domain(hip):
    """(a) every pair of [-1020, 1020]^2, the corners of s16 and 2^20 random s16 pairs against math.isqrt and the octant
    test; (b) every triple of [0, 160)^3 and 2^20 random triples up to 741455 against the rule's offset."""
    rng = np.random.default_rng(17)
    side = np.arange(-1020, 1021, dtype=np.int16)
    ends = np.array([-32768, -32767, -1, 0, 1, 32766, 32767], np.int16)
    gx = np.concatenate([np.tile(side, side.size), np.repeat(ends, ends.size),
                         rng.integers(-32768, 32768, 1 << 20).astype(np.int16)])
    gy = np.concatenate([np.repeat(side, side.size), np.tile(ends, ends.size),
                         rng.integers(-32768, 32768, 1 << 20).astype(np.int16)])
    assert side.size ** 2 == 4165681
    small = np.arange(160, dtype=np.uint32)
    abc = np.concatenate([np.stack(np.meshgrid(small, small, small, indexing="ij"), axis=-1).reshape(-1, 3),
                          rng.integers(0, 741456, (1 << 20, 3)).astype(np.uint32)])
    abc[-(1 << 19):].sort(axis=1)  # half of the random ones with b as the median or ...
    abc[-(1 << 19):, [1, 2]] = abc[-(1 << 19):, [2, 1]]  # ... the largest: refined more often than a third of the time
    m = gx.astype(np.int64) ** 2 + gy.astype(np.int64) ** 2
    want_mag = np.array([math.isqrt(v) for v in (256 * m).tolist()], np.uint32)
    want_dir = er.direction(gx, gy).astype(np.int32)
    want_t, want_ok = er.offsets(abc[:, 0], abc[:, 1], abc[:, 2])
    assert want_ok[-(1 << 19):].mean() > 0.9 and np.abs(want_t).max() == 128
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_gx, d_gy, d_abc = b.upload(gx), b.upload(gy), b.upload(abc)
        d_mag, d_dir, d_t, d_ok = b.filled(gx.size), b.filled(gx.size), b.filled(len(abc)), b.filled(len(abc))
        ctx.dev_edgels_arith(d_gx, d_gy, gx.size, d_mag, d_dir, d_abc, len(abc), d_t, d_ok)
        for got, want, what in ((b.get(d_mag), want_mag, "mag_q4"), (b.get(d_dir).view(np.int32), want_dir, "dir"),
                                (b.get(d_t).view(np.int32), want_t.astype(np.int32), "t_q8"),
                                (b.get(d_ok).view(np.int32), want_ok.astype(np.int32), "refined")):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{what}: {bad.size} mismatches, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
        # either part alone
        b.refill(d_mag)
        ctx.dev_edgels_arith(0, 0, 0, 0, 0, d_abc, 10, d_t, d_ok)
        ctx.dev_edgels_arith(d_gx, d_gy, 10, d_mag, d_dir)
        assert np.array_equal(b.get(d_mag)[:10], want_mag[:10]) and (b.get(d_mag)[10:] == SENT).all()
        with pytest.raises(hip.CannyHipError):
            ctx.dev_edgels_arith(0, 0, 0, 0, 0)
        b.free()


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_cli_writes_the_edgels_of_a_frame(tmp_path):
    h, w = 70, 128
    frames, maps, planes, want_rec, want_idx = reference(h, w)
    pgm = tmp_path / "in.pgm"
    pgm.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + frames[0].tobytes())
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, str(SIGMA), str(LO), str(HI), "-i", str(pgm), "-o", str(tmp_path), "-e"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = (tmp_path / "canny_edgels.txt").read_text().splitlines()
    x, y, gx, gy, mag, d, refined, _ = er.unpack(want_rec[0])
    assert rows == ["%.3f %.3f %d %d %.4f %d %d" % v for v in zip(x, y, gx, gy, mag, d, refined)]
    assert len(rows) == len(want_idx[0]) > 50
