"""Edge point lists (canny_hip_dev_canny_points / canny_hip_canny_points / canny_hip_dev_points_from_bits): the edge map
compacted on the GPU to the ascending pixel indices r * width + c of every frame, CSR-shaped over the batch.

Reference: oracle.canny per frame -> np.flatnonzero.  Everything is integers, equality is exact.  Offsets and points are
checked separately so that a failure names which.  Every buffer is sized from the oracle's counts."""
import numpy as np
import pytest

import oracle
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
N_GUARD = 64
SHAPES = [(270, 480), (37, 53), (64, 8), (9, 2), (2, 9), (120, 1001), (256, 256), (130, 4096)]
SIGMAS = [1.0, 1.4]
THRESHOLDS = [(50, 150), (40, 120), (1, 1)]  # (1, 1): a dense map, a different regime for the scatter

_oracle_cache = {}


def _frames(n, h, w, seed0, first=None):
    fr = [synth_frame(h, w, seed0 + i) for i in range(n)]
    if first is not None:
        fr[0] = np.ascontiguousarray(first)
    return np.stack(fr)


def _oracle_maps(frames, sigma, lo, hi, key):
    """oracle.canny of every frame, cached per (key, sigma, lo, hi): the n = 1, 3, 23 batches share their frames."""
    k = (key, frames.shape, sigma, lo, hi)
    if k not in _oracle_cache:
        _oracle_cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _oracle_cache[k]


def _csr(maps):
    """(points uint32, offsets uint64) of a stack of maps, by definition."""
    lists = [np.flatnonzero(m).astype(np.uint32) for m in maps]
    offsets = np.zeros(len(lists) + 1, np.uint64)
    offsets[1:] = np.cumsum([l.size for l in lists], dtype=np.uint64)
    return (np.concatenate(lists) if lists else np.empty(0, np.uint32)), offsets


def _check_offsets(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, what
    assert got[0] == 0, f"{what}: offsets[0]"
    assert np.all(got[1:] >= got[:-1]), f"{what}: offsets not monotone"
    assert np.array_equal(got, want), f"{what}: offsets are not the true counts"


class _Dev:
    """Device buffers of one points call: input frames, a guarded points buffer, offsets, optionally the s16 map."""

    def __init__(self, ctx, frames, capacity, with_edges=False, with_points=True):
        self.ctx, self.frames, self.capacity = ctx, frames, int(capacity)
        self.n, self.h, self.w = frames.shape
        self.ptrs = []
        self.d_in = self._malloc(frames.nbytes)
        ctx.h2d(self.d_in, frames)
        self.d_pts = 0
        if with_points:
            self.d_pts = self._malloc(4 * (self.capacity + N_GUARD))
            ctx.h2d(self.d_pts, np.full(self.capacity + N_GUARD, GUARD, np.uint32))
        self.d_off = self._malloc(8 * (self.n + 1))
        ctx.h2d(self.d_off, np.full(self.n + 1, 0xEEEEEEEEEEEEEEEE, np.uint64))
        self.d_edges = self._malloc(frames.nbytes * 2) if with_edges else 0
        if with_edges:
            ctx.h2d(self.d_edges, np.full(frames.shape, 0x5A5A, np.int16))

    def _malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def run(self, sigma, lo, hi):
        self.ctx.dev_canny_points(self.d_in, sigma, lo, hi, self.h, self.w, self.n, self.d_pts,
                                  self.capacity if self.d_pts else 0, self.d_off, self.d_edges)

    def offsets(self):
        out = np.empty(self.n + 1, np.uint64)
        self.ctx.d2h(out, self.d_off)
        return out

    def points_and_guard(self):
        out = np.empty(self.capacity + N_GUARD, np.uint32)
        self.ctx.d2h(out, self.d_pts)
        return out[:self.capacity], out[self.capacity:]

    def edges(self):
        out = np.empty(self.frames.shape, np.int16)
        self.ctx.d2h(out, self.d_edges)
        return out

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_dev_call(ctx, frames, maps, sigma, lo, hi, what, with_edges=True):
    want_pts, want_off = _csr(maps)
    with _Dev(ctx, frames, want_pts.size, with_edges=with_edges) as d:
        d.run(sigma, lo, hi)
        _check_offsets(d.offsets(), want_off, what)
        pts, guard = d.points_and_guard()
        assert np.array_equal(pts, want_pts), f"{what}: points differ"
        assert np.all(guard == GUARD), f"{what}: guard words written"
        if with_edges:
            assert np.array_equal(d.edges(), maps), f"{what}: the s16 map differs from the oracle"


@pytest.mark.parametrize("thr", THRESHOLDS, ids=lambda t: f"thr{t[0]}_{t[1]}")
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_points_match_the_oracle(hip, fixture_image, shape, sigma, thr):
    h, w = shape
    lo, hi = thr
    all_frames = _frames(23, h, w, 300 + h + w, first=fixture_image if shape == (256, 256) else None)
    all_maps = _oracle_maps(all_frames, sigma, lo, hi, "main")
    with hip.Context(0) as ctx:
        for n in (1, 3, 23):
            frames, maps = all_frames[:n], all_maps[:n]
            what = f"{shape} sigma={sigma} thr={thr} n={n}"
            _check_dev_call(ctx, frames, maps, sigma, lo, hi, "dev_canny_points " + what)
            want_pts, want_off = _csr(maps)
            pts, off = ctx.canny_points(frames, sigma, lo, hi)
            _check_offsets(off, want_off, "canny_points " + what)
            assert pts.dtype == np.uint32 and np.array_equal(pts, want_pts), f"canny_points {what}: points differ"


@pytest.mark.parametrize("thr", THRESHOLDS, ids=lambda t: f"thr{t[0]}_{t[1]}")
@pytest.mark.parametrize("sigma", SIGMAS)
def test_points_of_a_4k_batch(hip, sigma, thr):
    lo, hi = thr
    frames = _frames(4, 2160, 3840, 11)
    maps = _oracle_maps(frames, sigma, lo, hi, "4k")
    with hip.Context(0) as ctx:
        _check_dev_call(ctx, frames, maps, sigma, lo, hi, f"dev_canny_points 4K sigma={sigma} thr={thr}")
        want_pts, want_off = _csr(maps)
        pts, off = ctx.canny_points(frames, sigma, lo, hi)
        _check_offsets(off, want_off, f"canny_points 4K sigma={sigma} thr={thr}")
        assert np.array_equal(pts, want_pts), f"canny_points 4K sigma={sigma} thr={thr}: points differ"


@pytest.mark.parametrize("shape", [(270, 480), (45, 77)])
def test_empty_segments_in_the_middle_of_the_csr(hip, shape):
    h, w = shape
    frames = _frames(7, h, w, 60)
    for i in (0, 2, 3, 6):  # black frames first, in the middle (two in a row) and last
        frames[i] = 0
    maps = _oracle_maps(frames, 1.4, 50, 150, "black")
    want_pts, want_off = _csr(maps)
    assert want_off[1] == 0 and want_off[3] == want_off[4] == want_off[2] and want_off[7] == want_off[6]
    assert want_pts.size > 0
    with hip.Context(0) as ctx:
        _check_dev_call(ctx, frames, maps, 1.4, 50, 150, f"black frames {shape}")
        pts, off = ctx.canny_points(frames, 1.4, 50, 150)
        _check_offsets(off, want_off, f"canny_points black frames {shape}")
        assert np.array_equal(pts, want_pts)


def test_max_val_above_255_gives_empty_lists(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300, "hi300")
    assert not maps.any(), "the oracle's map is all zero for max_val = 300"
    busy = _csr(_oracle_maps(frames, 1.0, 50, 150, "hi300"))[0].size
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, busy, with_edges=True) as d:
            d.run(1.0, 50, 300)
            _check_offsets(d.offsets(), np.zeros(4, np.uint64), "max_val=300")
            pts, guard = d.points_and_guard()
            assert np.all(pts == GUARD) and np.all(guard == GUARD), "max_val=300: points written"
            assert np.array_equal(d.edges(), maps)
        pts, off = ctx.canny_points(frames, 1.0, 50, 300)
        assert pts.size == 0 and np.array_equal(off, np.zeros(4, np.uint64))


def _plain_status(hip, ctx, frames, sigma, lo, hi):
    """Status of canny_hip_dev_canny for these arguments (0 = OK)."""
    n, h, w = frames.shape
    d_in, d_edges = ctx.malloc(frames.nbytes), ctx.malloc(frames.nbytes * 2)
    try:
        ctx.h2d(d_in, frames)
        try:
            ctx.dev_canny(d_in, sigma, lo, hi, h, w, n, d_edges)
        except hip.CannyHipError as e:
            return e.status
        return 0
    finally:
        ctx.free(d_in)
        ctx.free(d_edges)


@pytest.mark.parametrize("thr", [(0, 150), (300, 100), (-3, 150)], ids=lambda t: f"thr{t[0]}_{t[1]}")
def test_status_is_dev_cannys_and_a_rejected_call_writes_nothing(hip, thr):
    """min_val = 0 and the other corners of the threshold domain: the points call returns the status canny_hip_dev_canny
    returns for the same arguments.  (dev_canny ACCEPTS min_val <= 0 on a whole pipeline -- suppressed magnitudes are
    never negative, so no candidate lies below min_val and the reference's scan order cannot matter -- and rejects
    min_val > 255 >= max_val with CANNY_HIP_ERR_DOMAIN.)  Rejected: nothing is written.  Accepted: the oracle's lists."""
    lo, hi = thr
    frames = _frames(2, 64, 64, 9)
    with hip.Context(0) as ctx:
        plain = _plain_status(hip, ctx, frames, 1.0, lo, hi)
        if thr == (300, 100):
            assert plain == 5  # CANNY_HIP_ERR_DOMAIN
        if plain == 0:
            maps = _oracle_maps(frames, 1.0, lo, hi, "status")
            _check_dev_call(ctx, frames, maps, 1.0, lo, hi, f"thr={thr}")
            pts, off = ctx.canny_points(frames, 1.0, lo, hi)
            _check_offsets(off, _csr(maps)[1], f"canny_points thr={thr}")
            assert np.array_equal(pts, _csr(maps)[0])
            return
        with _Dev(ctx, frames, 256, with_edges=True) as d:
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1.0, lo, hi)
            assert ei.value.status == plain
            ctx.synchronize()
            pts, guard = d.points_and_guard()
            assert np.all(pts == GUARD) and np.all(guard == GUARD)
            assert np.all(d.offsets() == 0xEEEEEEEEEEEEEEEE)
            assert np.all(d.edges() == 0x5A5A)
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.canny_points(frames, 1.0, lo, hi)
        assert ei.value.status == plain


@pytest.mark.parametrize("thr", [(50, 150), (1, 1)], ids=lambda t: f"thr{t[0]}_{t[1]}")
def test_overflow_keeps_the_exact_prefix(hip, thr):
    lo, hi = thr
    frames = _frames(5, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, lo, hi, "overflow")
    want_pts, want_off = _csr(maps)
    total = want_pts.size
    assert total > 2
    with hip.Context(0) as ctx:
        for cap in (total - 1, total // 2, 0):
            with _Dev(ctx, frames, cap) as d:  # capacity 0 WITH a real buffer: nothing may be written to it
                d.ctx.dev_canny_points(d.d_in, 1.4, lo, hi, d.h, d.w, d.n, d.d_pts, cap, d.d_off, 0)
                _check_offsets(d.offsets(), want_off, f"capacity={cap}")
                pts, guard = d.points_and_guard()
                assert np.array_equal(pts, want_pts[:cap]), f"capacity={cap}: the prefix differs"
                assert np.all(guard == GUARD), f"capacity={cap}: written past points + capacity"
            pts, off = ctx.canny_points(frames, 1.4, lo, hi, capacity=cap)
            _check_offsets(off, want_off, f"canny_points capacity={cap}")
            assert np.array_equal(pts, want_pts[:cap])
        # counts only: no points buffer at all
        with _Dev(ctx, frames, 0, with_points=False) as d:
            d.run(1.4, lo, hi)
            _check_offsets(d.offsets(), want_off, "counts only")
        # a capacity without a buffer is an argument error
        with _Dev(ctx, frames, 0, with_points=False) as d:
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_canny_points(d.d_in, 1.4, lo, hi, d.h, d.w, d.n, 0, 8, d.d_off, 0)
            assert ei.value.status == 1


@pytest.mark.parametrize("density", [0.0, 0.03, 0.5, 1.0])
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (9, 2), (37, 53), (64, 8), (120, 1001), (270, 480), (3, 4600)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_dev_points_from_bits(hip, shape, density):
    h, w = shape
    n = 3
    rng = np.random.default_rng(17 * h + w)
    masks = rng.random((n, h, w)) < density
    bits = np.packbits(masks, axis=-1)
    if w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)  # padding bits deliberately set: they are not pixels
    lists = [hip.points_from_bits(b, h, w) for b in bits]
    want_pts = np.concatenate(lists)
    want_off = np.zeros(n + 1, np.uint64)
    want_off[1:] = np.cumsum([l.size for l in lists], dtype=np.uint64)
    assert np.array_equal(want_pts, _csr(masks)[0])
    cap = want_pts.size
    with hip.Context(0) as ctx:
        d_bits, d_pts, d_off = ctx.malloc(bits.nbytes + 32), ctx.malloc(4 * (cap + N_GUARD)), ctx.malloc(8 * (n + 1))
        try:
            for shift in (0, 1, 16):
                ctx.h2d(d_bits + shift, bits)
                ctx.h2d(d_pts, np.full(cap + N_GUARD, GUARD, np.uint32))
                ctx.h2d(d_off, np.full(n + 1, 0xEEEEEEEEEEEEEEEE, np.uint64))
                ctx.dev_points_from_bits(d_bits + shift, h, w, n, d_pts, cap, d_off)
                off, pts = np.empty(n + 1, np.uint64), np.empty(cap + N_GUARD, np.uint32)
                ctx.d2h(off, d_off)
                ctx.d2h(pts, d_pts)
                _check_offsets(off, want_off, f"{shape} density={density} shift={shift}")
                assert np.array_equal(pts[:cap], want_pts), f"{shape} density={density} shift={shift}: points differ"
                assert np.all(pts[cap:] == GUARD)
        finally:
            for p in (d_bits, d_pts, d_off):
                ctx.free(p)


def test_formats_agree_and_no_workspace_is_clobbered(hip):
    h, w, n = 96, 256, 4
    frames = _frames(n, h, w, 900)
    maps = _oracle_maps(frames, 1.4, 40, 120, "formats")
    want_pts, want_off = _csr(maps)
    with hip.Context(0) as ctx:
        d_in, d_map, d_bits = ctx.malloc(frames.nbytes), ctx.malloc(frames.nbytes * 2), ctx.malloc(n * h * (w // 8))
        try:
            ctx.h2d(d_in, frames)

            def s16():
                ctx.dev_canny(d_in, 1.4, 40, 120, h, w, n, d_map)
                out = np.empty(frames.shape, np.int16)
                ctx.d2h(out, d_map)
                return out

            before = s16()
            ctx.dev_canny_bits(d_in, 1.4, 40, 120, h, w, n, d_bits)
            bits = np.empty(hip.bits_shape(frames.shape), np.uint8)
            ctx.d2h(bits, d_bits)
            _check_dev_call(ctx, frames, maps, 1.4, 40, 120, "formats", with_edges=False)
            after = s16()
            assert np.array_equal(before, maps) and np.array_equal(after, maps), "dev_canny changed by a points call"
            from_bits, from_map = _csr(hip.unpack_bits(bits, w))[0], _csr(before)[0]
            assert np.array_equal(from_bits, want_pts) and np.array_equal(from_map, want_pts)
            # ... and the bit map, compacted on the device, is the same list again
            d_pts, d_off = ctx.malloc(4 * max(want_pts.size, 4)), ctx.malloc(8 * (n + 1))
            try:
                ctx.dev_points_from_bits(d_bits, h, w, n, d_pts, want_pts.size, d_off)
                pts, off = np.empty(want_pts.size, np.uint32), np.empty(n + 1, np.uint64)
                ctx.d2h(pts, d_pts)
                ctx.d2h(off, d_off)
                _check_offsets(off, want_off, "bits -> points")
                assert np.array_equal(pts, want_pts)
            finally:
                ctx.free(d_pts)
                ctx.free(d_off)
        finally:
            for p in (d_in, d_map, d_bits):
                ctx.free(p)


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("option", ["smoothed_u8", "fuse_classify", "hysteresis_tail", "overlap_hysteresis"])
def test_every_route_through_canny_gives_the_same_lists(hip, option, value):
    """The list is read from hysteresis' strong plane: every route through dev_canny has to leave the converged plane of
    the whole batch there.  17 frames, so that overlap_hysteresis really splits the batch; a width that is a multiple of
    8 (the fused routes) and one that is not (Sobel+NMS, then the separate hysteresis kernels)."""
    for shape in ((96, 256), (45, 77), (130, 4096)):
        h, w = shape
        n = 17 if shape != (130, 4096) else 16
        frames = _frames(n, h, w, 4000 + w)
        maps = _oracle_maps(frames, 1.4, 40, 120, "routes")
        with hip.Context(0) as ctx:
            ctx.set_option(option, value)
            _check_dev_call(ctx, frames, maps, 1.4, 40, 120, f"{option}={value} {shape}")
            _check_dev_call(ctx, frames[:3], maps[:3], 1.4, 40, 120, f"{option}={value} {shape} n=3", with_edges=False)


def test_two_calls_give_identical_bytes(hip):
    frames = _frames(6, 270, 480, 77)
    total = _csr(_oracle_maps(frames, 1.0, 1, 1, "determinism"))[0].size
    with hip.Context(0) as ctx:
        runs = []
        for _ in range(2):
            with _Dev(ctx, frames, total) as d:
                d.run(1.0, 1, 1)
                runs.append((d.points_and_guard()[0].tobytes(), d.offsets().tobytes()))
        assert runs[0] == runs[1]
        a, b = ctx.canny_points(frames, 1.0, 1, 1), ctx.canny_points(frames, 1.0, 1, 1)
        assert a[0].tobytes() == b[0].tobytes() == runs[0][0] and a[1].tobytes() == b[1].tobytes()


def test_points_call_after_an_unflushed_stream_call(hip):
    """dev_canny_stream leaves its sweeps in flight (hysteresis_tail = 0: the route that defers its host round trip); the
    points call flushes them, compacts ITS batch, and the streamed batch's map is still right."""
    h, w = 96, 256
    streamed, mine = _frames(5, h, w, 1200), _frames(3, h, w, 1300)
    streamed_maps = _oracle_maps(streamed, 1.4, 50, 150, "streamed")
    maps = _oracle_maps(mine, 1.4, 50, 150, "mine")
    want_pts, want_off = _csr(maps)
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", 0)
        d_in, d_map = ctx.malloc(streamed.nbytes), ctx.malloc(streamed.nbytes * 2)
        try:
            ctx.h2d(d_in, streamed)
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            with _Dev(ctx, mine, want_pts.size, with_edges=True) as d:
                d.run(1.4, 50, 150)
                _check_offsets(d.offsets(), want_off, "after a streamed call")
                assert np.array_equal(d.points_and_guard()[0], want_pts)
                assert np.array_equal(d.edges(), maps)
            got = np.empty(streamed.shape, np.int16)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map"
        finally:
            ctx.free(d_in)
            ctx.free(d_map)


def test_compact_stage_is_timed(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150, "timed")
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << hip.STAGE_COMPACT)
        _check_dev_call(ctx, frames, maps, 1.4, 50, 150, "profiled", with_edges=False)
        ms, launches = ctx.profile_get(hip.STAGE_COMPACT)
        assert launches == 2 and ms > 0.0  # count + scan, scatter
        assert ctx.profile_get(hip.STAGE_GAUSSIAN)[1] == 0
