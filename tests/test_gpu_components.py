"""Connected components on the GPU (canny_hip_dev_canny_components / canny_hip_dev_components_bits /
canny_hip_canny_components): 8-connected labelling of the finished edge map per frame of a batch, with per-component
records and a minimum-area filter, CSR-shaped over the batch.

Reference: oracle.canny per frame -> the numpy rule of tests/components_rule.py.  Everything is integers, equality is exact.
labels, kept_u8, stats and offsets are checked separately so that a failure names which.  Every output buffer is pre-filled
with a pattern and followed by guard words."""
import os
import subprocess

import numpy as np
import pytest

import components_rule as rule
import oracle
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = np.int32(0x5A5A5A5A)
GUARD8 = np.uint8(0xA5)
N_GUARD = 64
OFF_FILL = 0xEEEEEEEEEEEEEEEE
SHAPES = [(270, 480), (37, 53), (64, 8), (9, 2), (2, 9), (120, 1001), (256, 256), (130, 4096)]
MIN_AREAS = [1, 5, 20]

_oracle_cache = {}


def _frames(n, h, w, seed0, first=None):
    fr = [synth_frame(h, w, seed0 + i) for i in range(n)]
    if first is not None:
        fr[0] = np.ascontiguousarray(first)
    return np.stack(fr)


def _oracle_maps(frames, sigma, lo, hi, key):
    k = (key, frames.shape, sigma, lo, hi)
    if k not in _oracle_cache:
        _oracle_cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _oracle_cache[k]


def _check_offsets(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, what
    assert got[0] == 0, f"{what}: offsets[0]"
    assert np.array_equal(got, want), f"{what}: offsets are not the true counts"


class _Dev:
    """Device buffers of one components call.  source: frames uint8 [n, h, w] (the canny route) or, with bits=True, packed
    bit maps [n, h, ceil(w / 8)] placed `shift` bytes into their allocation."""

    def __init__(self, ctx, source, capacity, h=None, w=None, bits=False, shift=0, labels=True, kept=True, stats=True,
                 edges=False):
        self.ctx, self.capacity, self.bits = ctx, int(capacity), bits
        self.n = source.shape[0]
        self.h, self.w = (h, w) if bits else source.shape[1:]
        self.npx = self.n * self.h * self.w
        self.ptrs = []
        self.d_src = self._malloc(source.nbytes + shift + 16) + shift
        ctx.h2d(self.d_src, source)
        self.d_labels = self._filled(np.full(self.npx + N_GUARD, GUARD32, np.int32)) if labels else 0
        self.d_kept = self._filled(np.full(self.npx + N_GUARD, GUARD8, np.uint8)) if kept else 0
        self.d_stats = self._filled(np.full((self.capacity + N_GUARD) * 6, GUARD32, np.int32)) if stats else 0
        self.d_off = self._filled(np.full(self.n + 1, OFF_FILL, np.uint64))
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
        cap = self.capacity if self.d_stats else 0
        if self.bits:
            self.ctx.dev_components_bits(self.d_src, self.h, self.w, self.n, min_area, self.d_labels, self.d_kept,
                                         self.d_stats, cap, self.d_off)
        else:
            self.ctx.dev_canny_components(self.d_src, sigma, lo, hi, self.h, self.w, self.n, min_area, self.d_labels,
                                          self.d_kept, self.d_stats, cap, self.d_off, self.d_edges)

    def _get(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        self.ctx.d2h(out, ptr)
        return out

    def offsets(self):
        return self._get(self.d_off, self.n + 1, np.uint64)

    def labels(self):
        a = self._get(self.d_labels, self.npx + N_GUARD, np.int32)
        return a[:self.npx].reshape(self.n, self.h, self.w), a[self.npx:]

    def kept(self):
        a = self._get(self.d_kept, self.npx + N_GUARD, np.uint8)
        return a[:self.npx].reshape(self.n, self.h, self.w), a[self.npx:]

    def stats(self):
        a = self._get(self.d_stats, (self.capacity + N_GUARD) * 6, np.int32)
        return a[:self.capacity * 6].reshape(self.capacity, 6), a[self.capacity * 6:]

    def edges(self):
        return self._get(self.d_edges, self.npx, np.int16).reshape(self.n, self.h, self.w)

    def check(self, want, what):
        """want = rule.csr(...): every output that exists against it, each named."""
        want_l, want_s, want_off = want
        _check_offsets(self.offsets(), want_off, what)
        if self.d_labels:
            got, guard = self.labels()
            assert np.array_equal(got, want_l), f"{what}: labels differ"
            assert np.all(guard == GUARD32), f"{what}: written past labels"
        if self.d_kept:
            got, guard = self.kept()
            assert np.array_equal(got, np.where(want_l != 0, 255, 0).astype(np.uint8)), f"{what}: kept_u8 differs"
            assert np.all(guard == GUARD8), f"{what}: written past kept_u8"
        if self.d_stats:
            got, guard = self.stats()
            n = min(self.capacity, want_s.shape[0])
            assert np.array_equal(got[:n], want_s[:n]), f"{what}: stats differ"
            assert np.all(got[n:] == GUARD32) and np.all(guard == GUARD32), f"{what}: written past the records that fit"

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_canny_call(ctx, frames, maps, sigma, lo, hi, min_area, what, edges=True, **outs):
    want = rule.csr(maps, min_area)
    with _Dev(ctx, frames, want[1].shape[0], edges=edges, **outs) as d:
        d.run(min_area, sigma, lo, hi)
        d.check(want, what)
        if edges:
            assert np.array_equal(d.edges(), maps), f"{what}: the s16 map differs from the oracle"
    return want


def _check_bits_call(ctx, masks, min_area, what, shift=0, pad_ones=False, **outs):
    n, h, w = masks.shape
    bits = np.packbits(masks, axis=-1)
    if pad_ones and w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want = rule.csr(masks, min_area)
    with _Dev(ctx, bits, want[1].shape[0], h=h, w=w, bits=True, shift=shift, **outs) as d:
        d.run(min_area)
        d.check(want, what)
    return want


@pytest.mark.parametrize("min_area", MIN_AREAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_components_match_the_rule_on_the_oracles_maps(hip, fixture_image, shape, min_area):
    h, w = shape
    all_frames = _frames(23, h, w, 300 + h + w, first=fixture_image if shape == (256, 256) else None)
    for sigma, (lo, hi) in ((1.4, (50, 150)), (1.0, (1, 1))):   # (1, 1): a dense map, few large components
        all_maps = _oracle_maps(all_frames, sigma, lo, hi, "main")
        with hip.Context(0) as ctx:
            for n in (1, 3, 23):
                frames, maps = all_frames[:n], all_maps[:n]
                what = f"{shape} sigma={sigma} thr=({lo},{hi}) min_area={min_area} n={n}"
                _check_canny_call(ctx, frames, maps, sigma, lo, hi, min_area, "d_edges given, " + what, edges=True)
                _check_canny_call(ctx, frames, maps, sigma, lo, hi, min_area, "d_edges NULL, " + what, edges=False)


def test_the_synthetic_frame_of_the_issue(hip):
    frames = _frames(1, 480, 640, 1)
    maps = _oracle_maps(frames, 1.4, 50, 150, "issue")
    with hip.Context(0) as ctx:
        for min_area, k in ((0, 419), (1, 419), (44, 0), (480 * 640 + 1, 0)):
            want = _check_canny_call(ctx, frames, maps, 1.4, 50, 150, min_area, f"min_area={min_area}")
            assert want[1].shape[0] == k
        want = _check_canny_call(ctx, frames, maps, 1.4, 50, 150, 5, "min_area=5")
        assert 0 < want[1].shape[0] < 419


@pytest.mark.parametrize("min_area", [1, 20])
def test_components_of_a_4k_frame(hip, min_area):
    frames = _frames(1, 2160, 3840, 11)
    maps = _oracle_maps(frames, 1.4, 50, 150, "4k")
    with hip.Context(0) as ctx:
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, min_area, f"4K min_area={min_area}")


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("option", ["smoothed_u8", "fuse_classify", "hysteresis_tail", "overlap_hysteresis"])
def test_every_route_through_canny_gives_the_same_components(hip, option, value):
    """The labelling reads hysteresis' strong plane: every route through dev_canny has to leave the converged plane of the
    whole batch there.  17 frames, so that overlap_hysteresis really splits the batch; a width that is a multiple of 8 (the
    fused routes) and one that is not (Sobel+NMS, then the separate hysteresis kernels)."""
    for shape in ((96, 256), (45, 77), (130, 4096)):
        h, w = shape
        n = 17 if shape != (130, 4096) else 16
        frames = _frames(n, h, w, 4000 + w)
        maps = _oracle_maps(frames, 1.4, 40, 120, "routes")
        with hip.Context(0) as ctx:
            ctx.set_option(option, value)
            _check_canny_call(ctx, frames, maps, 1.4, 40, 120, 3, f"{option}={value} {shape}")
            _check_canny_call(ctx, frames[:3], maps[:3], 1.4, 40, 120, 1, f"{option}={value} {shape} n=3", edges=False)


def test_components_call_after_an_unflushed_stream_call(hip):
    h, w = 96, 256
    streamed, mine = _frames(5, h, w, 1200), _frames(3, h, w, 1300)
    streamed_maps = _oracle_maps(streamed, 1.4, 50, 150, "streamed")
    maps = _oracle_maps(mine, 1.4, 50, 150, "mine")
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", 0)
        d_in, d_map = ctx.malloc(streamed.nbytes), ctx.malloc(streamed.nbytes * 2)
        try:
            ctx.h2d(d_in, streamed)
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_canny_call(ctx, mine, maps, 1.4, 50, 150, 2, "after a streamed call")
            got = np.empty(streamed.shape, np.int16)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map"
            # ... and the bits form flushes a pending lane as well
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_bits_call(ctx, maps != 0, 2, "bits form after a streamed call")
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map (2)"
        finally:
            ctx.free(d_in)
            ctx.free(d_map)


@pytest.mark.parametrize("min_area", [1, 4])
def test_every_combination_of_null_outputs(hip, min_area):
    frames = _frames(3, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150, "nulls")
    want = rule.csr(maps, min_area)
    K = want[1].shape[0]
    assert K > 2
    with hip.Context(0) as ctx:
        for labels in (False, True):
            for kept in (False, True):
                for stats in (False, True):
                    what = f"labels={labels} kept={kept} stats={stats}"
                    _check_canny_call(ctx, frames, maps, 1.4, 50, 150, min_area, what, edges=False, labels=labels,
                                      kept=kept, stats=stats)
                    _check_bits_call(ctx, maps != 0, min_area, "bits, " + what, labels=labels, kept=kept, stats=stats)


@pytest.mark.parametrize("min_area", [1, 4])
def test_capacity_bounds_the_records_never_the_counts(hip, min_area):
    frames = _frames(5, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150, "capacity")
    want = rule.csr(maps, min_area)
    K = want[1].shape[0]
    assert K > 8
    with hip.Context(0) as ctx:
        for cap in (K, K - 1, K // 2, 1, 0, K + 9):   # 0 WITH a real buffer: nothing may be written to it
            with _Dev(ctx, frames, cap) as d:
                d.ctx.dev_canny_components(d.d_src, 1.4, 50, 150, d.h, d.w, d.n, min_area, d.d_labels, d.d_kept,
                                           d.d_stats, cap, d.d_off, 0)
                d.check(want, f"capacity={cap}")
            l, k, s, off = ctx.canny_components(frames, 1.4, 50, 150, min_area, want_kept=True, capacity=cap)
            _check_offsets(off, want[2], f"canny_components capacity={cap}")
            assert np.array_equal(s, want[1][:cap]) and np.array_equal(l, want[0])
        with _Dev(ctx, frames, 0, stats=False) as d:   # a capacity without a buffer is an argument error
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_canny_components(d.d_src, 1.4, 50, 150, d.h, d.w, d.n, min_area, d.d_labels, d.d_kept, 0, 8,
                                         d.d_off, 0)
            assert ei.value.status == 1
            ctx.synchronize()
            assert np.all(d.offsets() == OFF_FILL) and np.all(d.labels()[0] == GUARD32)


def test_bits_source_agrees_with_the_canny_route(hip):
    h, w, n = 45, 77, 4
    frames = _frames(n, h, w, 900)
    maps = _oracle_maps(frames, 1.4, 40, 120, "formats")
    with hip.Context(0) as ctx:
        d_in, d_bits = ctx.malloc(frames.nbytes), ctx.malloc(n * h * ((w + 7) // 8))
        try:
            ctx.h2d(d_in, frames)
            ctx.dev_canny_bits(d_in, 1.4, 40, 120, h, w, n, d_bits)
            bits = np.empty(hip.bits_shape(frames.shape), np.uint8)
            ctx.d2h(bits, d_bits)
        finally:
            ctx.free(d_in)
            ctx.free(d_bits)
        assert np.array_equal(hip.unpack_bits(bits, w) != 0, maps != 0)
        for min_area in (1, 3):
            a = _check_canny_call(ctx, frames, maps, 1.4, 40, 120, min_area, "canny route")
            for shift in (0, 1, 3):   # an odd byte address, padding bits set
                b = _check_bits_call(ctx, hip.unpack_bits(bits, w) != 0, min_area, f"bits route shift={shift}",
                                     shift=shift, pad_ones=True)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("density", [0.05, 0.3, 0.6, 0.9])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (37, 63), (40, 64), (33, 65), (50, 77), (66, 129), (200, 333),
                                   (3, 4600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_masks_through_the_bits_route(hip, shape, density):
    h, w = shape
    masks = np.random.default_rng(17 * h + w).random((3, h, w)) < density
    with hip.Context(0) as ctx:
        for min_area in (1, 2, 5):
            _check_bits_call(ctx, masks, min_area, f"{shape} density={density} min_area={min_area}", shift=1,
                             pad_ones=True)


@pytest.mark.parametrize("shape", [(1024, 1024), (300, 400), (129, 131), (64, 8), (9, 2), (2, 9)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_directed_masks_through_the_bits_route(hip, shape):
    h, w = shape
    named = rule.directed_masks(h, w)
    masks = np.stack(list(named.values()))
    with hip.Context(0) as ctx:
        for min_area in (1, 2):
            want = _check_bits_call(ctx, masks, min_area, f"directed {shape} min_area={min_area}: {list(named)}",
                                    pad_ones=True)
            if min_area == 1 and h >= 9 and w >= 9:
                counts = dict(zip(named, np.diff(want[2]).astype(int)))
                assert counts["serpentine"] == counts["spiral"] == counts["staircase"] == counts["diagonal_pair"] == 1
                assert counts["combs"] == 2 and counts["all_set"] == 1 and counts["all_clear"] == 0
                assert counts["checkerboard"] == ((h + 1) // 2) * ((w + 1) // 2)


def test_max_val_above_255_follows_the_map(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300, "hi300")
    assert not maps.any(), "the oracle's map is all zero for max_val = 300"
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 64, edges=True) as d:
            d.run(1, 1.0, 50, 300)
            d.check(rule.csr(maps, 1), "max_val=300")
            assert np.array_equal(d.edges(), maps)
        l, k, s, off = ctx.canny_components(frames, 1.0, 50, 300, want_kept=True)
        assert s.shape == (0, 6) and not off.any() and not l.any() and not k.any()


def test_a_rejected_call_writes_nothing(hip):
    frames = _frames(2, 64, 64, 9)
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, 256, edges=True) as d:
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1, 1.0, 300, 100)
            assert ei.value.status == 5   # CANNY_HIP_ERR_DOMAIN, dev_canny's own
            ctx.synchronize()
            assert np.all(d.offsets() == OFF_FILL)
            assert np.all(d.labels()[0] == GUARD32) and np.all(d.kept()[0] == GUARD8)
            assert np.all(d.stats()[0] == GUARD32) and np.all(d.edges() == 0x5A5A)
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.canny_components(frames, 1.0, 300, 100)
        assert ei.value.status == 5


def test_same_bytes_on_every_run(hip):
    frames = _frames(6, 270, 480, 77)
    maps = _oracle_maps(frames, 1.0, 1, 1, "determinism")
    K = rule.csr(maps, 2)[1].shape[0]
    with hip.Context(0) as ctx:
        runs = []
        for k in range(3):
            if k == 2:   # an unrelated call on the context in between
                ctx.canny_points(_frames(2, 96, 256, 1), 1.4, 50, 150)
            with _Dev(ctx, frames, K) as d:
                d.run(2, 1.0, 1, 1)
                runs.append((d.labels()[0].tobytes(), d.kept()[0].tobytes(), d.stats()[0].tobytes(),
                             d.offsets().tobytes()))
        assert runs[0] == runs[1] == runs[2]


def test_host_form_and_its_capacity_recall(hip):
    # noise frames: many small components, more records than canny_components allots at first (max(1024, pixels / 64))
    noise = np.random.default_rng(5).integers(0, 256, (4, 96, 160), dtype=np.uint8)
    want_l, want_s, want_off = rule.csr(_oracle_maps(noise, 0.5, 60, 120, "noise"), 1)
    assert want_s.shape[0] > 1024, "the re-call with the exact size is exercised"
    frames = _frames(3, 270, 480, 31)
    maps = _oracle_maps(frames, 1.4, 50, 150, "host")
    with hip.Context(0) as ctx:
        l, k, s, off = ctx.canny_components(noise, 0.5, 60, 120)
        _check_offsets(off, want_off, "canny_components, re-call")
        assert k is None and np.array_equal(l, want_l) and np.array_equal(s, want_s), "re-call"
        want_l, want_s, want_off = rule.csr(maps, 1)
        l, k, s, off = ctx.canny_components(frames, 1.4, 50, 150, want_kept=True)
        _check_offsets(off, want_off, "canny_components")
        assert l.dtype == np.int32 and np.array_equal(l, want_l), "labels"
        assert k.dtype == np.uint8 and np.array_equal(k, np.where(want_l != 0, 255, 0)), "kept_u8"
        assert s.dtype == np.int32 and np.array_equal(s, want_s), "stats"
        l, k, s, off = ctx.canny_components(frames[0], 1.4, 50, 150, min_area=6, want_labels=False)
        w1 = rule.csr(maps[:1], 6)
        assert l is None and k is None and np.array_equal(s, w1[1]) and np.array_equal(off, w1[2])


def test_cli_writes_the_components_and_the_kept_map(hip, tmp_path):
    h, w = 96, 160
    frame = synth_frame(h, w, 4)
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + frame.tobytes())
    out = tmp_path / "out"
    out.mkdir()
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, "1.4", "50", "150", "-i", str(src), "-o", str(out), "-m", "4"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    edges = oracle.canny(frame, 1.4, 50, 150)
    labels, stats = rule.components(edges, 4)
    lines = (out / "canny_components.txt").read_text().splitlines()
    got = np.array([[int(t) for t in ln.split()] for ln in lines], np.int64).reshape(-1, 6)
    want = np.concatenate([np.arange(1, stats.shape[0] + 1)[:, None], stats[:, :5]], axis=1)
    assert np.array_equal(got, want)
    data = (out / "canny_kept.pgm").read_bytes()
    assert data.startswith(b"P5\n%d %d\n255\n" % (w, h))
    kept = np.frombuffer(data[-h * w:], np.uint8).reshape(h, w)
    assert np.array_equal(kept, np.where(labels != 0, 255, 0))


def test_parts_are_timed_and_the_stages_are_unaffected(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150, "timed")
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 0b1111 << 13)
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, 1, "profiled", edges=False)
        for part in range(4):
            ms, launches = ctx.components_profile_get(part)
            assert launches == 1 and ms > 0.0, hip.CC_PARTS[part]
        for stage in range(9):
            assert ctx.profile_get(stage)[1] == 0
        assert ctx.hough_profile_get(0)[1] == 0
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0)   # all stages
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, 1, "profiled, all stages", edges=False, labels=False,
                          kept=False)
        assert ctx.profile_get(hip.STAGE_GAUSSIAN)[1] == 1
        assert ctx.components_profile_get(0)[1] == 1 and ctx.components_profile_get(3)[1] == 0   # nothing to write out
