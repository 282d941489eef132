"""Binarization on the GPU (canny_hip_dev_binarize, canny_hip_binarize_batch) against
tests/binarize_rule.py, byte for byte: every output byte, count and threshold, with sentinel bytes behind each buffer, inputs
that start at odd addresses, and counts and thresholds untouched when they are not asked for.  Every adaptive case runs under
every route and the routes must agree."""
import os
import subprocess

import numpy as np
import pytest

import binarize_rule as R
import components_rule
import morph_rule as M
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
_, TILING = capi.binarize_plan(1, 64, 64, R.ADAPTIVE_MEAN, 3, 3)
STRIP = TILING.strip_cols
WIDTHS = (1, 7, 8, 9, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1)
BATCHES = (1, 3, 5)
WINDOWS = ((3, 3), (3, 255), (255, 3), (31, 31), (255, 255))
CS = (-255, -1, 0, 1, 7, 255)
THRS = (-1, 0, 127, 254, 255)
ROUTES = (capi.BIN_ROUTE_AUTO, capi.BIN_ROUTE_DIRECT, capi.BIN_ROUTE_MARCH)


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard bytes behind each, and plain uploads."""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptrs = ctx, {}, []

    def filled(self, nbytes):
        p = self.ctx.malloc(nbytes + N_GUARD)
        self.ptrs.append(p)
        self.size[p] = nbytes
        self.ctx.h2d(p, np.full(nbytes + N_GUARD, SENT, np.uint8))
        return p

    def upload(self, a, odd=False):
        """odd: the data starts one byte into the allocation."""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if odd:
            a = np.concatenate([np.full(1, 0xFF, np.uint8), a])
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.ctx.h2d(p, a)
        return p + (1 if odd else 0)

    def get(self, p, what=""):
        out = np.empty(self.size[p] + N_GUARD, np.uint8)
        self.ctx.d2h(out, p)
        assert (out[self.size[p]:] == SENT).all(), f"guard bytes overwritten behind {what}"
        return out[:self.size[p]]

    def untouched(self):
        for p in self.size:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.size, self.ptrs = {}, []


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def run(ctx, b, what, shape, d_in, want, method, thr_or_c=0, kw=3, kh=3, invert=0, route=0, with_counts=True, with_thr=True):
    """One call into fresh sentinel-filled buffers, compared with `want` = (bits, counts, thresholds); -> all the bytes."""
    n, h, w = shape
    rb = (w + 7) // 8
    d_out, d_cnt, d_thr = b.filled(n * h * rb), b.filled(n * 8), b.filled(n * 4)
    ctx.set_option("binarize_route", route)
    ctx.dev_binarize(d_in, n, h, w, method, thr_or_c, d_out, d_cnt if with_counts else 0, d_thr if with_thr else 0, kw, kh, invert)
    ctx.set_option("binarize_route", 0)
    what = f"{what}: {n} x {h} x {w} method {method} {thr_or_c} {kw}x{kh} invert {invert} route {route}"
    out, cnt, thr = b.get(d_out, what + ": out").reshape(n, h, rb), b.get(d_cnt, what + ": counts"), b.get(d_thr, what + ": thr")
    same(out, want[0], what)
    if with_counts:
        assert cnt.view(np.int64).tolist() == want[1].tolist(), what + ": counts"
    else:
        assert (cnt == SENT).all(), what + ": counts written without a buffer"
    if with_thr:
        assert thr.view(np.int32).tolist() == want[2].tolist(), what + ": thresholds"
    else:
        assert (thr == SENT).all(), what + ": thresholds written without a buffer"
    return out.tobytes() + cnt.tobytes() + thr.tobytes()


def adaptive(ctx, b, what, a, c, kw, kh, invert, k=0, odd=False, want=None):
    """ADAPTIVE_MEAN under every route against the rule; the routes must agree."""
    want = R.binarize(a, R.ADAPTIVE_MEAN, c, kw, kh, invert) if want is None else want
    d_in = b.upload(a, odd)
    runs = [run(ctx, b, what, a.shape, d_in, want, R.ADAPTIVE_MEAN, c, kw, kh, invert, r, k % 4 != 3, k % 3 != 2) for r in ROUTES]
    assert runs[0] == runs[1] == runs[2], what + ": the routes differ"


def frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    kind = seed % 3
    if kind == 0:
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if kind == 1:
        return R.unit_frames(n, h, w, seed)
    a = rng.integers(0, 256, (n, h, w)).astype(np.int64)
    a = (a + np.roll(a, 1, 1) + np.roll(a, 1, 2) + np.roll(a, -1, 2)) // 4 + rng.integers(-2, 3, (n, h, w))   # smooth: sums near v A
    return np.clip(a, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("w", WIDTHS)
def test_fixed_and_otsu_on_every_width(hip, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate((1, 2, 5, 33, 64)):
            k = 5 * WIDTHS.index(w) + i
            n, invert = BATCHES[k % 3], k & 1
            a = frames(n, h, w, k)
            d_in = b.upload(a, odd=k % 2 == 0)
            thr = THRS[k % 5]
            run(ctx, b, "fixed", a.shape, d_in, R.binarize(a, R.FIXED, thr, invert=invert), R.FIXED, thr, 0, 0, invert,
                with_counts=k % 4 != 3, with_thr=k % 3 != 2)
            run(ctx, b, "otsu", a.shape, d_in, R.binarize(a, R.OTSU, invert=1 - invert), R.OTSU, 77, 0, 0, 1 - invert,
                with_counts=k % 4 != 1, with_thr=k % 3 != 1)
            b.free()


def test_every_fixed_threshold_and_both_inversions(hip):
    a = frames(3, 9, 21, 3)
    a[0, 0, :5] = (0, 127, 128, 254, 255)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(a, odd=True)
        for thr in THRS:
            for invert in (0, 1):
                run(ctx, b, "thr", a.shape, d_in, R.binarize(a, R.FIXED, thr, invert=invert), R.FIXED, thr, invert=invert)
        want = R.binarize(a, R.FIXED, -1)
        assert want[1].tolist() == [9 * 21] * 3 and (want[0][:, :, 2] == 0xF8).all()       # every pixel, and no pad bit
        b.free()


@pytest.mark.parametrize("w", WIDTHS)
def test_adaptive_on_every_width_under_every_route(hip, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, (kw, kh) in enumerate(WINDOWS):
            k = 5 * WIDTHS.index(w) + i
            hs = (1, 2, kh - 1, kh, kh + 1)
            h = hs[k % 5] if kh < 255 or w < 100 else (1, 2, 31, 40, 66)[k % 5]       # the tall windows on wide frames: few rows
            a = frames(BATCHES[k % 3] if h * w < 20000 else 1, h, w, k)
            adaptive(ctx, b, "widths", a, CS[k % 6], kw, kh, k & 1, k, odd=k % 2 == 1)
            b.free()


@pytest.mark.parametrize("kw,kh", WINDOWS)
def test_adaptive_heights_around_the_window_and_the_segment(hip, kw, kh):
    seg = hip.binarize_plan(1, 64, 64, R.ADAPTIVE_MEAN, kw, kh)[1].segment_rows
    assert seg >= 2 * (kh - 1) and seg >= 64
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate((1, 2, kh - 1, kh, kh + 1, seg - 1, seg, seg + 1, 2 * seg + 1)):
            k = 11 * WINDOWS.index((kw, kh)) + i
            w = (9, 17, 5, 64, 33)[k % 5] if kw == 255 else (9, 70, 130, 64, 33)[k % 5]
            a = frames(BATCHES[k % 3] if h * w < 5000 else 1, h, w, k + 1)
            adaptive(ctx, b, "heights", a, CS[k % 6], kw, kh, k & 1, k, odd=k % 2 == 0)
            b.free()


def test_adaptive_frames_smaller_than_the_window_and_every_c(hip):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        k = 0
        for shape in ((2, 1, 1), (3, 5, 7)):
            a = frames(*shape, seed=4 + shape[1])
            for kw, kh in WINDOWS:
                for c in CS:
                    adaptive(ctx, b, "small", a, c, kw, kh, k & 1, k)
                    k += 1
                b.free()


def test_one_unit_of_the_window_sum_decides_bits(hip):
    """The frames of tests/test_binarize_rule.py's mutants, and wider ones across two strips and two segments."""
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for n, h, w, seed in ((3, 12, 17, 11), (2, 70, STRIP + 40, 12)):
            a = R.unit_frames(n, h, w, seed)
            want = R.binarize(a, R.ADAPTIVE_MEAN, 1, 3, 3, form=R.cond_mean)
            assert 0 < want[1].min() and want[1].max() < h * w
            adaptive(ctx, b, "unit", a, 1, 3, 3, 0, 0, want=want)
        b.free()


def otsu_frames():
    """Frames whose histograms are the designed ones of the CPU test, flat frames, and frames of different brightness."""
    h, w = 20, 32
    def of(values_counts):
        px = np.concatenate([np.full(c, v, np.uint8) for v, c in values_counts])
        assert px.size <= h * w
        px = np.concatenate([px, np.full(h * w - px.size, values_counts[0][0], np.uint8)])
        return np.random.default_rng(1).permutation(px).reshape(h, w)
    named = [("flat", of([(77, 640)]), 0), ("two values", of([(10, 320), (20, 320)]), 10),
             ("two values, uneven", of([(20, 634), (10, 6)]), 10), ("tie across a gap", of([(0, 320), (255, 320)]), 0),
             ("symmetric three", of([(100, 214), (110, 213), (120, 213)]), None), ("top bin", of([(254, 320), (255, 320)]), 254),
             ("flat 0", of([(0, 640)]), 0), ("flat 255", of([(255, 640)]), 0)]
    rng = np.random.default_rng(2)
    for base in (20, 90, 170):                                       # the same scene at three brightnesses: three thresholds
        scene = np.where(rng.random((h, w)) < 0.4, base + 60, base) + rng.integers(0, 9, (h, w))
        named.append((f"bright {base}", scene.astype(np.uint8), None))
    return named


def test_otsu_gives_every_frame_its_own_threshold(hip):
    named = otsu_frames()
    a = np.stack([f for _n, f, _t in named])
    want = R.binarize(a, R.OTSU)
    for (name, _f, t), got in zip(named, want[2].tolist()):
        assert t is None or got == t, name
    bright = want[2][-3:].tolist()
    assert bright[0] < bright[1] < bright[2] and len(set(want[2].tolist())) >= 6
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(a, odd=True)
        for invert in (0, 1):
            run(ctx, b, "otsu designed", a.shape, d_in, R.binarize(a, R.OTSU, invert=invert), R.OTSU, invert=invert)
        out, counts, thr = ctx.binarize_batch(a, R.OTSU)
        same(out, want[0], "binarize_batch")
        assert counts.tolist() == want[1].tolist() and thr.tolist() == want[2].tolist()
        b.free()


def test_otsu_where_the_score_needs_more_than_64_bits(hip):
    """One frame of 8192 x 8192, the 2^26 pixels of the limit, with two far values: d^2 is about 2^116 and the scores pass
    2^64 (a smaller frame cannot reach that: the largest score is below 255^2 N^2 / 4)."""
    h, w = 8192, 8192
    assert h * w == R.OTSU_MAX_PIXELS
    a = np.full((1, h, w), 3, np.uint8)
    a[0, ::2] = 250
    a[0, 5, :7] = (100, 101, 102, 103, 104, 105, 106)
    assert max(R.otsu_scores(R.histogram(a[0]))) >= 1 << 64
    want = R.binarize(a, R.OTSU)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        run(ctx, b, "wide scores", a.shape, b.upload(a), want, R.OTSU)
        b.free()


def test_more_work_items_than_the_grid_cap(hip):
    """16385 frames of 2 x 3: one chunk of output bytes and one (strip, segment) a frame.  4096 workgroups take one chunk, or
    four wave items, per trip: every launch goes through a second trip, as the plan query says."""
    n, h, w = 16385, 2, 3
    plan, tiling = hip.binarize_plan(n, h, w, R.ADAPTIVE_MEAN, 3, 3)
    assert tiling.direct_trips == 5 and tiling.march_trips == 2 and plan.grid == 4096
    assert hip.binarize_plan(16384, h, w, R.ADAPTIVE_MEAN, 3, 3)[1].march_trips == 1
    assert hip.binarize_plan(4096, h, w, R.FIXED)[0].trips == 1 and hip.binarize_plan(4097, h, w, R.FIXED)[0].trips == 2
    a = R.unit_frames(n, h, w, 13)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for method, c in ((R.ADAPTIVE_MEAN, 1), (R.FIXED, 100), (R.OTSU, 0)):
            want = hip.binarize(a, method, c, 3, 3)                                   # the host rule: the CPU tests pin it
            for f in (0, 1, 4095, 4096, 8191, 16383, 16384):
                ref = R.binarize(a[f:f + 1], method, c, 3, 3)
                assert all(np.array_equal(x[f:f + 1], y) for x, y in zip(want, ref))
            if method == R.ADAPTIVE_MEAN:
                adaptive(ctx, b, "past the cap", a, c, 3, 3, 0, 0, want=want)
            else:
                run(ctx, b, "past the cap", a.shape, b.upload(a), want, method, c)
            b.free()


def test_the_contexts_smoothed_plane(hip):
    """d_plane = NULL after dev_canny: the rule on the oracle's Gaussian plane, whether the context kept bytes or shorts."""
    n, h, w = 3, 72, 200
    imgs = np.stack([synth_frame(h, w, s) for s in (7, 8, 9)])
    planes = np.stack([oracle.gaussian(f, SIGMA) for f in imgs])
    assert planes.min() >= 0 and planes.max() <= 255
    planes = planes.astype(np.uint8)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges = b.upload(imgs), b.filled(n * h * w * 2)
        d_out = b.filled(n * h * 25)
        with pytest.raises(capi.CannyHipError) as ei:                  # a context that ran no canny call has no plane
            ctx.dev_binarize(0, n, h, w, R.OTSU, 0, d_out)
        assert ei.value.status == 1
        seen = set()
        for u8 in (0, 1):
            ctx.set_option("smoothed_u8", u8)
            ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
            seen.add(ctx.get_option("last_canny_smoothed_u8"))
            run(ctx, b, f"plane u8 {u8}", (n, h, w), 0, R.binarize(planes, R.OTSU), R.OTSU)
            run(ctx, b, f"plane u8 {u8}", (n, h, w), 0, R.binarize(planes, R.FIXED, 100, invert=1), R.FIXED, 100, invert=1)
            want = R.binarize(planes, R.ADAPTIVE_MEAN, 2, 15, 9)
            runs = [run(ctx, b, f"plane u8 {u8}", (n, h, w), 0, want, R.ADAPTIVE_MEAN, 2, 15, 9, route=r) for r in ROUTES]
            assert runs[0] == runs[1] == runs[2]
            run(ctx, b, f"plane u8 {u8}", (n, h, w), 0, R.binarize(planes, R.ADAPTIVE_MEAN, -3, 101, 3, 1), R.ADAPTIVE_MEAN, -3, 101,
                3, 1, route=2)
        assert seen == {0, 1}
        for n2, h2, w2 in ((2, h, w), (3, h - 1, w), (3, w, h)):      # ... nor one of another shape
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_binarize(0, n2, h2, w2, R.OTSU, 0, d_out)
            assert ei.value.status == 1
        ctx.synchronize()
        assert (b.get(d_out) == SENT).all()
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs larger calls, and every data workspace it holds is
    filled with a sentinel before each of three identical runs."""
    other = frames(5, 90, 200, 6)
    n, h, w = 3, 50, 130
    a = frames(n, h, w, 21)
    with hip.Context(0) as ctx:
        ctx.binarize_batch(other, R.OTSU)
        ctx.binarize_batch(other, R.FIXED, 9)
        b = _Bufs(ctx)
        d_in = b.upload(a)
        for method, c, kw, kh, route in ((R.OTSU, 0, 3, 3, 0), (R.FIXED, 130, 3, 3, 0), (R.ADAPTIVE_MEAN, 3, 31, 5, 2),
                                         (R.ADAPTIVE_MEAN, -2, 5, 7, 1)):
            want = R.binarize(a, method, c, kw, kh)
            runs = []
            for i in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(run(ctx, b, "dirty", a.shape, d_in, want, method, c, kw, kh, route=route, with_thr=i != 1))
            assert runs[0] == runs[2]
        assert any(name == "binarize_ws" and kind == hip.WS_DATA and nbytes for name, _p, nbytes, kind in ctx.selftest_workspaces())
        b.free()


def test_blobs_on_a_ramp_to_components_without_a_download(hip):
    """dev_binarize (adaptive mean, inverted) -> dev_morph_bits OPEN 3 x 3 -> dev_components_bits on one stream: exactly the
    blobs, as the rules say; Otsu's global threshold on the same frame cuts the ramp and does not find them."""
    frame, n_blobs = R.blobs_on_a_ramp()
    h, w = frame.shape
    rb = (w + 7) // 8
    el = M.named_elements()["rect3x3"]
    want = R.binarize(frame[None], R.ADAPTIVE_MEAN, 10, 31, 31, 1)
    want_open, want_n = M.morph(want[0], w, M.OPEN, *el)
    want_labels, want_stats, want_off = components_rule.csr(M.unpack(want_open, w), 1)
    assert len(want_stats) == n_blobs
    otsu = R.binarize(frame[None], R.OTSU, invert=1)
    otsu_open, otsu_n = M.morph(otsu[0], w, M.OPEN, *el)
    otsu_stats = components_rule.csr(M.unpack(otsu_open, w), 1)[1]
    assert len(otsu_stats) != n_blobs
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(frame, odd=True)
        for bits, opened, counts, stats, method, c in ((want, want_open, want_n, want_stats, R.ADAPTIVE_MEAN, 10),
                                                       (otsu, otsu_open, otsu_n, otsu_stats, R.OTSU, 0)):
            cap = max(len(stats), 1)
            d_bits, d_cnt, d_open, d_n = b.filled(h * rb), b.filled(8), b.filled(h * rb), b.filled(8)
            d_labels, d_stats, d_off = b.filled(h * w * 4), b.filled(cap * 6 * 4), b.filled(2 * 8)
            ctx.dev_binarize(d_in, 1, h, w, method, c, d_bits, d_cnt, 0, 31, 31, 1)
            ctx.dev_morph_bits(d_bits, 1, h, w, M.OPEN, *el, d_open, d_n)
            ctx.dev_components_bits(d_open, h, w, 1, 1, d_labels, 0, d_stats, cap, d_off)
            same(b.get(d_bits, "bits").reshape(1, h, rb), bits[0], "bits")
            assert b.get(d_cnt, "counts").view(np.int64).tolist() == bits[1].tolist()
            same(b.get(d_open, "opened").reshape(1, h, rb), opened, "opened")
            assert b.get(d_n, "opened counts").view(np.int64).tolist() == counts.tolist()
            assert b.get(d_off, "offsets").view(np.uint64).tolist() == [0, len(stats)]
            if len(stats):
                same(b.get(d_stats, "stats").view(np.int32).reshape(cap, 6), stats, "stats")
            b.free()
            d_in = b.upload(frame, odd=True)
        b.free()


def test_profile_part_counts_the_launches_of_its_own_parts(hip):
    a = frames(2, 40, 70, 8)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        parts = lambda: [ctx.profile_part("binarize", p)[1] for p in range(3)]
        ctx.set_option("profile_stage_mask", 1)                              # the first canny stage alone: bit 30 is off
        ctx.profile_reset()
        ctx.binarize_batch(a, R.OTSU)
        assert parts() == [0, 0, 0]
        ctx.set_option("profile_stage_mask", 1 << 30)                        # every part behind the polygons
        ctx.binarize_batch(a, R.OTSU)
        assert parts() == [1, 1, 1]
        ctx.set_option("profile_stage_mask", 0)                              # all slots
        ctx.profile_reset()
        assert parts() == [0, 0, 0]
        ctx.binarize_batch(a, R.FIXED, 100)
        assert parts() == [0, 0, 1]
        ctx.binarize_batch(a, R.ADAPTIVE_MEAN, 1, 5, 5)
        assert parts() == [0, 0, 2]
        ctx.binarize_batch(a, R.OTSU)
        assert parts() == [1, 1, 3]
        assert all(ctx.profile_part("binarize", p)[0] > 0 for p in range(3))
        assert ctx.profile_part("morph", 0)[1] == 0 and ctx.profile_part("components", 0)[1] == 0
        # ... and agrees with the named getters of two existing groups
        ctx.canny_morph(a, SIGMA, LO, HI, M.DILATE, *M.named_elements()["rect3x3"])
        ctx.canny_components(a, SIGMA, LO, HI)
        assert ctx.profile_part("morph", 0) == ctx.morph_profile(0) and ctx.morph_profile(0)[1] == 1
        for p in range(len(hip.CC_PARTS)):
            assert ctx.profile_part("components", p) == ctx.components_profile_get(p)
        assert sum(ctx.components_profile_get(p)[1] for p in range(len(hip.CC_PARTS))) > 0
        assert parts() == [1, 1, 3]
        for feature, part in (("binarize", 3), ("binarize", -1), ("nonesuch", 0), ("", 0), ("morph", 1)):
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.profile_part(feature, part)
            assert ei.value.status == 1


def test_the_refused_calls(hip):
    n, h, w, rb = 2, 20, 30, 4
    a = frames(n, h, w, 40)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(a)
        d_out, d_cnt, d_thr = b.filled(n * h * rb), b.filled(n * 8 + 8), b.filled(n * 4 + 4)
        good = dict(src=d_in, n=n, h=h, w=w, method=R.ADAPTIVE_MEAN, c=1, out=d_out, cnt=d_cnt, thr=d_thr, kw=3, kh=3, invert=0)

        def call(**kw):
            k = dict(good, **kw)
            try:
                ctx.dev_binarize(k["src"], k["n"], k["h"], k["w"], k["method"], k["c"], k["out"], k["cnt"], k["thr"], k["kw"],
                                 k["kh"], k["invert"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(method=-1), dict(method=3), dict(invert=2),
                   dict(invert=-1), dict(kw=1), dict(kh=1), dict(kw=4), dict(kh=6), dict(kw=257), dict(kh=257), dict(c=256),
                   dict(c=-256), dict(method=R.FIXED, c=-2), dict(method=R.FIXED, c=256), dict(cnt=d_cnt + 4), dict(thr=d_thr + 2),
                   dict(out=d_in), dict(out=d_in + n * h * w - 1), dict(cnt=d_in), dict(thr=d_in + 8), dict(cnt=d_out + 8),
                   dict(thr=d_out + 4), dict(thr=d_cnt + 4), dict(src=0)):
            assert call(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2), dict(method=R.OTSU, h=8193, w=8192)):
            assert call(**kw) == 2, kw
        for value in (3, -1):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option("binarize_route", value)
        ctx.synchronize()
        b.untouched()
        assert call() == 0 and call(cnt=0, thr=0) == 0 and call(method=R.OTSU, kw=0, kh=-5, c=999) == 0
        ctx.set_option("binarize_route", 2)
        assert ctx.get_option("binarize_route") == 2
        b.get(d_out), b.get(d_cnt), b.get(d_thr)
        b.free()


def test_cli_writes_the_binary_image(hip, fixture_image, tmp_path):
    """Main ... -a: the frame itself binarized into canny_binary.pgm, and Otsu's threshold on stdout."""
    h, w = fixture_image.shape
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + fixture_image.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canny_edge_amd", "Main")
    for value, args in (("otsu", (R.OTSU, 0, 3, 3, 0)), ("otsu,0,0,0,1", (R.OTSU, 0, 3, 3, 1)), ("fixed", (R.FIXED, 127, 3, 3, 0)),
                        ("fixed,-1", (R.FIXED, -1, 3, 3, 0)), ("mean", (R.ADAPTIVE_MEAN, 7, 31, 31, 0)),
                        ("mean,-3,5", (R.ADAPTIVE_MEAN, -3, 5, 5, 0)), ("mean,2,101,3,1", (R.ADAPTIVE_MEAN, 2, 101, 3, 1))):
        out = tmp_path / ("out_" + value.replace(",", "_"))
        out.mkdir()
        r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(out), "-a", value], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        bits, counts, thr = R.binarize(fixture_image[None], *args)
        data = (out / "canny_binary.pgm").read_bytes()
        assert data.startswith(b"P5\n%d %d\n255\n" % (w, h))
        got = np.frombuffer(data[-h * w:], np.uint8).reshape(h, w)
        assert np.array_equal(got, np.where(R.unpack(bits, w)[0], 255, 0)), value
        assert ("otsu threshold %d\n" % thr[0] in r.stdout) == (args[0] == R.OTSU), (value, r.stdout)
    usage = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "-a method" in usage.stderr and "canny_binary.pgm" in usage.stderr
