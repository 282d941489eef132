"""Binary morphology on the GPU (canny_hip_dev_morph_bits, canny_hip_dev_canny_morph, canny_hip_canny_morph; DESIGN.md section
34) against tests/morph_rule.py, byte for byte: every output byte and count, with sentinel bytes behind each buffer, and the
counts untouched when they are not asked for."""
import numpy as np
import pytest

import components_rule
import contours_rule
import fuse_rule as fr
import morph_rule as R
import oracle
import warp_rule as wr
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
WIDTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 257)
HEIGHTS = (1, 2, 15, 16, 17, 33, 65)
BATCHES = (1, 3, 5)
ITERATIONS = (1, 2, 5)
ROUTES = (capi.MORPH_ROUTE_AUTO, capi.MORPH_ROUTE_GENERAL, capi.MORPH_ROUTE_SEPARABLE)
ELEMENTS = R.named_elements()
NAMES = tuple(ELEMENTS)
PATTERNS = tuple(R.named_patterns(1, 2, 2))


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
        if a.nbytes:
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


def check_output(b, what, d_out, d_cnt, shape, want, want_counts, with_counts):
    out = b.get(d_out, what + ": out").reshape(shape)
    cnt = b.get(d_cnt, what + ": counts")
    same(out, want, what)
    if with_counts:
        assert cnt.view(np.int64).tolist() == want_counts.tolist(), what + ": counts"
    else:
        assert (cnt == SENT).all(), what + ": counts written without a buffer"
    return out.tobytes() + cnt.tobytes()


def morph_and_check(ctx, b, what, bits, w, op, el, border, iterations, route=0, with_counts=True, odd=False, d_in=None,
                    want=None):
    n, h, rb = bits.shape
    rows, kw, kh = el
    want, want_counts = want if want is not None else R.morph(bits, w, op, rows, kw, kh, border, iterations)
    d_in = b.upload(bits, odd) if d_in is None else d_in
    d_out, d_cnt = b.filled(n * h * rb), b.filled(n * 8)
    ctx.set_option("morph_route", route)
    ctx.dev_morph_bits(d_in, n, h, w, op, rows, kw, kh, d_out, d_cnt if with_counts else 0, border, iterations)
    ctx.set_option("morph_route", 0)
    return check_output(b, f"{what} route {route}", d_out, d_cnt, (n, h, rb), want, want_counts, with_counts)


def case(ctx, b, k, n, h, w, name, op, border, iterations, pattern=None, dirty=True, odd=False):
    """One case of the thinned product; a rectangle runs under every route, any other element under the route k picks."""
    pattern = PATTERNS[k % len(PATTERNS)] if pattern is None else pattern
    px = R.named_patterns(n, h, w, k)[pattern]
    bits = R.pack_dirty(px, np.random.default_rng(k) if k % 2 else None) if dirty else R.pack(px)
    el = ELEMENTS[name]
    what = f"{n} x {h} x {w} {name} op {op} border {border} x{iterations} {pattern}"
    want = R.morph(bits, w, op, *el, border, iterations)
    d_in = b.upload(bits, odd)
    routes = ROUTES if name in R.RECT_NAMES else (ROUTES[k % 3],)
    runs = [morph_and_check(ctx, b, what, bits, w, op, el, border, iterations, r, k % 4 != 3, d_in=d_in, want=want)
            for r in routes]
    assert all(r == runs[0] for r in runs), what + ": the routes differ"


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_with_every_height_and_border(hip, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate(HEIGHTS):
            for border in R.BORDERS:
                k = 3 * (7 * WIDTHS.index(w) + i) + border
                case(ctx, b, k, BATCHES[k % 3], h, w, NAMES[k % len(NAMES)], R.OPS[k % 7], border, ITERATIONS[(k // 2) % 3],
                     odd=k % 5 == 0)
            b.free()


@pytest.mark.parametrize("name", NAMES)
def test_every_element_with_every_op_and_border(hip, name):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for op in R.OPS:
            for border in R.BORDERS:
                k = 3 * (7 * NAMES.index(name) + op) + border + 1000
                case(ctx, b, k, BATCHES[k % 3], HEIGHTS[(k // 3) % 7], WIDTHS[k % 13], name, op, border, ITERATIONS[k % 3])
            b.free()


@pytest.mark.parametrize("op", R.OPS)
def test_every_op_with_every_border_and_iteration_count(hip, op):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for border in R.BORDERS:
            for j, iterations in enumerate(ITERATIONS):
                k = 9 * op + 3 * border + j + 2000
                case(ctx, b, k, 2, 33, 65, ("rect3x3", "cross5x5", "L", "ring3x3", "rect5x3")[k % 5], op, border, iterations,
                     pattern="random0.50")
        b.free()


def test_sixteen_iterations(hip):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for k, (op, name) in enumerate(((R.DILATE, "rect3x3"), (R.CLOSE, "L"), (R.GRADIENT, "ring3x3"))):
            case(ctx, b, 3000 + k, 2, 33, 65, name, op, R.BORDER_NEUTRAL, 16, pattern="random0.05")
        b.free()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_pattern(hip, pattern):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for j, name in enumerate(("rect3x3", "rect31x31", "ellipse7x7", "far_bit", "alternating31", "random31_1")):
            for border in R.BORDERS:
                k = 3 * (6 * PATTERNS.index(pattern) + j) + border + 4000
                case(ctx, b, k, 3, (17, 65)[k % 2], (33, 129, 257)[k % 3], name, R.OPS[k % 7], border, 1 + k % 2,
                     pattern=pattern, dirty=k % 3 != 0)
        b.free()


def test_nothing_crosses_a_frame_boundary(hip):
    """A frame of ones between frames of zeros, DILATE 31 x 31 with BORDER_ZERO: the frames are adjacent in memory."""
    for h, w in ((7, 40), (65, 129)):
        px = np.zeros((3, h, w), bool)
        px[1] = True
        with hip.Context(0) as ctx:
            b = _Bufs(ctx)
            for r in ROUTES:
                out = morph_and_check(ctx, b, "frames", R.pack(px), w, R.DILATE, ELEMENTS["rect31x31"], R.BORDER_ZERO, 1, r)
                got = R.unpack(np.frombuffer(out, np.uint8)[:3 * h * ((w + 7) // 8)].reshape(3, h, -1), w)
                assert not got[0].any() and got[1].all() and not got[2].any()
            b.free()


def _canny_bits(frames):
    return R.pack(np.stack([oracle.canny(f, SIGMA, LO, HI) != 0 for f in frames]))


@pytest.mark.parametrize("n,h,w", [(3, 37, 77), (2, 130, 264)])
def test_dev_canny_morph_behind_dev_canny(hip, n, h, w):
    frames = np.stack([synth_frame(h, w, 11 + s) for s in range(n)])
    rb = (w + 7) // 8
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges, d_bits = b.upload(frames), b.filled(n * h * w * 2), b.filled(n * h * rb)
        ctx.dev_canny_bits(d_img, SIGMA, LO, HI, h, w, n, d_bits)
        bits = b.get(d_bits, "the map").reshape(n, h, rb)
        same(bits, _canny_bits(frames), "dev_canny_bits against the oracle")
        ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
        assert bits.any()
        for k, (op, name, border, it) in enumerate(((R.CLOSE, "rect3x3", R.BORDER_NEUTRAL, 1), (R.TOPHAT, "cross5x5", R.BORDER_ZERO, 2),
                                                    (R.BLACKHAT, "ellipse7x7", R.BORDER_ONE, 1), (R.GRADIENT, "L", R.BORDER_NEUTRAL, 3),
                                                    (R.ERODE, "rect3x5", R.BORDER_ONE, 1), (R.DILATE, "rect31x31", R.BORDER_ZERO, 1))):
            rows, kw, kh = ELEMENTS[name]
            want, want_counts = R.morph(bits, w, op, rows, kw, kh, border, it)
            runs = []
            for rep in range(2):
                d_out, d_cnt = b.filled(n * h * rb), b.filled(n * 8)
                ctx.dev_canny_morph(n, h, w, op, rows, kw, kh, d_out, d_cnt, border, it)
                runs.append(check_output(b, f"canny_morph {name} op {op}", d_out, d_cnt, (n, h, rb), want, want_counts, True))
                if rep == 0:   # another analysis call of the map in between
                    d_off = b.filled((n + 1) * 8)
                    ctx.dev_points_from_bits(d_bits, h, w, n, 0, 0, d_off)
                    morph_and_check(ctx, b, "in between", bits, w, R.OPEN, ELEMENTS["rect3x3"], R.BORDER_NEUTRAL, 2)
            assert runs[0] == runs[1]
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_morph(n, h + 1, w, R.ERODE, [1], 1, 1, d_bits)
        b.free()
    with hip.Context(0) as ctx:   # no canny call yet
        b = _Bufs(ctx)
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_morph(n, h, w, R.ERODE, [1], 1, 1, b.filled(n * h * rb))
        b.untouched()
        b.free()


def test_canny_morph_on_host_frames(hip):
    frames = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    bits = _canny_bits(frames)
    with hip.Context(0) as ctx:
        for op, name, border, it in ((R.CLOSE, "rect3x3", R.BORDER_NEUTRAL, 1), (R.GRADIENT, "ellipse7x7", R.BORDER_ZERO, 2)):
            rows, kw, kh = ELEMENTS[name]
            want, want_counts = R.morph(bits, 200, op, rows, kw, kh, border, it)
            out, counts = ctx.canny_morph(frames, SIGMA, LO, HI, op, rows, kw, kh, border, it)
            same(out, want, f"canny_morph op {op}")
            assert counts.tolist() == want_counts.tolist() and counts.sum() > 0
        out, counts = ctx.canny_morph(frames, SIGMA, LO, 300, R.DILATE, *ELEMENTS["rect3x3"])   # max_val > 255: an empty map
        assert not out.any() and not counts.any()


def test_the_change_mask_chain_on_one_stream(hip):
    """dev_warp_frames -> dev_fuse_frames -> dev_change_mask -> dev_morph_bits OPEN 3 x 3 -> dev_components_bits with nothing
    downloaded in between, against the host rules chained."""
    bg, frames, patch = fr.moving_object()
    h, w = bg.shape
    rng = np.random.default_rng(5)
    frames = frames.copy()
    for f in range(3):   # salt: single pixels raised above the threshold, away from the patch
        ys, xs = rng.integers(0, h, 12), rng.integers(0, w, 12)
        for y, x in zip(ys, xs):
            if not patch[:, max(y - 4, 0):y + 5, max(x - 4, 0):x + 5].any():
                frames[f, y, x] = min(int(frames[f, y, x]) + 50, 255)
    recs = np.stack([wr.record(wr.shift(0, 0), k) for k in range(3)])
    want_frames, want_bits = wr.warp(frames, recs, h, w, wr.NEAREST, 0)
    want_bg, want_count = fr.fuse(want_frames, want_bits, 3, 3, fr.MEDIAN, 0, 2)
    want_mask, _ = fr.change_mask(want_frames, want_bits, want_bg, want_count, 3, 49, 2)
    el = ELEMENTS["rect3x3"]
    want_open, want_counts = R.morph(want_mask, w, R.OPEN, *el)
    assert want_mask.sum() != want_open.sum() and (R.unpack(want_open, w) == patch).all()
    want_labels, want_stats, want_off = components_rule.csr(R.unpack(want_open, w), 1)
    rb, cap = (w + 7) // 8, len(want_stats)
    assert cap == 3 and want_counts.tolist() == [54, 54, 54]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_src, d_x = b.upload(frames), b.upload(recs)
        d_al, d_valid = b.filled(3 * h * w), b.filled(3 * h * rb)
        d_bg, d_cnt, d_mask, d_changed = b.filled(h * w), b.filled(h * w), b.filled(3 * h * rb), b.filled(3 * 8)
        d_open, d_n = b.filled(3 * h * rb), b.filled(3 * 8)
        d_labels, d_stats, d_off = b.filled(3 * h * w * 4), b.filled(cap * 6 * 4), b.filled(4 * 8)
        ctx.dev_warp_frames(d_src, 3, h, w, d_x, 3, h, w, d_al, d_valid, wr.NEAREST, 0)
        ctx.dev_fuse_frames(d_al, d_valid, 3, h, w, 3, 3, d_bg, d_cnt, fr.MEDIAN, 0, 2)
        ctx.dev_change_mask(d_al, d_valid, 3, h, w, d_bg, d_cnt, 3, d_mask, d_changed, 49, 2)
        ctx.dev_morph_bits(d_mask, 3, h, w, R.OPEN, *el, d_open, d_n)
        ctx.dev_components_bits(d_open, h, w, 3, 1, d_labels, 0, d_stats, cap, d_off)
        same(b.get(d_mask, "the masks").reshape(3, h, rb), want_mask, "mask")
        same(b.get(d_open, "the opened masks").reshape(3, h, rb), want_open, "opened")
        assert b.get(d_n, "counts").view(np.int64).tolist() == [54, 54, 54]
        assert b.get(d_off, "offsets").view(np.uint64).tolist() == want_off.tolist()
        same(b.get(d_stats, "stats").view(np.int32).reshape(cap, 6), want_stats, "stats")
        same(b.get(d_labels, "labels").view(np.int32).reshape(3, h, w), want_labels, "labels")
        b.free()


def test_the_edge_map_chain_on_one_stream(hip):
    """dev_canny -> dev_canny_morph CLOSE 3 x 3 -> dev_contours_bits against the oracle's map and the host rules chained."""
    n, h, w = 2, 90, 200
    frames = np.stack([synth_frame(h, w, s) for s in (7, 8)])
    el = ELEMENTS["rect3x3"]
    want_closed, _ = R.morph(_canny_bits(frames), w, R.CLOSE, *el)
    stats, off, chain_off, points, point_off = contours_rule.csr(R.unpack(want_closed, w), 1)
    rb, cap, pcap = (w + 7) // 8, len(stats), len(points)
    assert cap > 0
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges, d_closed = b.upload(frames), b.filled(n * h * w * 2), b.filled(n * h * rb)
        d_stats, d_off, d_chain = b.filled(cap * 6 * 4), b.filled((n + 1) * 8), b.filled((cap + 1) * 8)
        d_points, d_poff = b.filled(pcap * 4), b.filled((n + 1) * 8)
        ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
        ctx.dev_canny_morph(n, h, w, R.CLOSE, *el, d_closed)
        ctx.dev_contours_bits(d_closed, h, w, n, 1, d_stats, cap, d_off, d_chain, d_points, pcap, d_poff)
        same(b.get(d_closed, "closed").reshape(n, h, rb), want_closed, "closed")
        same(b.get(d_stats, "stats").view(np.int32).reshape(cap, 6), stats, "stats")
        assert b.get(d_points, "points").view(np.int32).tolist() == points.tolist()
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 1 x 64 frame and 4096 workgroups at most: 4097 frames send workgroup 0 through a second trip, as the plan
    query says."""
    assert hip.morph_plan(4096, 1, 64).trips == 1
    plan = hip.morph_plan(4097, 1, 64)
    assert (plan.units, plan.grid, plan.per_group, plan.trips) == (4097, 4096, 1, 2)
    px = np.random.default_rng(9).random((4097, 1, 64)) < 0.5
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for r in ROUTES:
            morph_and_check(ctx, b, "4097 frames", R.pack(px), 64, R.DILATE, ELEMENTS["rect3x3"], R.BORDER_ZERO, 1, r)
        morph_and_check(ctx, b, "4097 frames", R.pack(px), 64, R.TOPHAT, ELEMENTS["alternating31"], R.BORDER_NEUTRAL, 2)
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs a larger call, and every data workspace it holds is
    filled with a sentinel before each of three identical runs."""
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    n, h, w = 3, 50, 130
    bits = R.pack_dirty(R.named_patterns(n, h, w, 21)["random0.50"])
    with hip.Context(0) as ctx:
        ctx.canny_morph(other, SIGMA, LO, HI, R.GRADIENT, *ELEMENTS["rect3x3"], iterations=3)
        b = _Bufs(ctx)
        d_in = b.upload(bits)
        for op, name, it, route in ((R.OPEN, "rect3x3", 2, 0), (R.GRADIENT, "ellipse7x7", 3, 0), (R.BLACKHAT, "rect5x3", 2, 2),
                                    (R.ERODE, "L", 5, 1)):
            want = R.morph(bits, w, op, *ELEMENTS[name], R.BORDER_NEUTRAL, it)
            runs = []
            for _ in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(morph_and_check(ctx, b, "dirty", bits, w, op, ELEMENTS[name], R.BORDER_NEUTRAL, it, route, d_in=d_in,
                                            want=want))
            assert runs[0] == runs[1] == runs[2]
        assert any(name == "morph_ws" and kind == hip.WS_DATA and nbytes for name, _p, nbytes, kind in ctx.selftest_workspaces())
        b.free()


def test_the_refused_calls(hip):
    n, h, w = 2, 20, 30
    rb = 4
    bits = R.pack(R.named_patterns(n, h, w, 40)["random0.50"])
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(bits)
        d_out, d_cnt = b.filled(n * h * rb), b.filled(n * 8 + 8)
        good = dict(bits=d_in, n=n, h=h, w=w, op=R.OPEN, rows=[7, 7, 7], kw=3, kh=3, out=d_out, cnt=d_cnt, border=2, it=1)

        def morph(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_morph_bits(a["bits"], a["n"], a["h"], a["w"], a["op"], a["rows"], a["kw"], a["kh"], a["out"], a["cnt"],
                                   a["border"], a["it"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(bits=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(op=-1), dict(op=7),
                   dict(border=-1), dict(border=3), dict(it=0), dict(it=17), dict(rows=[7, 15, 7]), dict(rows=[0, 0, 0]),
                   dict(kw=2, rows=[3, 3, 3]), dict(kh=2, rows=[7, 7]), dict(kw=33, rows=[7, 7, 7]), dict(kh=33, rows=[1] * 33),
                   dict(kw=0), dict(kw=-1), dict(out=d_in), dict(out=d_in + n * h * rb - 1), dict(cnt=d_cnt + 4), dict(cnt=d_in),
                   dict(cnt=d_out + 8)):
            assert morph(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
            assert morph(**kw) == 2, kw
        for kw in (dict(op=7), dict(it=0), dict(rows=[7, 15, 7]), dict(border=3)):
            a = dict(good, **kw)
            with pytest.raises(capi.CannyHipError):
                ctx.dev_canny_morph(a["n"], a["h"], a["w"], a["op"], a["rows"], a["kw"], a["kh"], a["out"], a["cnt"], a["border"],
                                    a["it"])
        for value in (3, -1):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option("morph_route", value)
        ctx.synchronize()
        b.untouched()
        assert morph() == 0 and morph(cnt=0) == 0 and morph(it=16, op=R.GRADIENT) == 0
        ctx.set_option("morph_route", 2)
        assert ctx.get_option("morph_route") == 2
        b.get(d_out), b.get(d_cnt)
        b.free()
