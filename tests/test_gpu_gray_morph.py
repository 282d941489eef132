"""Grey-level morphology and median filtering on the GPU (canny_hip_dev_gray_morph, canny_hip_gray_morph_batch; DESIGN.md
section 39) against tests/gray_morph_rule.py, byte for byte: every output byte, with sentinel bytes in front of and behind each
output, under every route."""
import numpy as np
import pytest

import binarize_rule as B
import components_rule
import gray_morph_rule as R
import morph_rule as M
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 127, 128, 129, 131, 257)   # word ends, the tile edge - 1, + 1 and + 3
HEIGHTS = (1, 2, 3, 15, 17, 31, 32, 33, 65)
BATCHES = (1, 3, 5)
ITERATIONS = (1, 2, 5)
ROUTES = (capi.GRAY_ROUTE_AUTO, capi.GRAY_ROUTE_GENERAL, capi.GRAY_ROUTE_FAST)
ELEMENTS = R.named_elements()
NAMES = tuple(ELEMENTS)
BORDER_CASES = ((R.BORDER_NEUTRAL, 0), (R.BORDER_REPLICATE, 0), (R.BORDER_CONSTANT, 0), (R.BORDER_CONSTANT, 255),
                (R.BORDER_CONSTANT, 77))
MEDIAN_BORDERS = tuple(b for b in BORDER_CASES if b[0] != R.BORDER_NEUTRAL)


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard bytes around each, and plain uploads."""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptrs = ctx, {}, []

    def filled(self, nbytes, odd=False):
        """odd: the data starts one byte into the allocation."""
        off = 1 if odd else 0
        p = self.ctx.malloc(off + nbytes + N_GUARD)
        self.ptrs.append(p)
        self.size[p + off] = (nbytes, off)
        self.ctx.h2d(p, np.full(off + nbytes + N_GUARD, SENT, np.uint8))
        return p + off

    def upload(self, a, odd=False):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if odd:
            a = np.concatenate([np.full(1, 0xFF, np.uint8), a])
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.ctx.h2d(p, a)
        return p + (1 if odd else 0)

    def get(self, p, what=""):
        nbytes, off = self.size[p]
        out = np.empty(off + nbytes + N_GUARD, np.uint8)
        self.ctx.d2h(out, p - off)
        assert (out[:off] == SENT).all() and (out[off + nbytes:] == SENT).all(), f"guard bytes overwritten around {what}"
        return out[off:off + nbytes]

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


def run(ctx, b, what, shape, d_in, want, op, el, border, iterations=1, route=0, odd=False):
    """One device call into a sentinel-filled output, compared with `want`; -> the output's bytes."""
    n, h, w = shape
    rows, kw, kh = el
    d_out = b.filled(n * h * w, odd)
    ctx.set_option("gray_morph_route", route)
    ctx.dev_gray_morph(d_in, n, h, w, op, rows, kw, kh, d_out, border[0], border[1], iterations)
    ctx.set_option("gray_morph_route", 0)
    out = b.get(d_out, what).reshape(shape)
    same(out, want, f"{what} route {route}")
    return out.tobytes()


def case(ctx, b, k, n, h, w, name, op, border, iterations, plane=None, odd=False):
    """One case of the thinned product; a rectangle and the median run under every route, any other element under the route k
    picks."""
    if op == R.MEDIAN:
        name = R.MEDIAN_NAMES[k % 2]
        border = border if border[0] != R.BORDER_NEUTRAL else MEDIAN_BORDERS[k % len(MEDIAN_BORDERS)]
    plane = R.PLANE_NAMES[k % len(R.PLANE_NAMES)] if plane is None else plane
    px = R.named_planes(n, h, w, k)[plane]
    el = ELEMENTS[name]
    what = f"{n} x {h} x {w} {name} op {op} border {border} x{iterations} {plane}"
    want = R.gray_morph(px, op, *el, *border, iterations)
    d_in = b.upload(px, odd)
    routes = ROUTES if name in R.RECT_NAMES else (ROUTES[k % 3],)
    runs = [run(ctx, b, what, px.shape, d_in, want, op, el, border, iterations, r, odd) for r in routes]
    assert all(r == runs[0] for r in runs), what + ": the routes differ"


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_with_every_height(hip, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate(HEIGHTS):
            k = 9 * WIDTHS.index(w) + i
            case(ctx, b, k, BATCHES[k % 3], h, w, NAMES[k % len(NAMES)], R.OPS[k % 8], BORDER_CASES[k % 5], ITERATIONS[(k // 2) % 3],
                 odd=k % 3 == 0)
            b.free()


@pytest.mark.parametrize("name", NAMES)
def test_every_element_with_every_op_and_border(hip, name):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for op in R.MORPH_OPS:
            for j, border in enumerate(BORDER_CASES):
                k = 5 * (7 * NAMES.index(name) + op) + j + 1000
                case(ctx, b, k, BATCHES[k % 3], HEIGHTS[(k // 3) % 9], WIDTHS[k % 15], name, op, border, ITERATIONS[k % 3],
                     odd=k % 3 == 0)
            b.free()


@pytest.mark.parametrize("op", R.OPS)
def test_every_op_with_every_border_route_and_iteration_count(hip, op):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for j, border in enumerate(BORDER_CASES):
            for i, iterations in enumerate((1, 2, 5, 16)):
                k = 20 * op + 4 * j + i + 2000
                name = ("rect3x3", "cross5x5", "L", "rect5x5", "rect5x3")[k % 5]
                n, h, w = 2, 33, 131
                px = R.named_planes(n, h, w, k)[("random", "few_valued")[k % 2]]
                if op == R.MEDIAN:
                    name, border = R.MEDIAN_NAMES[k % 2], (border if border[0] else MEDIAN_BORDERS[k % 4])
                want = R.gray_morph(px, op, *ELEMENTS[name], *border, iterations)
                d_in = b.upload(px, k % 3 == 0)
                runs = [run(ctx, b, f"{name} op {op} border {border} x{iterations}", px.shape, d_in, want, op, ELEMENTS[name], border,
                            iterations, r, k % 3 == 0) for r in ROUTES]
                assert runs[0] == runs[1] == runs[2]
            b.free()


@pytest.mark.parametrize("plane", R.PLANE_NAMES)
def test_every_named_plane(hip, plane):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for j, name in enumerate(("rect3x3", "rect31x31", "ellipse7x7", "far_bit", "rect5x5", "random31_1", "rect15x15")):
            for i, border in enumerate(BORDER_CASES):
                k = 5 * (7 * R.PLANE_NAMES.index(plane) + j) + i + 4000
                case(ctx, b, k, 3, (17, 65)[k % 2], (33, 129, 257)[k % 3], name, R.OPS[k % 7], border, 1 + k % 2, plane=plane)
                if name in R.MEDIAN_NAMES:
                    case(ctx, b, k, 2, 33, 129, name, R.MEDIAN, border, 1 + k % 2, plane=plane)
            b.free()


def test_the_median_under_every_route_on_every_width(hip):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, w in enumerate(WIDTHS):
            for j, name in enumerate(R.MEDIAN_NAMES):
                k = 2 * i + j + 5000
                case(ctx, b, k, BATCHES[k % 3], HEIGHTS[k % 9], w, name, R.MEDIAN, MEDIAN_BORDERS[k % 4], 1 + k % 2,
                     plane=("random", "few_valued", "checker")[k % 3], odd=k % 3 == 0)
            b.free()


def test_an_impulse_dilated_by_an_asymmetric_element_shows_the_reflection(hip):
    rows, kw, kh = ELEMENTS["L"]
    fp = M.element_array(rows, kw, kh)
    px = np.full((1, 40, 140), 3, np.uint8)
    px[0, 20, 126] = 250                                             # the pasted element crosses the tile edge at column 128
    want = np.full_like(px, 3)                                       # the L does not hold its centre
    want[0, 18:23, 124:129][fp] = 250
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        run(ctx, b, "impulse", px.shape, b.upload(px), want, R.DILATE, ELEMENTS["L"], (R.BORDER_REPLICATE, 0))
        b.free()


def test_nothing_crosses_a_frame_boundary(hip):
    """An all-255 frame between all-0 frames: the frames are adjacent in memory."""
    for h, w in ((7, 40), (65, 129)):
        px = np.zeros((3, h, w), np.uint8)
        px[1] = 255
        with hip.Context(0) as ctx:
            b = _Bufs(ctx)
            d_in = b.upload(px)
            for r in ROUTES:
                for op, border in ((R.DILATE, (R.BORDER_CONSTANT, 0)), (R.ERODE, (R.BORDER_CONSTANT, 255)), (R.DILATE, (R.BORDER_REPLICATE, 0)),
                                   (R.ERODE, (R.BORDER_NEUTRAL, 0))):
                    run(ctx, b, "frames", px.shape, d_in, px, op, ELEMENTS["rect31x31"], border, 1, r)
                run(ctx, b, "frames", px.shape, d_in, px, R.MEDIAN, ELEMENTS["rect5x5"], (R.BORDER_REPLICATE, 0), 2, r)
            b.free()


@pytest.mark.parametrize("n,h,w,kept", [(3, 37, 77, {0}), (2, 72, 200, {0, 1})])
def test_the_contexts_smoothed_plane(hip, n, h, w, kept):
    """d_plane = NULL after dev_canny: the rule on the oracle's Gaussian plane, whether the context kept bytes or shorts (at
    37 x 77 it keeps shorts under both settings of "smoothed_u8": the shape does not permit bytes)."""
    imgs = np.stack([synth_frame(h, w, 11 + s) for s in range(n)])
    planes = np.stack([oracle.gaussian(f, SIGMA) for f in imgs])
    assert planes.min() >= 0 and planes.max() <= 255
    planes = planes.astype(np.uint8)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges = b.upload(imgs), b.filled(n * h * w * 2)
        d_none = b.filled(n * h * w)
        with pytest.raises(capi.CannyHipError) as ei:                  # a context that ran no canny call has no plane
            ctx.dev_gray_morph(0, n, h, w, R.ERODE, *ELEMENTS["rect3x3"], d_none)
        assert ei.value.status == 1
        seen = set()
        for u8 in (0, 1):
            ctx.set_option("smoothed_u8", u8)
            ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
            seen.add(ctx.get_option("last_canny_smoothed_u8"))
            for op, name, border, it in ((R.BLACKHAT, "rect5x5", (R.BORDER_REPLICATE, 0), 1), (R.TOPHAT, "ellipse7x7", (R.BORDER_NEUTRAL, 0), 2),
                                         (R.GRADIENT, "rect3x3", (R.BORDER_CONSTANT, 9), 1), (R.MEDIAN, "rect5x5", (R.BORDER_REPLICATE, 0), 1),
                                         (R.ERODE, "L", (R.BORDER_NEUTRAL, 0), 1)):
                want = R.gray_morph(planes, op, *ELEMENTS[name], *border, it)
                runs = [run(ctx, b, f"plane u8 {u8} op {op}", planes.shape, 0, want, op, ELEMENTS[name], border, it, r) for r in ROUTES]
                assert runs[0] == runs[1] == runs[2]
        assert seen == kept
        for n2, h2, w2 in ((n - 1, h, w), (n, h - 1, w), (n, w, h)):   # ... nor one of another shape
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_gray_morph(0, n2, h2, w2, R.ERODE, *ELEMENTS["rect3x3"], d_none)
            assert ei.value.status == 1
        ctx.synchronize()
        assert (b.get(d_none) == SENT).all()
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs calls of another geometry and of the binary
    morphology, and every data workspace it holds is filled with a sentinel before each of three identical runs."""
    other = R.named_planes(3, 90, 200, 6)["random"]
    n, h, w = 3, 50, 130
    px = R.named_planes(n, h, w, 21)["random"]
    with hip.Context(0) as ctx:
        ctx.gray_morph_batch(other, R.GRADIENT, *ELEMENTS["rect5x3"], iterations=3)
        ctx.canny_morph(other, SIGMA, LO, HI, M.GRADIENT, *ELEMENTS["rect3x3"], iterations=3)
        b = _Bufs(ctx)
        d_in = b.upload(px)
        for op, name, border, it, route in ((R.OPEN, "rect3x3", (R.BORDER_NEUTRAL, 0), 2, 0), (R.GRADIENT, "ellipse7x7", (R.BORDER_REPLICATE, 0), 3, 0),
                                            (R.BLACKHAT, "rect15x15", (R.BORDER_CONSTANT, 30), 2, 2), (R.ERODE, "L", (R.BORDER_NEUTRAL, 0), 5, 1),
                                            (R.MEDIAN, "rect5x5", (R.BORDER_REPLICATE, 0), 3, 2)):
            want = R.gray_morph(px, op, *ELEMENTS[name], *border, it)
            runs = []
            for _ in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(run(ctx, b, "dirty", px.shape, d_in, want, op, ELEMENTS[name], border, it, route))
            assert runs[0] == runs[1] == runs[2]
        assert any(name == "morph_ws" and kind == hip.WS_DATA and nbytes >= 2 * n * h * w for name, _p, nbytes, kind in ctx.selftest_workspaces())
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 3 x 5 frame and 4096 workgroups at most: 4100 frames send workgroups through a second trip, as the plan
    query says."""
    assert hip.gray_morph_plan(4096, 3, 5).trips == 1
    plan = hip.gray_morph_plan(4100, 3, 5)
    assert (plan.units, plan.grid, plan.per_group, plan.trips) == (4100, 4096, 1, 2)
    px = R.named_planes(4100, 3, 5, 9)["random"]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(px)
        want = R.gray_morph(px, R.DILATE, *ELEMENTS["rect3x3"], R.BORDER_REPLICATE, 0, 1)
        want_median = R.gray_morph(px, R.MEDIAN, *ELEMENTS["rect3x3"], R.BORDER_REPLICATE, 0, 1)
        for r in ROUTES:
            run(ctx, b, "4100 frames", px.shape, d_in, want, R.DILATE, ELEMENTS["rect3x3"], (R.BORDER_REPLICATE, 0), 1, r)
            run(ctx, b, "4100 frames", px.shape, d_in, want_median, R.MEDIAN, ELEMENTS["rect3x3"], (R.BORDER_REPLICATE, 0), 1, r)
        want = R.gray_morph(px, R.TOPHAT, *ELEMENTS["L"], R.BORDER_CONSTANT, 40, 2)
        run(ctx, b, "4100 frames", px.shape, d_in, want, R.TOPHAT, ELEMENTS["L"], (R.BORDER_CONSTANT, 40), 2)
        b.free()


def test_gray_morph_batch_on_host_frames_and_the_profile_part(hip):
    px = R.named_planes(3, 45, 150, 3)["random"]
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.profile_reset()
        for k, (op, name, border, it) in enumerate(((R.CLOSE, "rect3x3", (R.BORDER_NEUTRAL, 0), 1), (R.GRADIENT, "ellipse7x7", (R.BORDER_CONSTANT, 0), 2),
                                                    (R.MEDIAN, "rect3x3", (R.BORDER_REPLICATE, 0), 1))):
            out = ctx.gray_morph_batch(px, op, *ELEMENTS[name], *border, it)
            same(out, R.gray_morph(px, op, *ELEMENTS[name], *border, it), f"gray_morph_batch op {op}")
            assert ctx.profile_part("gray_morph", 0)[1] == k + 1
        assert ctx.profile_part("gray_morph", 0)[0] > 0 and ctx.profile_part("morph", 0)[1] == 0
        with pytest.raises(capi.CannyHipError):
            ctx.profile_part("gray_morph", 1)
        assert ctx.get_option("gray_morph_route") == 0
        ctx.set_option("gray_morph_route", 2)
        assert ctx.get_option("gray_morph_route") == 2
        with pytest.raises(capi.CannyHipError):
            ctx.set_option("gray_morph_route", 3)


def test_the_refused_calls(hip):
    n, h, w = 2, 20, 30
    px = R.named_planes(n, h, w, 40)["random"]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(px)
        d_out = b.filled(n * h * w)
        good = dict(src=d_in, n=n, h=h, w=w, op=R.OPEN, rows=[7, 7, 7], kw=3, kh=3, out=d_out, mode=0, value=0, it=1)

        def call(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_gray_morph(a["src"], a["n"], a["h"], a["w"], a["op"], a["rows"], a["kw"], a["kh"], a["out"], a["mode"], a["value"],
                                   a["it"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(op=-1), dict(op=8), dict(mode=-1), dict(mode=3),
                   dict(mode=2, value=256), dict(mode=2, value=-1), dict(it=0), dict(it=17), dict(rows=[7, 8, 7]), dict(rows=[0, 0, 0]),
                   dict(kw=2, rows=[3, 3, 3]), dict(kh=2, rows=[7, 7]), dict(kw=33), dict(kw=0), dict(op=R.MEDIAN, mode=0),
                   dict(op=R.MEDIAN, mode=1, rows=[7, 5, 7]), dict(op=R.MEDIAN, mode=1, rows=[127] * 7, kw=7, kh=7),
                   dict(op=R.MEDIAN, mode=1, rows=[31] * 3, kw=5, kh=3), dict(src=0),            # no canny call yet: no plane
                   dict(out=d_in), dict(out=d_in + n * h * w - 1), dict(src=d_out + 5)):           # no in-place form
            assert call(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
            assert call(**kw) == 2, kw
        ctx.synchronize()
        b.untouched()
        assert call() == 0 and call(mode=1, value=999) == 0
        same(b.get(d_out, "out").reshape(px.shape), R.gray_morph(px, R.OPEN, [7, 7, 7], 3, 3, R.BORDER_REPLICATE), "after the refusals")
        b.free()


def test_blackhat_otsu_components_finds_the_blobs_on_one_stream(hip):
    """Dark blobs of 5..9 pixels on a 96 x 160 brightness ramp: BLACKHAT by a 15 x 15 rectangle -> OTSU -> components yields
    exactly the blobs; OTSU alone cuts the ramp.  First on the rules, then dev_gray_morph -> dev_binarize ->
    dev_components_bits on one stream with nothing downloaded in between."""
    plane, truth = R.blobs_on_ramp()
    h, w = plane.shape
    rb = (w + 7) // 8
    el = ELEMENTS["rect15x15"]
    want_hat = R.gray_morph(plane[None], R.BLACKHAT, *el)
    want_bits, want_n, want_thr = B.binarize(want_hat, B.OTSU)
    assert np.array_equal(B.unpack(want_bits, w)[0], truth)
    want_labels, want_stats, want_off = components_rule.csr(B.unpack(want_bits, w), 1)
    n_blobs = len(components_rule.csr(truth[None], 1)[1])
    assert len(want_stats) == n_blobs == 8
    alone = B.unpack(B.binarize(plane[None], B.OTSU, invert=1)[0], w)[0]
    assert not np.array_equal(alone, truth) and len(components_rule.csr(alone[None], 1)[1]) != n_blobs
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(plane, odd=True)
        for r in ROUTES:
            d_hat, d_bits, d_cnt, d_thr = b.filled(h * w), b.filled(h * rb), b.filled(8), b.filled(4)
            d_labels, d_stats, d_off = b.filled(h * w * 4), b.filled(n_blobs * 6 * 4), b.filled(2 * 8)
            ctx.set_option("gray_morph_route", r)
            ctx.dev_gray_morph(d_in, 1, h, w, R.BLACKHAT, *el, d_hat)
            ctx.dev_binarize(d_hat, 1, h, w, B.OTSU, 0, d_bits, d_cnt, d_thr)
            ctx.dev_components_bits(d_bits, h, w, 1, 1, d_labels, 0, d_stats, n_blobs, d_off)
            same(b.get(d_hat, "black hat").reshape(1, h, w), want_hat, "black hat")
            same(b.get(d_bits, "bits").reshape(1, h, rb), want_bits, "bits")
            assert b.get(d_cnt, "counts").view(np.int64).tolist() == want_n.tolist() == [int(truth.sum())]
            assert b.get(d_thr, "threshold").view(np.int32).tolist() == want_thr.tolist()
            assert b.get(d_off, "offsets").view(np.uint64).tolist() == [0, n_blobs]
            same(b.get(d_stats, "stats").view(np.int32).reshape(n_blobs, 6), want_stats, "stats")
            same(b.get(d_labels, "labels").view(np.int32).reshape(1, h, w), want_labels, "labels")
        b.free()


def test_cli_writes_the_gray_plane_and_its_binarization(hip, fixture_image, tmp_path):
    """Main ... -G: the operator on the input frame into canny_gray.pgm; with -a also the binarization of THAT plane into
    canny_gray_binary.pgm, while canny_binary.pgm stays the binarization of the input frame."""
    import os
    import subprocess
    h, w = fixture_image.shape
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + fixture_image.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canny_edge_amd", "Main")
    plane_of = lambda p: np.frombuffer(p.read_bytes()[-h * w:], np.uint8).reshape(h, w)
    for value, (op, name, border, it) in (("blackhat,15", (R.BLACKHAT, "rect15x15", (R.BORDER_NEUTRAL, 0), 1)),
                                          ("median,5", (R.MEDIAN, "rect5x5", (R.BORDER_REPLICATE, 0), 1)),
                                          ("gradient,7,7,ellipse,2,77", (R.GRADIENT, "ellipse7x7", (R.BORDER_CONSTANT, 77), 2)),
                                          ("open,5,3,rect,1,replicate", (R.OPEN, "rect5x3", (R.BORDER_REPLICATE, 0), 1))):
        want = R.gray_morph(fixture_image[None], op, *ELEMENTS[name], *border, it)
        out = tmp_path / ("out_" + value.replace(",", "_"))
        out.mkdir()
        r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(out), "-G", value], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert (out / "canny_gray.pgm").read_bytes().startswith(b"P5\n%d %d\n255\n" % (w, h))
        same(plane_of(out / "canny_gray.pgm")[None], want, value)
        assert not (out / "canny_gray_binary.pgm").exists() and not (out / "canny_binary.pgm").exists()
        both = tmp_path / ("both_" + value.replace(",", "_"))
        both.mkdir()
        r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(both), "-a", "otsu", "-G", value], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        same(plane_of(both / "canny_gray.pgm")[None], want, value)
        bits, _, thr = B.binarize(want, B.OTSU)
        same(plane_of(both / "canny_gray_binary.pgm"), np.where(B.unpack(bits, w)[0], 255, 0), value + " binarized")
        frame_bits, _, frame_thr = B.binarize(fixture_image[None], B.OTSU)
        same(plane_of(both / "canny_binary.pgm"), np.where(B.unpack(frame_bits, w)[0], 255, 0), "canny_binary.pgm")
        assert "otsu threshold %d\n" % frame_thr[0] in r.stdout and "gray otsu threshold %d\n" % thr[0] in r.stdout
