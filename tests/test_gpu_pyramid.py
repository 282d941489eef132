"""Image pyramids on the GPU (canny_hip_dev_pyr_down, canny_hip_dev_pyramid, canny_hip_dev_pyr_up and the host-buffer forms;
DESIGN.md section 40) against tests/pyramid_rule.py, byte for byte: every output byte, with sentinel bytes in front of and
behind each output and in the pads between the levels, under both routes."""
import os
import subprocess

import numpy as np
import pytest

import corners_rule as cr
import gray_morph_rule as G
import oracle
import pyramid_rule as R
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
ROUTES = (capi.PYR_ROUTE_DIRECT, capi.PYR_ROUTE_TILED)
# the source sizes around one tile (64 x 256) and around the folds; 130 x 520 and 131 x 522 have a tile whose footprint lies
# inside the frame (the tiled route's path without folds where the rows start on word addresses, 520, and where not, 522)
SHAPES = ((1, 1), (1, 2), (2, 2), (3, 5), (1, 300), (300, 1), (64, 256), (65, 257), (66, 258), (63, 255), (67, 131), (70, 77),
          (130, 520), (131, 522))
UP_SHAPES = ((1, 1), (2, 3), (33, 70), (64, 129))


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard bytes around each, and plain uploads; `off`: the data
    starts that many bytes into the allocation (which is aligned)."""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptrs = ctx, {}, []

    def filled(self, nbytes, off=0):
        p = self.ctx.malloc(N_GUARD + off + nbytes + N_GUARD)
        self.ptrs.append(p)
        self.size[p + N_GUARD + off] = (nbytes, N_GUARD + off)
        self.ctx.h2d(p, np.full(N_GUARD + off + nbytes + N_GUARD, SENT, np.uint8))
        return p + N_GUARD + off

    def upload(self, a, off=0):
        a = np.concatenate([np.full(off, 0xFF, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.ctx.h2d(p, a)
        return p + off

    def get(self, p, what=""):
        nbytes, lead = self.size[p]
        out = np.empty(lead + nbytes + N_GUARD, np.uint8)
        self.ctx.d2h(out, p - lead)
        assert (out[:lead] == SENT).all() and (out[lead + nbytes:] == SENT).all(), f"guard bytes overwritten around {what}"
        return out[lead:lead + nbytes]

    def untouched(self):
        for p in self.size:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.size, self.ptrs = {}, []


def same(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def down(ctx, b, what, d_in, shape, want, route, off=0):
    """One dev_pyr_down into a sentinel-filled output, compared with `want`."""
    n, h, w = shape
    d_out = b.filled(want.size, off)
    ctx.set_option("pyramid_route", route)
    ctx.dev_pyr_down(d_in, n, h, w, d_out)
    ctx.set_option("pyramid_route", 0)
    same(b.get(d_out, what).reshape(want.shape), want, f"{what} route {route}")


def up(ctx, b, what, d_in, shape, oh, ow, want, off=0):
    n, h, w = shape
    d_out = b.filled(want.size, off)
    ctx.dev_pyr_up(d_in, n, h, w, oh, ow, d_out)
    same(b.get(d_out, what).reshape(want.shape), want, what)


def pyramid(ctx, b, what, d_in, shape, levels, route, off=0):
    """One dev_pyramid into a sentinel-filled buffer: every level's bytes and every pad byte."""
    n, h, w = shape
    total = R.layout(n, h, w, levels)[1]
    d_out = b.filled(total, off)
    ctx.set_option("pyramid_route", route)
    ctx.dev_pyramid(d_in, n, h, w, levels, d_out)
    ctx.set_option("pyramid_route", 0)
    return b.get(d_out, what), d_out


@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_down_under_both_routes(hip, h, w):
    planes = R.named_planes(3, h, w, 7 * h + w)
    want = R.pyr_down(planes)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        for route in ROUTES + (capi.PYR_ROUTE_AUTO,):
            down(ctx, b, f"3 x {h} x {w}", d_in, planes.shape, want, route)
        b.free()


@pytest.mark.parametrize("h,w", [(70, 77), (65, 257), (5, 300)])
def test_the_pyramid_to_the_deepest_level(hip, h, w):
    """... which is 1 x 1, through levels 2 and 3 wide where the fold loops; the pads between the levels keep the sentinel."""
    n = 3
    planes = R.named_planes(n, h, w, h)
    top = R.max_levels(h, w)
    want = R.pyramid(planes, top)
    assert want[-1].shape == (n, 1, 1) and {lv.shape[2] for lv in want} >= {2, 3}
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        for route in ROUTES:
            for levels in (1, 2, top):
                got, _ = pyramid(ctx, b, f"{h} x {w} levels {levels}", d_in, planes.shape, levels, route)
                same(got, R.pack(want[:levels], n, h, w, SENT), f"{h} x {w} levels {levels} route {route}")
        b.free()


@pytest.mark.parametrize("off_in,off_out", [(1, 1), (2, 3), (3, 2), (0, 1), (1, 0)])
def test_odd_base_addresses(hip, off_in, off_out):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for h, w in ((67, 131), (130, 520), (3, 5)):
            planes = R.named_planes(3, h, w, off_in + 4 * off_out)
            d_in = b.upload(planes, off_in)
            want = R.pyr_down(planes)
            for route in ROUTES:
                down(ctx, b, f"{h} x {w} at +{off_in} -> +{off_out}", d_in, planes.shape, want, route, off_out)
            levels = R.max_levels(h, w)
            got, _ = pyramid(ctx, b, "pyramid", d_in, planes.shape, levels, capi.PYR_ROUTE_TILED, off_out)
            same(got, R.pack(R.pyramid(planes, levels), 3, h, w, SENT), f"pyramid {h} x {w} at +{off_in} -> +{off_out}")
            up(ctx, b, f"up {h} x {w} at +{off_in} -> +{off_out}", d_in, planes.shape, 2 * h - 1, 2 * w, R.pyr_up(planes, 2 * h - 1, 2 * w),
               off_out)
            b.free()


def test_the_refused_calls(hip):
    n, h, w = 2, 20, 30
    planes = R.named_planes(n, h, w, 1)
    total = R.layout(n, h, w, 3)[1]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        d_out = b.filled(max(total, n * 40 * 60))

        def st(call, *args):
            try:
                call(*args)
            except capi.CannyHipError as e:
                return e.status
            return 0

        for args in ((d_in, n, h, w, 0), (d_in, 0, h, w, d_out), (d_in, n, 0, w, d_out), (d_in, n, h, -1, d_out), (0, n, h, w, d_out),
                     (d_in, n, h, w, d_in), (d_in, n, h, w, d_in + n * h * w - 1), (d_out + 5, n, h, w, d_out)):
            assert st(ctx.dev_pyr_down, *args) == 1, args                # (0, ..): no canny call yet, no plane
        for args in ((d_in, n, h, w, 3, 0), (d_in, n, h, w, 0, d_out), (d_in, n, h, w, 6, d_out), (d_in, n, h, w, 16, d_out),
                     (d_in, n, h, w, -1, d_out), (d_in, n, 1, 1, 1, d_out), (0, n, h, w, 3, d_out), (d_in, n, h, w, 3, d_in + 100),
                     (d_out + total - 1, n, h, w, 3, d_out), (d_out + 300, n, h, w, 3, d_out)):   # + 300: it begins in a pad
            assert st(ctx.dev_pyramid, *args) == 1, args
        for args in ((0, n, h, w, 40, 60, d_out), (d_in, n, h, w, 40, 60, 0), (d_in, n, h, w, 41, 60, d_out), (d_in, n, h, w, 38, 60, d_out),
                     (d_in, n, h, w, 40, 58, d_out), (d_in, n, h, w, 40, 61, d_out), (d_in, 0, h, w, 40, 60, d_out),
                     (d_in, n, h, w, 40, 60, d_in + 7), (d_out + 100, n, h, w, 40, 60, d_out)):
            assert st(ctx.dev_pyr_up, *args) == 1, args
        for args in ((d_in, 65536, h, w, d_out), (d_in, n, 32769, w, d_out), (d_in, n, h, 32769, d_out), (d_in, n, 32768, 65536, d_out)):
            assert st(ctx.dev_pyr_down, *args) == 2, args
        assert st(ctx.dev_pyramid, d_in, 65536, h, w, 3, d_out) == 2 and st(ctx.dev_pyramid, d_in, n, 32769, w, 3, d_out) == 2
        assert st(ctx.dev_pyr_up, d_in, n, 16385, w, 32770, 2 * w, d_out) == 2
        assert st(ctx.dev_pyr_up, d_in, 65536, h, w, 40, 60, d_out) == 2
        ctx.synchronize()
        b.untouched()
        assert st(ctx.dev_pyramid, d_in, n, h, w, 3, d_out) == 0
        got = b.get(d_out, "after the refusals")
        same(got[:total], R.pack(R.pyramid(planes, 3), n, h, w, SENT), "after the refusals")
        assert (got[total:] == SENT).all()
        b.free()


@pytest.mark.parametrize("n,h,w,kept", [(3, 37, 77, {0}), (2, 72, 200, {0, 1})])
def test_the_contexts_smoothed_plane(hip, n, h, w, kept):
    """d_plane = NULL after dev_canny: the rule on the oracle's Gaussian plane, whether the context kept bytes or shorts (at
    37 x 77 it keeps shorts under both settings of "smoothed_u8": the shape does not permit bytes)."""
    imgs = np.stack([synth_frame(h, w, 11 + s) for s in range(n)])
    planes = np.stack([oracle.gaussian(f, SIGMA) for f in imgs])
    assert planes.min() >= 0 and planes.max() <= 255
    planes = planes.astype(np.uint8)
    levels = R.max_levels(h, w)
    want, want_pyr = R.pyr_down(planes), R.pack(R.pyramid(planes, levels), n, h, w, SENT)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges = b.upload(imgs), b.filled(n * h * w * 2)
        d_none = b.filled(n * h * w)
        for call in (lambda: ctx.dev_pyr_down(0, n, h, w, d_none), lambda: ctx.dev_pyramid(0, n, h, w, 2, d_none)):
            with pytest.raises(capi.CannyHipError) as ei:             # a context that ran no canny call has no plane
                call()
            assert ei.value.status == 1
        seen = set()
        for u8 in (0, 1):
            ctx.set_option("smoothed_u8", u8)
            ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
            seen.add(ctx.get_option("last_canny_smoothed_u8"))
            for route in ROUTES:
                down(ctx, b, f"plane u8 {u8}", 0, planes.shape, want, route)
                got, _ = pyramid(ctx, b, f"plane u8 {u8}", 0, planes.shape, levels, route)
                same(got, want_pyr, f"pyramid of the plane, u8 {u8} route {route}")
        assert seen == kept
        for n2, h2, w2 in ((n - 1, h, w), (n, h - 1, w), (n, w, h)):   # ... nor one of another shape
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_pyr_down(0, n2, h2, w2, d_none)
            assert ei.value.status == 1
        ctx.synchronize()
        assert (b.get(d_none) == SENT).all()
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 3 x 5 frame and 4096 workgroups at most: 4100 frames send workgroups through a second trip, as the plan
    query says -- pyrDown under both routes, and pyrUp, whose output 6 x 10 is one tile a frame as well."""
    assert hip.pyramid_plan(4096, 3, 5).trips == 1
    plan = hip.pyramid_plan(4100, 3, 5)
    assert (plan.units, plan.grid, plan.per_group, plan.trips) == (4100, 4096, 1, 2)
    assert hip.pyramid_plan(4100, 12, 20)[:4] == plan[:4]               # the plan of a launch that writes 6 x 10 planes
    planes = np.random.default_rng(9).integers(0, 256, (4100, 3, 5), dtype=np.uint8)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        want = R.pyr_down(planes)
        for route in ROUTES:
            down(ctx, b, "4100 frames", d_in, planes.shape, want, route)
        up(ctx, b, "4100 frames up", d_in, planes.shape, 6, 10, R.pyr_up(planes, 6, 10))
        up(ctx, b, "4100 frames up", d_in, planes.shape, 5, 9, R.pyr_up(planes, 5, 9))
        b.free()


@pytest.mark.parametrize("h,w", UP_SHAPES)
def test_pyr_up_to_all_four_sizes(hip, h, w):
    planes = R.named_planes(3, h, w, 3 * h + w)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        for oh in (2 * h - 1, 2 * h):
            for ow in (2 * w - 1, 2 * w):
                up(ctx, b, f"{h} x {w} -> {oh} x {ow}", d_in, planes.shape, oh, ow, R.pyr_up(planes, oh, ow))
        b.free()


def test_the_round_trip_of_an_odd_sized_plane(hip):
    """Level 1 of 65 x 257 planes (33 x 129) goes back up onto 65 x 257, on the device from the pyramid's own buffer."""
    n, h, w = 3, 65, 257
    planes = R.named_planes(n, h, w, 2)
    level1 = R.pyr_down(planes)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        _, d_pyr = pyramid(ctx, b, "pyramid", b.upload(planes), planes.shape, 2, 0)
        up(ctx, b, "round trip", d_pyr, level1.shape, h, w, R.pyr_up(level1, h, w))
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs the grey morphology, the binarization and a pyramid
    of another shape, and every data workspace it holds is filled with a sentinel before each of three identical runs."""
    other = R.named_planes(3, 90, 200, 6)
    n, h, w = 3, 70, 131
    planes = R.named_planes(n, h, w, 21)
    levels = R.max_levels(h, w)
    want = R.pack(R.pyramid(planes, levels), n, h, w, SENT)
    want_up = R.pyr_up(planes, 2 * h, 2 * w - 1)
    with hip.Context(0) as ctx:
        ctx.gray_morph_batch(other, capi.GRAY_GRADIENT, *G.named_elements()["rect5x3"], iterations=3)
        ctx.binarize_batch(other, capi.BIN_OTSU)
        ctx.pyramid_batch(other, 4)
        ctx.pyr_up_batch(other, 180, 399)
        b = _Bufs(ctx)
        d_in = b.upload(planes)
        for route in ROUTES:
            runs = []
            for _ in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                got, _ = pyramid(ctx, b, "dirty", d_in, planes.shape, levels, route)
                same(got, want, f"dirty route {route}")
                up(ctx, b, "dirty up", d_in, planes.shape, 2 * h, 2 * w - 1, want_up)
                runs.append(got.tobytes())
            assert runs[0] == runs[1] == runs[2]
        b.free()


def test_levels_go_to_canny_and_corners_as_they_lie(hip):
    """Levels 1 and 2 of a 3 x 140 x 256 batch are handed as they lie in the pyramid's buffer (d_out + off_l) to dev_canny and
    to dev_corners_plane: the outputs equal the oracle and tests/corners_rule.py on the numpy rule's levels."""
    n, h, w = 3, 140, 256
    frames = np.stack([synth_frame(h, w, s) for s in (1, 2, 3)])
    levels = R.pyramid(frames, 2)
    rows, total = R.layout(n, h, w, 2)
    cmax, corner_args = 64, (cr.MIN_EIGEN, 3, 0, 655, 0, 3)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        got, d_pyr = pyramid(ctx, b, "pyramid", b.upload(frames), frames.shape, 2, 0)
        same(got, R.pack(levels, n, h, w, SENT), "the pyramid")
        for lv, (hl, wl, off, _nbytes) in zip(levels, rows):
            d_edges = b.filled(n * hl * wl * 2)
            ctx.dev_canny(d_pyr + off, SIGMA, LO, HI, hl, wl, n, d_edges)
            edges = b.get(d_edges, "edges").view(np.int16).reshape(n, hl, wl)
            same(edges, np.stack([oracle.canny(f, SIGMA, LO, HI) for f in lv]), f"canny on the level {hl} x {wl}")
            d_rec, d_cnt = b.filled(32 * n * cmax), b.filled(4 * n)
            ctx.dev_corners_plane(d_pyr + off, n, hl, wl, *corner_args, cmax, d_rec, d_cnt, 0, 0, 0)
            cnt = b.get(d_cnt, "counts").view(np.int32)
            rec = b.get(d_rec, "records").view(np.int64).reshape(n, cmax, 4)
            want = [cr.corners(P, *corner_args, cmax)[0] for P in lv]
            assert cnt.tolist() == [len(r) for r in want] and sum(cnt) > 0, (hl, wl, cnt.tolist())
            for f, r in enumerate(want):
                assert np.array_equal(rec[f, :len(r)], r), f"corners on the level {hl} x {wl}, frame {f}"
        same(b.get(d_pyr, "the pyramid afterwards"), R.pack(levels, n, h, w, SENT), "the calls only read the levels")
        b.free()


def test_the_host_buffer_forms_and_the_profile_parts(hip):
    planes = R.named_planes(3, 45, 150, 3)
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.profile_reset()
        for k, levels in enumerate((1, 3, R.max_levels(45, 150))):
            got = ctx.pyramid_batch(planes, levels)
            want = R.pyramid(planes, levels)
            assert len(got) == levels
            for g, x in zip(got, want):
                same(g, x, f"pyramid_batch levels {levels}")
            assert ctx.profile_part("pyramid", capi.PYR_PART_DOWN)[1] == k + 1
        assert hip.pyramid_batch(ctx, planes, 2)[1].tobytes() == R.pyramid(planes, 2)[1].tobytes()
        # the pads of the caller's buffer stay as they are
        total = R.layout(3, 45, 150, 3)[1]
        buf = np.full(total + 64, SENT, np.uint8)
        assert ctx._L.canny_hip_pyramid_batch(ctx._h, capi._hp(planes), 3, 45, 150, 3, capi._hp(buf)) == 0
        assert np.array_equal(buf[:total], R.pack(R.pyramid(planes, 3), 3, 45, 150, SENT)) and (buf[total:] == SENT).all()
        assert ctx.profile_part("pyramid", capi.PYR_PART_UP)[1] == 0
        for oh, ow in ((90, 300), (89, 299)):
            same(ctx.pyr_up_batch(planes, oh, ow), R.pyr_up(planes, oh, ow), f"pyr_up_batch {oh} x {ow}")
        same(hip.pyr_up_batch(ctx, planes, 89, 300), R.pyr_up(planes, 89, 300), "pyr_up_batch")
        assert ctx.profile_part("pyramid", capi.PYR_PART_UP)[1] == 3 and ctx.profile_part("pyramid", capi.PYR_PART_UP)[0] > 0
        assert ctx.profile_part("pyramid", capi.PYR_PART_DOWN)[0] > 0 and ctx.profile_part("gray_morph", 0)[1] == 0
        with pytest.raises(capi.CannyHipError):
            ctx.profile_part("pyramid", 2)
        for bad in (lambda: ctx.pyramid_batch(planes, 9), lambda: ctx.pyramid_batch(planes, 0), lambda: ctx.pyr_up_batch(planes, 91, 300)):
            with pytest.raises(capi.CannyHipError) as ei:
                bad()
            assert ei.value.status == 1
        assert ctx.get_option("pyramid_route") == 0
        ctx.set_option("pyramid_route", 2)
        assert ctx.get_option("pyramid_route") == 2
        with pytest.raises(capi.CannyHipError):
            ctx.set_option("pyramid_route", 3)


def test_cli_writes_the_levels(hip, fixture_image, tmp_path):
    """Main ... -P 3,up: the levels of the input frame into canny_pyr1.pgm .. canny_pyr3.pgm and level 1 brought back to the
    frame's size into canny_pyr_up.pgm."""
    h, w = fixture_image.shape
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + fixture_image.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canny_edge_amd", "Main")
    want = R.pyramid(fixture_image[None], 3)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(out), "-P", "3,up"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for l, lv in enumerate(want):
        hl, wl = lv.shape[1:]
        data = (out / f"canny_pyr{l + 1}.pgm").read_bytes()
        assert data.startswith(b"P5\n%d %d\n255\n" % (wl, hl))
        same(np.frombuffer(data[-hl * wl:], np.uint8).reshape(1, hl, wl), lv, f"canny_pyr{l + 1}.pgm")
    assert not (out / "canny_pyr4.pgm").exists()
    data = (out / "canny_pyr_up.pgm").read_bytes()
    assert data.startswith(b"P5\n%d %d\n255\n" % (w, h))
    same(np.frombuffer(data[-h * w:], np.uint8).reshape(1, h, w), R.pyr_up(want[0], h, w), "canny_pyr_up.pgm")
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(plain), "-P", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and (plain / "canny_pyr2.pgm").exists() and not (plain / "canny_pyr_up.pgm").exists()
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(plain), "-P", "9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "has no level 9" in r.stderr                 # 256 x 256 has 8 levels
