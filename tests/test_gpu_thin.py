"""Thinning on the GPU (canny_hip_dev_thin_bits, canny_hip_dev_canny_thin, canny_hip_thin_batch) against
tests/thin_rule.py, byte for byte: every output byte and every word of info, with sentinel bytes behind each buffer, info
untouched when it is not asked for, and the same bytes under the stepwise route, the fused route at 1, 2 and 8 iterations a
launch and whatever automatic takes."""
import itertools

import numpy as np
import pytest

import curves_rule
import thin_rule as R
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
WIDTHS = (1, 7, 8, 9, 63, 64, 65, 127, 129, 511, 512, 513, 577)
HEIGHTS = (1, 2, 15, 16, 17, 63, 64, 65, 97, 129)
BATCHES = (1, 3, 5)
# (thin_route, thin_fuse): stepwise, fused at 1, 2 and 8 full iterations a launch, automatic
SETTINGS = ((capi.THIN_ROUTE_STEPWISE, 0), (capi.THIN_ROUTE_FUSED, 1), (capi.THIN_ROUTE_FUSED, 2), (capi.THIN_ROUTE_FUSED, 8),
            (capi.THIN_ROUTE_AUTO, 0))


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


def check_output(b, what, d_out, d_info, shape, want, want_info, with_info):
    out = b.get(d_out, what + ": out").reshape(shape)
    info = b.get(d_info, what + ": info")
    same(out, want, what)
    if with_info:
        assert info.view(np.int64).reshape(-1, 4).tolist() == want_info.tolist(), what + ": info"
    else:
        assert (info == SENT).all(), what + ": info written without a buffer"
    return out.tobytes() + info.tobytes()


def thin_and_check(ctx, b, what, bits, w, method, k=0, setting=(0, 0), with_info=True, odd=False, d_in=None, want=None):
    n, h, rb = bits.shape
    want, want_info = want if want is not None else R.thin(bits, w, method, k)
    d_in = b.upload(bits, odd) if d_in is None else d_in
    d_out, d_info = b.filled(n * h * rb), b.filled(n * 32)
    ctx.set_option("thin_route", setting[0])
    ctx.set_option("thin_fuse", setting[1])
    ctx.dev_thin_bits(d_in, n, h, w, method, d_out, d_info if with_info else 0, k)
    ctx.set_option("thin_route", 0)
    ctx.set_option("thin_fuse", 0)
    return check_output(b, f"{what} route {setting[0]} fuse {setting[1]}", d_out, d_info, (n, h, rb), want, want_info, with_info)


def every_setting(ctx, b, what, px, method, k=0, dirty=None, odd=False, with_info=True):
    """One map under every route and fuse: the rule's bytes and info, identical among the settings.  -> the rule's info."""
    px = np.asarray(px, bool)
    w = px.shape[-1]
    bits = R.pack(px) if dirty is None else R.pack_dirty(px, dirty)
    want = R.thin(bits, w, method, k)
    d_in = b.upload(bits, odd)
    runs = [thin_and_check(ctx, b, what, bits, w, method, k, s, with_info, d_in=d_in, want=want) for s in SETTINGS]
    assert all(r == runs[0] for r in runs), what + ": the settings differ"
    return want[1]


def random_maps(n, h, w, seed):
    rng = np.random.default_rng(seed)
    if min(h, w) > 6:
        return np.stack([R.blobs(h, w, seed * 8 + f, 3 + (seed + f) % 5) for f in range(n)])
    return rng.random((n, h, w)) < 0.7


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_with_heights_batches_and_both_methods(hip, w):
    wi = WIDTHS.index(w)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for j in range(4):   # a thinned product: every height meets five or six widths
            k = 4 * wi + j
            h = HEIGHTS[(wi + 3 * j) % len(HEIGHTS)]
            n = BATCHES[k % 3]
            px = random_maps(n, h, w, k)
            every_setting(ctx, b, f"{n} x {h} x {w} method {(wi + j) % 2}", px, (wi + j) % 2, 0, np.random.default_rng(k) if k % 3 else None,
                          odd=k % 5 == 0, with_info=k % 4 != 3)
            b.free()


def designed(name):
    """name -> (bool [n, h, w], iterations the slowest frame must take under GUOHALL or None)"""
    if name == "bar40":       # across column 512 and row 64: both tile edges, more than one fused launch at every fuse
        return R.bar(129, 577, 44, 40, 30, 560)[None], 20
    if name == "bars1to9":
        return np.stack([R.bar(30, 70, 7, t, 3, 66) for t in range(1, 10)]), 4
    if name == "square2":
        return R.square2()[None], None
    if name == "diagonal2":   # the two-wide diagonal across the word edge at column 64
        return R.diagonal2(12, 2, 55)[None], None
    if name == "allset":
        return np.ones((2, 65, 130), bool), None
    if name == "empty":
        return np.zeros((2, 65, 130), bool), 0
    if name == "checker":
        yy, xx = np.mgrid[:66, :131]
        return ((yy + xx) & 1).astype(bool)[None], None
    if name == "scene":
        return R.demo_scene()[None], 5
    if name == "blobs":
        return np.stack([R.blobs(97, 200, s, 9) for s in range(3)]), None
    raise KeyError(name)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", ["bar40", "bars1to9", "square2", "diagonal2", "allset", "empty", "checker", "scene", "blobs"])
def test_designed_maps(hip, name, method):
    px, slowest = designed(name)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        info = every_setting(ctx, b, name, px, method, 0, np.random.default_rng(7))
        b.free()
    assert (info[:, 3] == 1).all()
    if slowest is not None and method == R.GUOHALL:
        assert info[:, 1].max() == slowest
    if name == "bars1to9":
        assert info[:, 1].tolist() == [t // 2 for t in range(1, 10)]
    if name == "square2":
        assert info[0, 0] == (0, 1)[method]


def test_a_batch_whose_frames_converge_after_0_2_and_20_iterations_in_every_order(hip):
    h, w = 97, 130
    frames = {0: R.bar(h, w, 50, 1, 5, 120), 2: R.bar(h, w, 20, 5, 9, 100), 20: R.bar(h, w, 30, 40, 4, 126)}
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, order in enumerate(itertools.permutations((0, 2, 20))):
            px = np.stack([frames[d] for d in order])
            for method in R.METHODS if i % 3 == 0 else (R.GUOHALL,):
                info = every_setting(ctx, b, f"order {order} method {method}", px, method)
                assert info[:, 1].tolist() == list(order) and (info[:, 3] == 1).all()
            b.free()


@pytest.mark.parametrize("method", R.METHODS)
def test_max_iterations_cuts_the_bar(hip, method):
    px, d = R.bar(97, 130, 30, 40, 4, 126)[None], 20
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for k, want_it, want_conv in ((1, 1, 0), (d - 1, d - 1, 0), (d, d, 0), (d + 1, d, 1), (0, d, 1)):
            info = every_setting(ctx, b, f"k {k}", px, method, k)
            assert info[0, 1] == want_it and info[0, 3] == want_conv
            b.free()


def test_the_fixed_point_of_a_frame_that_needs_more_iterations_than_the_poll_chunks(hip):
    """max_iterations = 0 polls behind 8, 16, then 32 iterations: a bar 120 thick needs 60 and goes through four chunks; its
    neighbour frame has converged in the first."""
    px = np.stack([R.bar(140, 140, 10, 120, 3, 137), R.bar(140, 140, 60, 6, 3, 137)])
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        info = every_setting(ctx, b, "bar 120", px, R.GUOHALL)
        assert info[:, 1].tolist() == [60, 3]
        info = every_setting(ctx, b, "bar 120, k 57", px, R.ZHANGSUEN, 57)   # the last chunk cut by max_iterations
        assert info[:, 1].tolist() == [57, 3] and info[:, 3].tolist() == [0, 1]
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 3 x 5 frame and 4096 workgroups at most: 4097 frames send workgroup 0 through a second trip, as the plan
    query says."""
    assert hip.thin_plan(4096, 3, 5).trips == 1
    plan = hip.thin_plan(4097, 3, 5)
    assert (plan.units, plan.grid, plan.per_group) == (4097, 4096, 1) and plan.trips >= 2
    px = np.random.default_rng(9).random((4097, 3, 5)) < 0.8
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for method in R.METHODS:
            info = every_setting(ctx, b, "4097 frames", px, method, 0, np.random.default_rng(1))
            assert len(set(info[:, 1].tolist())) > 1, "frames that stop at different iterations"
            b.free()


def test_dev_canny_thin_behind_dev_canny(hip):
    n, h, w = 3, 70, 200
    frames = np.stack([synth_frame(h, w, 11 + s) for s in range(n)])
    rb = (w + 7) // 8
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges, d_bits = b.upload(frames), b.filled(n * h * w * 2), b.filled(n * h * rb)
        ctx.dev_canny_bits(d_img, SIGMA, LO, HI, h, w, n, d_bits)
        bits = b.get(d_bits, "the map").reshape(n, h, rb)
        assert bits.any()
        ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
        for method, k, setting in ((R.GUOHALL, 0, SETTINGS[4]), (R.ZHANGSUEN, 0, SETTINGS[0]), (R.GUOHALL, 1, SETTINGS[3]),
                                   (R.ZHANGSUEN, 2, SETTINGS[1])):
            want, want_info = R.thin(bits, w, method, k)
            d_out, d_info = b.filled(n * h * rb), b.filled(n * 32)
            ctx.set_option("thin_route", setting[0])
            ctx.set_option("thin_fuse", setting[1])
            ctx.dev_canny_thin(n, h, w, method, d_out, d_info, k)
            check_output(b, f"canny_thin method {method} k {k}", d_out, d_info, (n, h, rb), want, want_info, True)
        assert want_info[:, 2].sum() > 0, "the edge map has pixels to delete"
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_thin(n, h + 1, w, R.GUOHALL, d_bits)
        b.free()
    with hip.Context(0) as ctx:   # no canny call yet
        b = _Bufs(ctx)
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_thin(n, h, w, R.GUOHALL, b.filled(n * h * rb))
        b.untouched()
        b.free()


def test_thin_batch_on_host_buffers(hip):
    px = np.concatenate([R.demo_scene()[None], random_maps(2, 96, 160, 5)])
    bits = R.pack_dirty(px, np.random.default_rng(2))
    with hip.Context(0) as ctx:
        for method, k in ((R.GUOHALL, 0), (R.ZHANGSUEN, 0), (R.GUOHALL, 2)):
            want, want_info = R.thin(bits, 160, method, k)
            out, info = ctx.thin_batch(bits, 160, method, k)
            same(out, want, f"thin_batch method {method} k {k}")
            assert info.tolist() == want_info.tolist()
        assert info[0, 1] == 2 and info[0, 3] == 0


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs a larger call, and every data workspace it holds is
    filled with a sentinel before each of three identical runs."""
    big = R.pack(random_maps(4, 129, 577, 3))
    n, h, w = 3, 50, 130
    bits = R.pack_dirty(random_maps(n, h, w, 21))
    with hip.Context(0) as ctx:
        ctx.thin_batch(big, 577, R.GUOHALL, 0)
        b = _Bufs(ctx)
        d_in = b.upload(bits)
        for method, k, setting in ((R.GUOHALL, 0, SETTINGS[4]), (R.ZHANGSUEN, 3, SETTINGS[0]), (R.GUOHALL, 0, SETTINGS[2]),
                                   (R.ZHANGSUEN, 0, SETTINGS[3])):
            want = R.thin(bits, w, method, k)
            runs = []
            for _ in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(thin_and_check(ctx, b, "dirty", bits, w, method, k, setting, d_in=d_in, want=want))
            assert runs[0] == runs[1] == runs[2]
        assert any(name == "thin_ws" and kind == hip.WS_DATA and nbytes for name, _p, nbytes, kind in ctx.selftest_workspaces())
        b.free()


def test_the_refused_calls(hip):
    n, h, w = 2, 20, 30
    rb = 4
    bits = R.pack(random_maps(n, h, w, 40))
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_in = b.upload(bits)
        d_out, d_info = b.filled(n * h * rb), b.filled(n * 32 + 8)
        good = dict(bits=d_in, n=n, h=h, w=w, method=R.GUOHALL, k=0, out=d_out, info=d_info)

        def thin(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_thin_bits(a["bits"], a["n"], a["h"], a["w"], a["method"], a["out"], a["info"], a["k"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(bits=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(method=-1), dict(method=2),
                   dict(k=-1), dict(k=16385), dict(out=d_in), dict(out=d_in + n * h * rb - 1), dict(info=d_info + 4),
                   dict(info=d_in), dict(info=d_out + 8)):
            assert thin(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
            assert thin(**kw) == 2, kw
        for kw in (dict(method=2), dict(k=-1), dict(k=16385)):
            a = dict(good, **kw)
            with pytest.raises(capi.CannyHipError):
                ctx.dev_canny_thin(a["n"], a["h"], a["w"], a["method"], a["out"], a["info"], a["k"])
        for name, value in (("thin_route", 3), ("thin_route", -1), ("thin_fuse", 9), ("thin_fuse", -1)):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option(name, value)
        ctx.synchronize()
        b.untouched()
        assert thin() == 0 and thin(info=0) == 0 and thin(k=16384, method=R.ZHANGSUEN) == 0
        ctx.set_option("thin_route", 2)
        ctx.set_option("thin_fuse", 8)
        assert ctx.get_option("thin_route") == 2 and ctx.get_option("thin_fuse") == 8
        b.get(d_out), b.get(d_info)
        b.free()


def test_the_chain_on_the_device(hip):
    """u8 frame -> dev_binarize FIXED -> dev_thin_bits GUOHALL -> dev_curves_bits with nothing downloaded in between, against
    the rules chained: two curves, where the thick map run straight into the linker gives 3078."""
    scene = R.demo_scene()
    h, w = scene.shape
    rb = (w + 7) // 8
    frame = np.where(scene, 40, 200).astype(np.uint8)[None]
    thick = R.pack(scene[None])
    want_thin, want_info = R.thin(thick, w, R.GUOHALL)
    assert want_info[0].tolist() == [203, 5, 1735 - 203, 1]

    def linked(ctx, b, d_bits, want_map):
        records, off, chain_off, points, point_off = curves_rule.csr(R.unpack(want_map, w), 1)
        cap, pcap = len(records), len(points)
        d_rec, d_off, d_chain = b.filled(cap * 16), b.filled(2 * 8), b.filled((cap + 1) * 8)
        d_points, d_poff = b.filled(pcap * 4), b.filled(2 * 8)
        ctx.dev_curves_bits(d_bits, h, w, 1, 1, d_rec, cap, d_off, d_chain, d_points, pcap, d_poff)
        assert b.get(d_off, "offsets").view(np.uint64).tolist() == off.tolist()
        same(b.get(d_rec, "records").view(np.int32).reshape(cap, 4), records, "records")
        assert b.get(d_chain, "chain offsets").view(np.uint64).tolist() == chain_off.tolist()
        assert b.get(d_points, "points").view(np.int32).tolist() == points.tolist()
        return records

    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_frame, d_bits, d_thin, d_info = b.upload(frame), b.filled(h * rb), b.filled(h * rb), b.filled(32)
        ctx.dev_binarize(d_frame, 1, h, w, capi.BIN_FIXED, 127, d_bits, invert=1)
        ctx.dev_thin_bits(d_bits, 1, h, w, R.GUOHALL, d_thin, d_info)
        records = linked(ctx, b, d_thin, want_thin)
        same(b.get(d_bits, "binarized").reshape(1, h, rb), thick, "binarized")
        same(b.get(d_thin, "thinned").reshape(1, h, rb), want_thin, "thinned")
        assert b.get(d_info, "info").view(np.int64).tolist() == want_info[0].tolist()
        assert sorted((int(r[curves_rule.POINTS]), int(r[curves_rule.FLAGS]) & 1) for r in records) == [(55, 0), (148, 1)]
        assert len(linked(ctx, b, d_bits, thick)) == 3078
        b.free()


def test_the_profile_parts_answer(hip):
    bits = R.pack(R.demo_scene()[None])
    with hip.Context(0) as ctx:
        ctx.profile_enable(1)
        for k in (0, 3):
            ctx.thin_batch(bits, 160, R.GUOHALL, k)
        for part in range(len(capi.THIN_PARTS)):
            ms, launches = ctx.profile_part("thin", part)
            assert launches > 0 and ms > 0.0, capi.THIN_PARTS[part]
        with pytest.raises(capi.CannyHipError):
            ctx.profile_part("thin", 2)
