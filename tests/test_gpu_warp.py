"""Frame alignment on the GPU (canny_hip_dev_compose_motion, canny_hip_dev_warp_frames, canny_hip_canny_align; DESIGN.md section
32) against tests/warp_rule.py, byte for byte: every output byte and every valid byte, with sentinel bytes behind each buffer."""
import numpy as np
import pytest

import corners_rule as cr
import descriptors_rule as dr
import motion_rule as mr
import oracle
import warp_rule as wr
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
ONE = wr.ONE
BOTH = (wr.NEAREST, wr.BILINEAR)
ROUTES = (capi.WARP_ROUTE_AUTO, capi.WARP_ROUTE_DIRECT, capi.WARP_ROUTE_TILED)
WIDTHS = (1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 67, 257)
HEIGHTS = (1, 2, 15, 16, 17, 33)


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard bytes behind each, and plain uploads."""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptrs = ctx, {}, []

    def filled(self, nbytes):
        p = self.ctx.malloc(nbytes + N_GUARD)
        self.ptrs.append(p)
        self.size[p] = nbytes
        self.refill(p)
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def refill(self, p):
        self.ctx.h2d(p, np.full(self.size[p] + N_GUARD, SENT, np.uint8))

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


def planes(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def warp_and_check(ctx, b, name, src, xforms, out_h, out_w, interp, border, want, d_src=None, d_x=None, valid=True):
    """One warp call on uploaded planes and records against `want` = wr.warp(...).  Returns the outputs' bytes."""
    n_src, sh, sw = src.shape
    xforms = np.asarray(xforms, np.int64).reshape(-1, 8)
    n_out, rb = len(xforms), (out_w + 7) // 8
    d_src = b.upload(src) if d_src is None else d_src
    d_x = b.upload(xforms) if d_x is None else d_x
    d_out, d_valid = b.filled(n_out * out_h * out_w), b.filled(n_out * out_h * rb)
    ctx.dev_warp_frames(d_src, n_src, sh, sw, d_x, n_out, out_h, out_w, d_out, d_valid if valid else 0, interp, border)
    got = b.get(d_out, "the frames").reshape(n_out, out_h, out_w)
    bits = b.get(d_valid, "the valid bits").reshape(n_out, out_h, rb)
    for o in range(n_out):
        bad = np.argwhere(got[o] != want[0][o])
        assert bad.size == 0, (f"{name} interp {interp}: frame {o} {xforms[o].tolist()}: {len(bad)} bytes differ, first at "
                               f"(y, x) = {bad[0].tolist()}: {got[o][tuple(bad[0])]} != {want[0][o][tuple(bad[0])]}")
        if valid:
            bad = np.argwhere(bits[o] != want[1][o])
            assert bad.size == 0, f"{name} interp {interp}: frame {o} {xforms[o].tolist()}: valid bytes differ, first {bad[0].tolist()}"
    if not valid:
        assert (bits == SENT).all(), f"{name}: valid bits written without a buffer"
    return got.tobytes() + bits.tobytes()


def transforms(out_h, out_w, sh, sw):
    """The list of tests/test_warp_rule.py for one shape, plus a 1 degree turn with scale 1.01 about the centre, a shear and a
    negative determinant; every record reads source plane 1 of 2 unless it says otherwise."""
    A, T = wr.LIM_A, wr.LIM_T
    coefs = [wr.IDENTITY, wr.shift(3, -2), wr.shift(-5, 1), wr.quarter_turn(out_w), (-ONE, 0, (out_w - 1) * ONE, 0, ONE, 0),
             (2 * ONE, 0, 0, 0, 2 * ONE, 0), (ONE, 0, 32768, 0, ONE, 0), (ONE, 0, -1, 0, ONE, -1),
             (ONE, 0, -129, 0, ONE, -129), wr.shift(-sw + 1.5, 0.25), wr.shift(sw - 2.25, -0.5), wr.shift(0.75, -sh + 1.5),
             wr.shift(-0.5, sh - 1.25), wr.shift(-sw - 70, 0), wr.shift(0, sh + 20), (A, 0, 0, 0, A, 0), (-A, A, T, A, -A, -T),
             (ONE, 0, T, 0, ONE, -T), wr.small_turn(out_w, out_h), (ONE, 3 * ONE // 4, -2 * ONE, ONE // 8, ONE, 0),
             (ONE // 2, ONE, 0, ONE, ONE // 3, -ONE), (0, -ONE, (sw - 1) * ONE, ONE, 0, 0),
             (-ONE, 0, (sw - 1) * ONE, 0, -ONE, (sh - 1) * ONE), (ONE // 3, 0, 0, 0, ONE // 5, 0)]
    recs = [wr.record(c, 1) for c in coefs]
    recs += [wr.record((A + 1, 0, 0, 0, ONE, 0), 1), wr.record((ONE, 0, 0, 0, ONE, T + 1), 1), wr.record(wr.IDENTITY, 2),
             wr.record(wr.IDENTITY, -1), wr.record(wr.IDENTITY, 0, flags=2), wr.record(wr.shift(1, 1), 0, flags=3)]
    return np.stack(recs)


@pytest.mark.parametrize("interp", BOTH)
def test_every_shape_every_transform_every_route(hip, interp):
    """Output widths and heights one before, on and past the tile, the lane's four pixels and the valid byte's eight; sources of
    the output's size, larger and smaller; all three routes against one reference."""
    with hip.Context(0) as ctx:
        for i, out_w in enumerate(WIDTHS):
            b = _Bufs(ctx)
            for j, out_h in enumerate(HEIGHTS):
                sh, sw = ((out_h, out_w), (out_h + 2, out_w + 3), (29, 41))[(i + j) % 3]
                src = planes(2, sh, sw, 100 * i + j)
                x = transforms(out_h, out_w, sh, sw)
                want = wr.warp(src, x, out_h, out_w, interp, 77)
                d_src, d_x = b.upload(src), b.upload(x)
                runs = []
                for route in ROUTES:
                    ctx.set_option("warp_route", route)
                    runs.append(warp_and_check(ctx, b, f"{out_h} x {out_w} from {sh} x {sw} route {route}", src, x, out_h,
                                               out_w, interp, 77, want, d_src, d_x))
                assert runs[0] == runs[1] == runs[2]
            b.free()


@pytest.mark.parametrize("interp", BOTH)
def test_one_frame_with_staged_and_unstaged_tiles(hip, interp):
    """The case of tests/test_warp_launch_plan.py: under scale 8 the full tile's footprint exceeds the LDS budget and gathers
    directly while the three-pixel tile beside it is staged -- proved through the plan query first."""
    x = wr.record((8 * ONE, 0, 0, 0, 8 * ONE, 0))
    wide, narrow = hip.warp_tile(x, 200, 600, 16, 67, interp, 0, 0), hip.warp_tile(x, 200, 600, 16, 67, interp, 1, 0)
    assert not wide.staged and wide.x1 - wide.x0 > 500 and narrow.staged
    src = planes(1, 200, 600, 7)
    recs = np.stack([x, wr.record((8 * ONE, ONE, -3 * ONE, ONE // 2, 7 * ONE, 5 * ONE)), wr.record(wr.shift(530, 180))])
    want = wr.warp(src, recs, 16, 67, interp, 3)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        runs = []
        for route in ROUTES:
            ctx.set_option("warp_route", route)
            runs.append(warp_and_check(ctx, b, f"scale 8 route {route}", src, recs, 16, 67, interp, 3, want))
        assert runs[0] == runs[1] == runs[2]
        b.free()


@pytest.mark.parametrize("route", ROUTES)
def test_permuted_and_repeated_sources_an_unusable_record_and_no_valid_buffer(hip, route):
    """Six outputs from three sources with permuted and repeated indices, an unusable record in the middle of the batch; the
    same call without the valid buffer writes the same frames and nothing else."""
    src = planes(3, 45, 70, 8)
    recs = np.stack([wr.record(wr.shift(1.5, 0.5), 2), wr.record(wr.IDENTITY, 0), wr.record(wr.small_turn(70, 45), 2),
                     wr.record(wr.IDENTITY, 1, flags=0), wr.record(wr.quarter_turn(70), 1), wr.record(wr.shift(-3, 2), 0)])
    with hip.Context(0) as ctx:
        ctx.set_option("warp_route", route)
        b = _Bufs(ctx)
        for interp in BOTH:
            want = wr.warp(src, recs, 45, 70, interp, 200)
            assert (want[0][3] == 200).all() and not want[1][3].any() and np.array_equal(want[0][1], src[0])
            a = warp_and_check(ctx, b, "six from three", src, recs, 45, 70, interp, 200, want)
            c = warp_and_check(ctx, b, "six from three, no valid", src, recs, 45, 70, interp, 200, want, valid=False)
            assert a[:6 * 45 * 70] == c[:6 * 45 * 70]
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One 64 x 16 tile per frame and 4096 workgroups at most: 4097 frames send workgroup 0 through a second trip, as the plan
    query says."""
    n = 4097
    assert hip.warp_plan(n - 1, 16, 64).trips == 1
    plan = hip.warp_plan(n, 16, 64)
    assert (plan.units, plan.grid, plan.per_group, plan.trips) == (n, 4096, 1, 2)
    src = planes(3, 20, 70, 9)
    kinds = np.stack([wr.record(c, s) for s in range(3) for c in (wr.IDENTITY, wr.shift(2.5, 1.25), wr.quarter_turn(64),
                                                                 wr.small_turn(64, 16), wr.shift(-80, 0))] +
                     [wr.record(wr.IDENTITY, 3)])
    which = np.random.default_rng(10).integers(0, len(kinds), n)
    which[[0, 4095, 4096]] = (3, 7, 12)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_src, d_x = b.upload(src), b.upload(kinds[which])
        for interp, route in ((wr.BILINEAR, capi.WARP_ROUTE_TILED), (wr.NEAREST, capi.WARP_ROUTE_DIRECT)):
            frames, bits = wr.warp(src, kinds, 16, 64, interp, 5)
            ctx.set_option("warp_route", route)
            warp_and_check(ctx, b, "past the cap", src, kinds[which], 16, 64, interp, 5, (frames[which], bits[which]), d_src, d_x)
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs the point lists and a warp of another shape, and
    every data workspace it holds is filled with a sentinel before each of three identical runs."""
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    src = planes(2, 50, 130, 11)
    recs = np.stack([wr.record(wr.small_turn(130, 50), 1), wr.record(wr.quarter_turn(130), 0), wr.record(wr.shift(0.3, 0.7), 1)])
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        b = _Bufs(ctx)
        big = planes(1, 100, 300, 12)
        warp_and_check(ctx, b, "another shape", big, wr.record(wr.shift(4, 4)), 100, 300, wr.BILINEAR, 0,
                       wr.warp(big, wr.record(wr.shift(4, 4)), 100, 300, wr.BILINEAR, 0))
        d_src, d_x = b.upload(src), b.upload(recs)
        for interp in BOTH:
            want = wr.warp(src, recs, 50, 130, interp, 9)
            for route in ROUTES:
                ctx.set_option("warp_route", route)
                runs = []
                for _ in range(3):
                    for name, ptr, nbytes, kind in ctx.selftest_workspaces():
                        if kind == hip.WS_DATA and ptr and nbytes:   # index and cache words only hold the library's own
                            ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                    runs.append(warp_and_check(ctx, b, "dirty", src, recs, 50, 130, interp, 9, want, d_src, d_x))
                assert runs[0] == runs[1] == runs[2]
        b.free()


def random_motion(rng, n, breaks=()):
    m = np.zeros((n, 16), np.int64)
    m[:, 0] = 3
    m[:, 1:4] = rng.integers(0, 100, (n, 3))
    turn = rng.random(n) * 0.2 - 0.1
    scale = 1 + (rng.random(n) - 0.5) * 0.05
    m[:, 4], m[:, 5] = np.round(np.cos(turn) * scale * ONE), np.round(-np.sin(turn) * scale * ONE)
    m[:, 7], m[:, 8] = -m[:, 5], m[:, 4]
    m[:, [6, 9]] = rng.integers(-40 * ONE, 40 * ONE, (n, 2))
    m[:, 10:] = rng.integers(0, 1000, (n, 6))
    for k, how in breaks:
        if how == "refit":
            m[k, 0] = 1
        elif how == "model":
            m[k, 0] = 2
        elif how == "a":
            m[k, 5] = -wr.LIM_A - 1
        else:
            m[k, 9] = wr.LIM_T + 1
    return m


@pytest.mark.parametrize("n,breaks", [(1, ()), (1, ((0, "refit"),)), (2, ()), (2, ((1, "a"),)), (64, ()), (64, ((63, "t"),)),
                                      (65, ((64, "model"),)), (65, ()), (300, ()), (300, ((150, "refit"), (200, "a")))])
def test_compose_on_the_device(hip, n, breaks):
    rng = np.random.default_rng(1000 + n + len(breaks))
    motion = random_motion(rng, n, breaks)
    want = wr.compose(motion, 5)
    assert want[:, 0].sum() == (min(k for k, _ in breaks) + 1 if breaks else n + 1)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_m, d_x = b.upload(motion), b.filled((n + 1) * 64)
        ctx.dev_compose_motion(d_m, n, 5, d_x)
        got = b.get(d_x, "the transform records").view(np.int64).reshape(n + 1, 8)
        assert got.tolist() == want.tolist()
        b.free()


def test_compose_takes_the_motion_records_as_the_estimate_leaves_them_and_the_warp_takes_the_chain(hip):
    """dev_estimate_motion -> dev_compose_motion -> dev_warp_frames on one stream with nothing downloaded in between; the
    records are brought down afterwards and the rules chained on them."""
    rng = np.random.default_rng(13)
    n = 5
    sets, rows = [], []
    pts = np.zeros((60, 4), np.int64)
    pts[:, :2] = rng.integers(20, 180, (60, 2))
    for f in range(n):
        s = pts.copy()
        s[:, 0] += 3 * f
        s[:, 1] -= 2 * f
        sets.append(s)
    for f in range(n - 1):
        row = np.zeros((60, 4), np.int32)
        row[:, 0], row[:, 3] = np.arange(60), 15
        if f == 2:
            row[:, 3] = 0                                   # no accepted match: no model, the chain breaks here
        rows.append(row)
    rec = np.stack(sets)
    counts = np.full(n, 60, np.int32)
    src = planes(n, 64, 200, 14)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_r, d_c, d_m = b.upload(rec), b.upload(counts), b.upload(np.stack(rows))
        d_motion, d_x, d_src = b.filled((n - 1) * 128), b.filled(n * 64), b.upload(src)
        d_out, d_valid = b.filled(n * 64 * 200), b.filled(n * 64 * 25)
        ctx.dev_estimate_motion(d_r, d_c, n, 60, d_r, d_c, n, 60, capi.consecutive_pairs(n), d_m, d_motion, 0,
                                capi.MOTION_TRANSLATION, 16, 8, 1)
        ctx.dev_compose_motion(d_motion, n - 1, 0, d_x)
        ctx.dev_warp_frames(d_src, n, 64, 200, d_x, n, 64, 200, d_out, d_valid, wr.BILINEAR, 50)
        motion = b.get(d_motion, "the motion records").view(np.int64).reshape(n - 1, 16)
        got = b.get(d_x, "the transform records").view(np.int64).reshape(n, 8)
        assert motion[:, 0].tolist() == [3, 3, 0, 3] and motion[0, 4:10].tolist() == [ONE, 0, 3 * ONE, 0, ONE, -2 * ONE]
        want = wr.compose(motion, 0)
        assert got.tolist() == want.tolist() and want[:, 0].tolist() == [1, 1, 1, 0, 0]
        assert want[2, 2:].tolist() == [ONE, 0, 6 * ONE, 0, ONE, -4 * ONE]
        frames, bits = wr.warp(src, want, 64, 200, wr.BILINEAR, 50)
        assert np.array_equal(b.get(d_out, "the frames").reshape(n, 64, 200), frames)
        assert np.array_equal(b.get(d_valid, "the valid bits").reshape(n, 64, 25), bits)
        assert (frames[3:] == 50).all() and np.array_equal(frames[1, 2:, :197], src[1, :62, 3:])
        b.free()


def test_the_refused_calls(hip):
    src = planes(2, 20, 30, 15)
    recs = np.stack([wr.record(wr.IDENTITY, 1)] * 2)
    motion = random_motion(np.random.default_rng(16), 3)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_src, d_x, d_m = b.upload(src), b.upload(np.concatenate([recs.ravel(), [0]])), b.upload(motion)
        d_out, d_valid, d_chain = b.filled(2 * 20 * 30), b.filled(2 * 20 * 4), b.filled(4 * 64 + 8)
        good = dict(src=d_src, n_src=2, sh=20, sw=30, x=d_x, n_out=2, oh=20, ow=30, out=d_out, valid=d_valid, interp=1, border=0)

        def status(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_warp_frames(a["src"], a["n_src"], a["sh"], a["sw"], a["x"], a["n_out"], a["oh"], a["ow"], a["out"],
                                    a["valid"], a["interp"], a["border"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        def chain_status(m=d_m, n=3, first=0, x=d_chain):
            try:
                ctx.dev_compose_motion(m, n, first, x)
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(src=0), dict(x=0), dict(out=0), dict(n_src=0), dict(n_out=0), dict(sh=0), dict(sw=0), dict(oh=0),
                   dict(ow=0), dict(n_src=-1), dict(n_out=-2), dict(interp=2), dict(interp=-1), dict(border=-1),
                   dict(border=256), dict(x=d_x + 4), dict(out=d_src), dict(out=d_src + 599), dict(out=d_src + 1199, n_out=1),
                   dict(valid=d_src + 10), dict(valid=d_out + 1199)):
            assert status(**kw) == 1, kw
        for kw in (dict(sh=32769), dict(sw=32769), dict(oh=32769), dict(ow=32769), dict(n_src=65536), dict(n_out=65536)):
            assert status(**kw) == 2, kw
        for kw in (dict(m=0), dict(x=0), dict(n=-1), dict(first=-1), dict(m=d_m + 4), dict(x=d_chain + 4)):
            assert chain_status(**kw) == 1, kw
        assert chain_status(n=65536) == 2
        for name, value in (("warp_route", 3), ("warp_route", -1)):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option(name, value)
        ctx.synchronize()
        b.untouched()
        assert status() == 0 and status(valid=0) == 0 and status(border=255, interp=0) == 0
        assert chain_status() == 0 and chain_status(m=0, n=0) == 0
        ctx.set_option("warp_route", 2)
        assert ctx.get_option("warp_route") == 2
        b.get(d_out), b.get(d_valid), b.get(d_chain)
        b.free()


def test_canny_align_end_to_end_on_three_frames(hip):
    """Views A, B, A of the descriptor tests' scene (240 x 320, B shifted by (-7, -4) with noise) as a three-frame batch: the
    motion records, the chain and the aligned frames against the host rules chained on the oracle's smoothed planes.  The
    third frame comes back onto the first: its transform is the first pair's shift undone by the second's."""
    big = synth_frame(300, 400, 7)
    rng = np.random.default_rng(1)
    noisy = np.clip(big[14:254, 17:337].astype(np.int64) + rng.integers(-4, 5, (240, 320)), 0, 255).astype(np.uint8)
    A = big[10:250, 10:330]
    frames = np.stack([A, noisy, A])
    smoothed = [oracle.gaussian(f, SIGMA) for f in frames]
    corner_args = dict(quality_q16=655, min_dist=8, corners_max=256)
    want_c = [cr.corners(P, **corner_args)[0] for P in smoothed]
    for steered, model, interp in ((False, mr.TRANSLATION, wr.BILINEAR), (True, mr.SIMILARITY, wr.NEAREST)):
        desc = [dr.describe(P, c[:, :2], steered)[0] for P, c in zip(smoothed, want_c)]
        want_motion = []
        for fq, ft in ((0, 1), (1, 2)):
            want_m, _ = dr.match(desc[fq], desc[ft], 64, 205, 1)
            want_motion.append(mr.estimate(want_c[fq], len(want_c[fq]), want_c[ft], len(want_c[ft]), want_m, model, 32, 128,
                                           3)[0])
        want_x = wr.compose(np.stack(want_motion), 0)
        want_frames, want_bits = wr.warp(frames, want_x, 240, 320, interp, 17)
        with hip.Context(0) as ctx:
            aligned, xf, motion, valid = ctx.canny_align(frames, SIGMA, LO, HI, steered=steered, model=model, thr_q4=32,
                                                         hypotheses=128, seed=3, interp=interp, border=17, details=True,
                                                         **corner_args)
            plain, plain_xf = ctx.canny_align(frames, SIGMA, LO, HI, steered=steered, model=model, thr_q4=32, hypotheses=128,
                                              seed=3, interp=interp, border=17, **corner_args)
            one, one_xf = ctx.canny_align(frames[1:2], SIGMA, LO, HI, interp=interp, border=17, **corner_args)
        assert motion.view(np.int64).reshape(2, 16).tolist() == np.stack(want_motion).tolist()
        assert xf.view(np.int64).reshape(3, 8).tolist() == want_x.tolist() and want_x[:, 0].tolist() == [1, 1, 1]
        assert np.array_equal(aligned, want_frames) and np.array_equal(valid, want_bits)
        assert plain.tobytes() == aligned.tobytes() and plain_xf.tobytes() == xf.tobytes()
        assert np.array_equal(one[0], frames[1]) and one_xf.view(np.int64).tolist() == [1, 0, ONE, 0, 0, 0, ONE, 0]
        assert np.array_equal(aligned[0], A)
        assert abs(xf[1]["tx"] / ONE + 7) < 2.5 and abs(xf[1]["ty"] / ONE + 4) < 2.5
        assert abs(xf[2]["tx"] / ONE) < 2.5 and abs(xf[2]["ty"] / ONE) < 2.5
        ok = wr.unpack_valid(valid, 320)
        err = np.abs(aligned[1].astype(int) - A.astype(int))[ok[1]].mean()
        raw = np.abs(noisy.astype(int) - A.astype(int))[ok[1]].mean()
        assert err < raw / 4, (err, raw)
