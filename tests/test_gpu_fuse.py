"""Temporal fusion and change masks on the GPU (canny_hip_dev_fuse_frames, canny_hip_dev_change_mask, canny_hip_canny_background,
canny_hip_selftest_fuse_mean) against tests/fuse_rule.py, byte for byte: every fused, count, mask and
`changed` byte, with sentinel bytes behind each buffer, and optional outputs untouched when they are not asked for."""
import numpy as np
import pytest

import components_rule
import corners_rule as cr
import descriptors_rule as dr
import fuse_rule as fr
import motion_rule as mr
import oracle
import warp_rule as wr
from canny_edge_amd import capi
from fuse_rule import GROUP_LENS, HEIGHTS, VALID, VALUES, WIDTHS, moving_object, valid_bits, values
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
ROUTES = (capi.FUSE_ROUTE_AUTO, capi.FUSE_ROUTE_REGISTERS, capi.FUSE_ROUTE_PASSES)


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
        self.size, self.ptrs = {}, []


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def fuse_and_check(ctx, b, what, n, h, w, d_frames, d_valid, group_len, step, op, fill, min_count, want, with_count=True):
    g = fr.n_groups(n, group_len, step)
    d_fused, d_count = b.filled(g * h * w), b.filled(g * h * w)
    ctx.dev_fuse_frames(d_frames, d_valid, n, h, w, group_len, step, d_fused, d_count if with_count else 0, op, fill, min_count)
    fused = b.get(d_fused, what + ": fused").reshape(g, h, w)
    count = b.get(d_count, what + ": count").reshape(g, h, w)
    same(fused, want[0], what + ": fused")
    if with_count:
        same(count, want[1], what + ": count")
    else:
        assert (count == SENT).all(), what + ": counts written without a buffer"
    return fused.tobytes() + count.tobytes()


def fuse_all_ops(ctx, b, what, frames, bits, group_len, step, fill, min_count, with_count=True, route=0):
    """All four ops of one case; the median under every route, the others under `route`."""
    n, h, w = frames.shape
    d_frames, d_valid = b.upload(frames), (b.upload(bits) if bits is not None else 0)
    for op in fr.OPS:
        want = fr.fuse(frames, bits, group_len, step, op, fill, min_count)
        runs = []
        for r in (ROUTES if op == fr.MEDIAN else (route,)):
            ctx.set_option("fuse_route", r)
            runs.append(fuse_and_check(ctx, b, f"{what} op {op} route {r}", n, h, w, d_frames, d_valid, group_len, step, op, fill,
                                       min_count, want, with_count))
        assert all(r == runs[0] for r in runs)
    ctx.set_option("fuse_route", 0)


@pytest.mark.parametrize("w", WIDTHS)
def test_every_shape(hip, w):
    """Widths and heights one before, on and past the tile, the lane's four pixels and the bit byte's eight; windows that
    slide, skip and tile the stack, with a remainder that belongs to no window; every valid and value pattern in turn."""
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate(HEIGHTS):
            for j, group_len in enumerate((1, 2, 3, 8, 9)):
                k = WIDTHS.index(w) + 5 * i + j
                step = (1, 2, group_len)[k % 3]
                n = group_len + 2 * step + (step > 1)          # three windows; with a step above 1 one frame is left over
                assert (n - group_len) % step == (1 if step > 1 else 0)
                frames = values(VALUES[k % len(VALUES)], n, h, w, k)
                bits = valid_bits(VALID[(k // 2) % len(VALID)], n, h, w, k)
                fuse_all_ops(ctx, b, f"{h} x {w} len {group_len} step {step}", frames, bits, group_len, step, (0, 77)[k % 2],
                             (1, 2, group_len)[(k // 3) % 3], with_count=k % 4 != 3, route=ROUTES[k % 3])
            b.free()


@pytest.mark.parametrize("h,w", [(33, 67), (17, 257)])
def test_every_group_len_straddles_the_register_instantiations(hip, h, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, group_len in enumerate(GROUP_LENS):
            assert hip.fuse_plan("fuse", group_len, h, w, group_len, 1).aux == (1 if group_len <= 32 else 2)
            n = group_len + 1
            frames = values(("random", "ties")[i % 2], n, h, w, 100 + i)
            bits = valid_bits(("half", "null", "sparse")[i % 3], n, h, w, 100 + i)
            fuse_all_ops(ctx, b, f"{h} x {w} len {group_len}", frames, bits, group_len, 1, 77, (1, 2, group_len)[i % 3])
            b.free()


@pytest.mark.parametrize("kind", VALID)
def test_every_valid_pattern_with_every_value_pattern(hip, kind):
    h, w = 17, 67
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, vals in enumerate(VALUES):
            for group_len in (9, 33):
                n = group_len + 3
                fuse_all_ops(ctx, b, f"{kind} {vals} len {group_len}", values(vals, n, h, w, i), valid_bits(kind, n, h, w, i),
                             group_len, (1, 2, group_len)[i % 3], 77 * (i % 2), (1, 2, group_len)[i % 3])
            b.free()


def mask_and_check(ctx, b, what, frames, bits, bg, bc, per, thr, min_count, with_changed=True):
    n, h, w = frames.shape
    rb = fr.row_bytes(w)
    want_mask, want_changed = fr.change_mask(frames, bits, bg, bc, per, thr, min_count)
    d_frames, d_valid = b.upload(frames), (b.upload(bits) if bits is not None else 0)
    d_bg, d_bc = b.upload(bg), (b.upload(bc) if bc is not None else 0)
    d_mask, d_changed = b.filled(n * h * rb), b.filled(n * 8)
    ctx.dev_change_mask(d_frames, d_valid, n, h, w, d_bg, d_bc, per, d_mask, d_changed if with_changed else 0, thr, min_count)
    mask = b.get(d_mask, what + ": mask").reshape(n, h, rb)
    changed = b.get(d_changed, what + ": changed")
    same(mask, want_mask, what + ": mask")
    if with_changed:
        assert changed.view(np.int64).tolist() == want_changed.tolist(), what + ": changed"
    else:
        assert (changed == SENT).all(), what + ": changed written without a buffer"
    return mask.tobytes() + changed.tobytes()


@pytest.mark.parametrize("w", WIDTHS)
def test_change_mask_every_shape(hip, w):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, h in enumerate(HEIGHTS):
            for j, thr in enumerate((0, 1, 49, 254, 255)):
                k = WIDTHS.index(w) + 5 * i + j
                n = 7
                per = (1, 3, 7, 100)[k % 4]
                n_bg = -(-n // per)
                rng = np.random.default_rng(500 + k)
                bg = rng.integers(0, 256, (n_bg, h, w), dtype=np.uint8)
                frames = bg[np.arange(n) // per].copy()
                move = rng.random((n, h, w)) < 0.4                      # differences on both sides of every threshold
                delta = rng.choice(np.array([-255, -254, -50, -49, -2, -1, 1, 2, 49, 50, 254, 255]), (n, h, w))
                frames = np.where(move, np.clip(frames.astype(np.int64) + delta, 0, 255), frames).astype(np.uint8)
                bits = valid_bits(VALID[k % len(VALID)], n, h, w, k)
                bc = rng.integers(0, 4, (n_bg, h, w), dtype=np.uint8) if k % 2 else None
                mask_and_check(ctx, b, f"{h} x {w} thr {thr} per {per}", frames, bits, bg, bc, per, thr, (1, 2, 3)[k % 3],
                               with_changed=k % 5 != 4)
            b.free()


def test_the_mean_helper_of_the_kernels_over_its_whole_domain(hip):
    with hip.Context(0) as ctx:
        got = ctx.selftest_fuse_mean()
    want = fr.mean_table()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of the mean's cells differ, first (c - 1, s) = {bad[0].tolist()}"


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 1 x 1 plane and 4096 workgroups at most: 4097 windows (and 4097 masks) send workgroup 0 through a second
    trip, as the plan query says."""
    for n, group_len in ((4097, 1), (4098, 2)):
        assert hip.fuse_plan("fuse", n - 1, 1, 1, group_len, 1).trips == 1
        plan = hip.fuse_plan("fuse", n, 1, 1, group_len, 1)
        assert (plan.units, plan.grid, plan.per_group, plan.trips) == (4097, 4096, 1, 2)
    assert hip.fuse_plan("mask", 4096, 1, 1).trips == 1 and hip.fuse_plan("mask", 4097, 1, 1).trips == 2
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for n, group_len in ((4097, 1), (4098, 2)):
            frames = values("random", n, 1, 1, n)
            bits = valid_bits("half", n, 1, 1, n)
            fuse_all_ops(ctx, b, f"{n} planes of 1 x 1", frames, bits, group_len, 1, 77, 1)
        frames = values("random", 4097, 1, 1, 3)
        bg = values("random", 4097, 1, 1, 4)
        mask_and_check(ctx, b, "4097 masks", frames, valid_bits("half", 4097, 1, 1, 5), bg, None, 1, 40, 1)
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs the point lists and a fusion of another shape, and
    every data workspace it holds is filled with a sentinel before each of three identical runs."""
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    n, h, w = 12, 50, 130
    frames, bits = values("random", n, h, w, 21), valid_bits("half", n, h, w, 21)
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        b = _Bufs(ctx)
        fuse_all_ops(ctx, b, "another shape", values("ties", 40, 30, 90, 22), None, 33, 7, 0, 1)
        d_frames, d_valid = b.upload(frames), b.upload(bits)
        for op, route in ((fr.MEAN, 0), (fr.MEDIAN, 1), (fr.MEDIAN, 2), (fr.MIN, 0), (fr.MAX, 0)):
            want = fr.fuse(frames, bits, 9, 3, op, 5, 2)
            ctx.set_option("fuse_route", route)
            runs = []
            for _ in range(3):
                for name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(fuse_and_check(ctx, b, "dirty", n, h, w, d_frames, d_valid, 9, 3, op, 5, 2, want))
            assert runs[0] == runs[1] == runs[2]
        bg, bc = fr.fuse(frames, bits, n, n, fr.MEDIAN, 0, 1)
        runs = [mask_and_check(ctx, b, "dirty mask", frames, bits, bg, bc, n, 30, 3) for _ in range(3)]
        assert runs[0] == runs[1] == runs[2]
        b.free()


def test_the_chain_on_one_stream(hip):
    """dev_warp_frames (NEAREST, integer shifts back, valid bits) -> dev_fuse_frames -> dev_change_mask -> dev_components_bits
    with nothing downloaded in between, against the host rules chained."""
    bg, frames, patch = moving_object()
    h, w = bg.shape
    shifts = ((0, 0), (3, -2), (-4, 5))
    src = np.stack([np.roll(f, (-dy, -dx), (0, 1)) for f, (dx, dy) in zip(frames, shifts)])   # src[y, x] = f[y + dy, x + dx]
    recs = np.stack([wr.record(wr.shift(-dx, -dy), k) for k, (dx, dy) in enumerate(shifts)])
    want_frames, want_bits = wr.warp(src, recs, h, w, wr.NEAREST, 0)
    want_bg, want_count = fr.fuse(want_frames, want_bits, 3, 3, fr.MEDIAN, 0, 2)
    want_mask, want_changed = fr.change_mask(want_frames, want_bits, want_bg, want_count, 3, 49, 2)
    masks = fr.unpack_bits(want_mask, w)
    want_labels, want_stats, want_off = components_rule.csr(masks, 1)
    assert want_changed.sum() > 100 and len(want_stats) >= 3
    rb, cap = fr.row_bytes(w), len(want_stats)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_src, d_x = b.upload(src), b.upload(recs)
        d_al, d_valid = b.filled(3 * h * w), b.filled(3 * h * rb)
        d_bg, d_cnt, d_mask, d_changed = b.filled(h * w), b.filled(h * w), b.filled(3 * h * rb), b.filled(3 * 8)
        d_labels, d_stats, d_off = b.filled(3 * h * w * 4), b.filled(cap * 6 * 4), b.filled(4 * 8)
        ctx.dev_warp_frames(d_src, 3, h, w, d_x, 3, h, w, d_al, d_valid, wr.NEAREST, 0)
        ctx.dev_fuse_frames(d_al, d_valid, 3, h, w, 3, 3, d_bg, d_cnt, fr.MEDIAN, 0, 2)
        ctx.dev_change_mask(d_al, d_valid, 3, h, w, d_bg, d_cnt, 3, d_mask, d_changed, 49, 2)
        ctx.dev_components_bits(d_mask, h, w, 3, 1, d_labels, 0, d_stats, cap, d_off)
        same(b.get(d_bg, "the background").reshape(h, w), want_bg[0], "background")
        same(b.get(d_cnt, "the counts").reshape(h, w), want_count[0], "count")
        same(b.get(d_mask, "the masks").reshape(3, h, rb), want_mask, "mask")
        assert b.get(d_changed, "changed").view(np.int64).tolist() == want_changed.tolist()
        assert b.get(d_off, "offsets").view(np.uint64).tolist() == want_off.tolist()
        same(b.get(d_stats, "stats").view(np.int32).reshape(cap, 6), want_stats, "stats")
        same(b.get(d_labels, "labels").view(np.int32).reshape(3, h, w), want_labels, "labels")
        b.free()


def test_canny_background_end_to_end_on_three_frames(hip):
    """Frames A, B, A of tests/test_gpu_warp.py: the background, its counts, the masks and their counts against the host rules
    chained on the oracle's smoothed planes."""
    big = synth_frame(300, 400, 7)
    rng = np.random.default_rng(1)
    noisy = np.clip(big[14:254, 17:337].astype(np.int64) + rng.integers(-4, 5, (240, 320)), 0, 255).astype(np.uint8)
    A = big[10:250, 10:330]
    frames = np.stack([A, noisy, A])
    smoothed = [oracle.gaussian(f, SIGMA) for f in frames]
    corner_args = dict(quality_q16=655, min_dist=8, corners_max=256)
    want_c = [cr.corners(P, **corner_args)[0] for P in smoothed]
    desc = [dr.describe(P, c[:, :2], False)[0] for P, c in zip(smoothed, want_c)]
    want_motion = []
    for fq, ft in ((0, 1), (1, 2)):
        want_m, _ = dr.match(desc[fq], desc[ft], 64, 205, 1)
        want_motion.append(mr.estimate(want_c[fq], len(want_c[fq]), want_c[ft], len(want_c[ft]), want_m, mr.TRANSLATION, 32, 128,
                                       3)[0])
    want_x = wr.compose(np.stack(want_motion), 0)
    al, bits = wr.warp(frames, want_x, 240, 320, wr.BILINEAR, 17)
    with hip.Context(0) as ctx:
        for op, min_count, thr in ((fr.MEDIAN, 2, 2), (fr.MEAN, 3, 1)):   # B's noise is +-4 grey levels: it shows above these
            want_bg, want_count = fr.fuse(al, bits, 3, 3, op, 9, min_count)
            want_mask, want_changed = fr.change_mask(al, bits, want_bg, want_count, 3, thr, min_count)
            bg, mask, changed, count, xf = ctx.canny_background(frames, SIGMA, LO, HI, model=mr.TRANSLATION, thr_q4=32,
                                                                hypotheses=128, seed=3, interp=wr.BILINEAR, border=17, op=op,
                                                                fill=9, min_count=min_count, thr=thr, details=True,
                                                                **corner_args)
            assert xf.view(np.int64).reshape(3, 8).tolist() == want_x.tolist()
            same(bg, want_bg[0], "background")
            same(count, want_count[0], "count")
            same(mask, want_mask, "mask")
            assert changed.tolist() == want_changed.tolist() and 0 < changed[1] < 240 * 320
            plain = ctx.canny_background(frames, SIGMA, LO, HI, model=mr.TRANSLATION, thr_q4=32, hypotheses=128, seed=3,
                                         interp=wr.BILINEAR, border=17, op=op, fill=9, min_count=min_count, thr=thr,
                                         **corner_args)
            assert plain[0].tobytes() == bg.tobytes() and plain[1].tobytes() == mask.tobytes()
        with pytest.raises(capi.CannyHipError):
            ctx.canny_background(np.zeros((256, 16, 16), np.uint8), SIGMA, LO, HI)


def test_the_refused_calls(hip):
    n, h, w = 4, 20, 30
    frames, bits = values("random", n, h, w, 40), valid_bits("half", n, h, w, 40)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_frames, d_valid, d_bg = b.upload(frames), b.upload(bits), b.upload(frames[:2])
        d_fused, d_count = b.filled(2 * h * w), b.filled(2 * h * w)
        d_mask, d_changed = b.filled(n * h * 4), b.filled(n * 8 + 8)
        good = dict(frames=d_frames, valid=d_valid, n=n, h=h, w=w, gl=2, step=2, fused=d_fused, count=d_count, op=1, fill=0, mc=1)

        def fuse(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_fuse_frames(a["frames"], a["valid"], a["n"], a["h"], a["w"], a["gl"], a["step"], a["fused"], a["count"],
                                    a["op"], a["fill"], a["mc"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        mgood = dict(frames=d_frames, valid=d_valid, n=n, h=h, w=w, bg=d_bg, bc=0, per=2, mask=d_mask, changed=d_changed, thr=10,
                     mc=1)

        def mask(**kw):
            a = dict(mgood, **kw)
            try:
                ctx.dev_change_mask(a["frames"], a["valid"], a["n"], a["h"], a["w"], a["bg"], a["bc"], a["per"], a["mask"],
                                    a["changed"], a["thr"], a["mc"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(frames=0), dict(fused=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(gl=0), dict(gl=5),
                   dict(gl=256, n=300), dict(step=0), dict(step=-1), dict(op=-1), dict(op=4), dict(fill=-1), dict(fill=256),
                   dict(mc=0), dict(mc=256), dict(fused=d_frames), dict(fused=d_frames + n * h * w - 1), dict(count=d_frames),
                   dict(fused=d_valid), dict(count=d_valid + 10), dict(count=d_fused + 5)):
            assert fuse(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
            assert fuse(**kw) == 2, kw
        for kw in (dict(frames=0), dict(bg=0), dict(mask=0), dict(n=0), dict(h=0), dict(w=0), dict(per=0), dict(per=-1),
                   dict(thr=-1), dict(thr=256), dict(mc=0), dict(mc=256), dict(changed=d_changed + 4), dict(mask=d_frames + 8),
                   dict(mask=d_valid), dict(mask=d_bg), dict(bc=d_bg, mask=d_bg + 2 * h * w - 1), dict(changed=d_frames),
                   dict(changed=d_mask)):
            assert mask(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536)):
            assert mask(**kw) == 2, kw
        for value in (3, -1):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option("fuse_route", value)
        with pytest.raises(capi.CannyHipError):
            ctx.fuse_profile(2)
        ctx.synchronize()
        b.untouched()
        assert fuse() == 0 and fuse(valid=0, count=0) == 0 and fuse(gl=4, step=1000, fill=255, mc=255) == 0
        assert mask() == 0 and mask(valid=0, changed=0, bc=d_bg) == 0 and mask(per=1000, bg=d_bg, thr=255) == 0
        ctx.set_option("fuse_route", 2)
        assert ctx.get_option("fuse_route") == 2
        b.get(d_fused), b.get(d_count), b.get(d_mask), b.get(d_changed)
        b.free()
