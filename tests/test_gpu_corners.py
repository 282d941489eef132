"""Corners on the GPU (canny_hip_dev_canny_corners, canny_hip_dev_corners_plane, canny_hip_canny_corners,
canny_hip_dev_corners_arith) against tests/corners_rule.py applied to the oracle's smoothed plane or to
the plane the call is given.  Every comparison is exact equality on whole arrays; every output buffer is sentinel-filled
with guard words behind it."""
import os
import subprocess

import numpy as np
import pytest

import corners_rule as cr
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
SIGMA, LO, HI = 1.4, 50, 150
MODES = [(cr.MIN_EIGEN, 0), (cr.HARRIS, 10)]
TILE_Y, TILE_X = 16, 64


class _Call:
    """The sentinel-filled outputs of one corners call on n frames, with guard words behind each, and their check."""

    def __init__(self, ctx, n, h, w, corners_max, response=False, cands=True, rmax=True, edges=False):
        self.ctx, self.n, self.h, self.w, self.cmax = ctx, n, h, w, corners_max
        self.words, self.ptrs = {}, []
        self.d_rec = self._filled(8 * n * corners_max)
        self.d_cnt = self._filled(n)
        self.d_cand = self._filled(n) if cands else 0
        self.d_max = self._filled(2 * n) if rmax else 0
        self.d_resp = self._filled(2 * n * h * w) if response else 0
        self.d_edges = self._filled((n * h * w + 1) // 2) if edges else 0

    def _filled(self, words):
        p = self.ctx.malloc(4 * (words + N_GUARD))
        self.ptrs.append(p)
        self.words[p] = words
        self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.ctx.h2d(p, a)
        return p

    def refill(self):
        for p, words in self.words.items():
            self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))

    def get(self, p, what=""):
        out = np.empty(self.words[p] + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[self.words[p]:] == SENT).all(), f"guard words overwritten behind {what}"
        return out[:self.words[p]]

    def tail(self, mode, block, k_q8, quality_q16, min_response, min_dist):
        """The arguments of the device forms from `mode` on."""
        return (mode, block, k_q8, quality_q16, min_response, min_dist, self.cmax, self.d_rec, self.d_cnt, self.d_cand,
                self.d_max, self.d_resp)

    def untouched(self):
        for p in self.words:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def raw(self):
        """Every output's bytes, for comparing runs with each other."""
        return b"".join(self.get(p).tobytes() for p in self.words)

    def check(self, want, what=""):
        """want: per frame (records, candidate count, Rmax, R) of the rule.  Returns the number of corners."""
        n, cmax = self.n, self.cmax
        rec = self.get(self.d_rec, "the records").view(np.int64).reshape(n, cmax, 4)
        cnt = self.get(self.d_cnt, "the counts").view(np.int32)
        assert cnt.tolist() == [len(r) for r, _, _, _ in want], f"{what}: counts {cnt.tolist()}"
        for f, (r, _, _, _) in enumerate(want):
            assert np.array_equal(rec[f, :len(r)], r), f"{what}: frame {f}: records differ"
            assert (rec[f, len(r):].view(np.uint32) == SENT).all(), f"{what}: frame {f}: slots past the count were written"
        if self.d_cand:
            assert self.get(self.d_cand, "cand_counts").view(np.int32).tolist() == [k for _, k, _, _ in want], what
        if self.d_max:
            assert self.get(self.d_max, "max_response").view(np.int64).tolist() == [m for _, _, m, _ in want], what
        if self.d_resp:
            resp = self.get(self.d_resp, "the responses").view(np.int64).reshape(n, self.h, self.w)
            for f, (_, _, _, R) in enumerate(want):
                bad = np.argwhere(resp[f] != R)
                assert bad.size == 0, f"{what}: frame {f}: {len(bad)} responses differ, first at {bad[0]}"
        return int(cnt.sum())

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def want_of(planes, mode, block, k_q8, quality_q16, min_response, min_dist, corners_max):
    return [cr.corners(P, mode, block, k_q8, quality_q16, min_response, min_dist, corners_max) for P in planes]


_REF = {}


def reference(h, w):
    """(frames, maps, the oracle's smoothed planes) of three frames of a shape -- for 70 x 77 the middle one is flat (its
    smoothed plane is flat but for the Gaussian's border rows and columns); computed once, never modified."""
    if (h, w) not in _REF:
        frames = np.stack([synth_frame(h, w, s) for s in (1, 2, 3)])
        if w == 77:
            frames[1] = 90
        maps = np.stack([oracle.canny(f, SIGMA, LO, HI) for f in frames])
        planes = np.stack([oracle.gaussian(f, SIGMA) for f in frames])
        assert planes.min() >= 0 and planes.max() <= 255
        for a in (frames, maps, planes):
            a.setflags(write=False)
        _REF[(h, w)] = (frames, maps, planes)
    return _REF[(h, w)]


_WANT = {}


def reference_corners(h, w, mode, block, k_q8):
    key = (h, w, mode, block, k_q8)
    if key not in _WANT:
        _WANT[key] = want_of(reference(h, w)[2], mode, block, k_q8, 2000, 0, 6, 40)
    return _WANT[key]


# ---- routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("h,w", [(70, 128), (70, 77)], ids=["70x128", "70x77"])
def test_behind_dev_canny_equals_the_rule_on_the_oracles_planes(hip, h, w, u8, fuse, tail):
    frames, maps, planes = reference(h, w)
    with hip.Context(0) as ctx:
        ctx.set_option("smoothed_u8", u8)
        ctx.set_option("fuse_classify", fuse)
        ctx.set_option("hysteresis_tail", tail)
        c = _Call(ctx, 3, h, w, 40, response=True, edges=True)
        d_img = c.upload(frames)
        d_plain = c.upload(np.zeros((3, h, w), np.int16))
        ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, 3, d_plain)
        plain = np.empty((3, h, w), np.int16)
        ctx.d2h(plain, d_plain)
        assert np.array_equal(plain, maps)
        total = 0
        for mode, k_q8 in MODES:
            for block in (3, 5, 7):
                c.refill()
                ctx.dev_canny_corners(d_img, SIGMA, LO, HI, h, w, 3, *c.tail(mode, block, k_q8, 2000, 0, 6), d_edges=c.d_edges)
                # the byte plane exists only between the two marching kernels of the fused route (width % 8 == 0)
                assert ctx.get_option("last_canny_smoothed_u8") == (1 if u8 and fuse and w % 8 == 0 else 0)
                want = reference_corners(h, w, mode, block, k_q8)
                total += c.check(want, f"mode {mode} block {block}")
                edges = c.get(c.d_edges, "d_edges").view(np.int16)[:3 * h * w].reshape(3, h, w)
                assert np.array_equal(edges, plain), "d_edges differs from dev_canny's"
        assert total > 50
        c.free()


def test_max_val_above_255_empties_the_map_but_not_the_corners(hip):
    h, w = 70, 128
    frames, _, _ = reference(h, w)
    with hip.Context(0) as ctx:
        c = _Call(ctx, 3, h, w, 40, edges=True)
        ctx.dev_canny_corners(c.upload(frames), SIGMA, LO, 300, h, w, 3, *c.tail(0, 5, 0, 2000, 0, 6), d_edges=c.d_edges)
        assert c.check(reference_corners(h, w, 0, 5, 0), "max_val 300") > 20
        assert not c.get(c.d_edges).view(np.int16)[:3 * h * w].any()
        c.free()


# ---- tile seams ----------------------------------------------------------------------------------------------------------
def seam_planes(h, w, seed):
    """Three planes of a shape: bright blocks whose corners lie on the seams of the 64 x 16 tiles and in the frame's four
    corners, the same with noise, and a flat plane (no candidate, Rmax = 0)."""
    rng = np.random.default_rng(seed)
    P = np.zeros((h, w), np.uint8)
    for y0 in range(0, h, TILE_Y):
        for x0 in range(0, w, TILE_X):
            P[max(y0 - 3, 0):y0 + 1, max(x0 - 5, 0):x0 + 1] = 180 + ((y0 + x0) // 16) % 7 * 10   # ends ON the seam
            P[y0 + 4:y0 + 7, x0 + 9:x0 + 12] = 120
    P[:2, :2] = P[:2, -2:] = P[-2:, :2] = P[-2:, -2:] = 255
    Q = np.clip(P.astype(np.int64) + rng.integers(0, 40, (h, w)), 0, 255).astype(np.uint8)
    return np.stack([P, Q, np.full((h, w), 77, np.uint8)])


SEAM_SHAPES = [(2, 2), (15, 63), (16, 64), (17, 65), (16, 65), (17, 64), (15, 129), (33, 63), (49, 130)]


@pytest.mark.parametrize("h,w", SEAM_SHAPES, ids=[f"{h}x{w}" for h, w in SEAM_SHAPES])
def test_tile_seams_and_frame_corners(hip, h, w):
    planes = seam_planes(h, w, h * 1000 + w)
    with hip.Context(0) as ctx:
        c = _Call(ctx, 3, h, w, 64, response=True)
        d_plane = c.upload(planes)
        total = 0
        for mode, k_q8 in MODES:
            for block in (3, 5, 7):
                c.refill()
                ctx.dev_corners_plane(d_plane, 3, h, w, *c.tail(mode, block, k_q8, 300, 0, 2))
                want = want_of(planes, mode, block, k_q8, 300, 0, 2, 64)
                assert (len(want[2][0]), want[2][1], want[2][2]) == (0, 0, 0), "the flat plane has no corner"
                total += c.check(want, f"mode {mode} block {block}")
        assert total > 50 or h == 2
        c.free()


# ---- the designed cases ----------------------------------------------------------------------------------------------------
def test_the_square_and_the_checkerboard_with_the_cut_in_a_tie_group(hip):
    planes = np.stack([cr.square_plane(), cr.checkerboard_plane()])
    with hip.Context(0) as ctx:
        d_plane = None
        for mode, k_q8 in MODES:
            for cmax in (50, 98, 99, 150):
                c = _Call(ctx, 2, 64, 64, cmax)
                d_plane = c.upload(planes)
                for md in (0, 6, 9):
                    c.refill()
                    ctx.dev_corners_plane(d_plane, 2, 64, 64, *c.tail(mode, 5, k_q8, 655, 0, md))
                    want = want_of(planes, mode, 5, k_q8, 655, 0, md, cmax)
                    assert want[0][1] == 4 and want[1][1] == 196
                    c.check(want, f"mode {mode} corners_max {cmax} min_dist {md}")
                c.free()
            for block in (3, 7):
                c = _Call(ctx, 2, 64, 64, 256, response=True)
                ctx.dev_corners_plane(c.upload(planes), 2, 64, 64, *c.tail(mode, block, k_q8, 655, 0, 0))
                want = want_of(planes, mode, block, k_q8, 655, 0, 0, 256)
                assert len(want[0][0]) == 4
                c.check(want, f"mode {mode} block {block}")
                c.free()


# ---- capacities, optional outputs ---------------------------------------------------------------------------------------
def test_capacities_and_null_outputs(hip):
    h, w = 70, 128
    _, _, planes = reference(h, w)
    planes = planes.astype(np.uint8)
    full = want_of(planes, 0, 3, 0, 1000, 0, 0, 4096)
    exact = max(k for _, k, _, _ in full)
    assert exact > 10
    with hip.Context(0) as ctx:
        raw = {}
        for cmax in (1, exact, exact - 1, 4096):
            want = want_of(planes, 0, 3, 0, 1000, 0, 0, cmax)
            for response in (False, True):
                c = _Call(ctx, 3, h, w, cmax, response=response)
                ctx.dev_corners_plane(c.upload(planes), 3, h, w, *c.tail(0, 3, 0, 1000, 0, 0))
                c.check(want, f"corners_max {cmax} response {response}")
                raw[(cmax, response)] = b"".join(c.get(p).tobytes() for p in (c.d_rec, c.d_cnt, c.d_cand, c.d_max))
                c.free()
            assert raw[(cmax, False)] == raw[(cmax, True)], "the outputs depend on d_response"
            # without the optional outputs: the same records and counts
            c = _Call(ctx, 3, h, w, cmax, cands=False, rmax=False)
            ctx.dev_corners_plane(c.upload(planes), 3, h, w, *c.tail(0, 3, 0, 1000, 0, 0))
            c.check(want, f"corners_max {cmax}, no optional output")
            c.free()
        # an absolute floor above every response: nothing, and the maxima are still reported
        c = _Call(ctx, 3, h, w, 8)
        ctx.dev_corners_plane(c.upload(planes), 3, h, w, *c.tail(0, 3, 0, 65536, 1 << 40, 0))
        want = want_of(planes, 0, 3, 0, 65536, 1 << 40, 0, 8)
        assert [k for _, k, _, _ in want] == [0, 0, 0]
        c.check(want, "min_response above the maximum")
        c.free()


# ---- one context, many calls ----------------------------------------------------------------------------------------------
def test_three_identical_runs_on_a_dirty_context(hip):
    """The dirty-workspace discipline of DESIGN.md section 20: no call may read what an earlier call left.  The context
    first runs the point lists, the circles, the chamfer matching and a corner call on another shape."""
    h, w = 70, 128
    frames, _, _ = reference(h, w)
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9, 10, 11)])
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        ctx.canny_hough_circles(other, SIGMA, LO, HI, 5, 30)
        cset = ctx.chamfer_set_create([np.array([[0, 0], [3, 1], [-2, 4]], np.int16)])
        ctx.canny_chamfer(other, SIGMA, LO, HI, cset, 160, 24, min_dist=4, matches_max=64)
        ctx.canny_corners(other, SIGMA, LO, HI, cr.HARRIS, 7, 10, quality_q16=10, corners_max=4096)
        c = _Call(ctx, 3, h, w, 25, response=True)
        d_img = c.upload(frames)
        runs = []
        for _ in range(3):
            c.refill()
            ctx.dev_canny_corners(d_img, SIGMA, LO, HI, h, w, 3, *c.tail(0, 5, 0, 100, 0, 3))
            runs.append(c.raw())
            c.check(want_of(reference(h, w)[2], 0, 5, 0, 100, 0, 3, 25), "dirty context")
        assert runs[0] == runs[1] == runs[2]
        # ... and a cut inside the candidates (the digit passes run on a histogram the last call used)
        c2 = _Call(ctx, 3, h, w, 7)
        for _ in range(2):
            c2.refill()
            ctx.dev_corners_plane(0, 3, h, w, *c2.tail(1, 3, 10, 10, 0, 0))
            c2.check(want_of(reference(h, w)[2], 1, 3, 10, 10, 0, 0, 7), "seven of many")
        c2.free()
        c.free()


def test_the_contexts_plane_and_the_refused_calls(hip):
    h, w = 70, 128
    frames, maps, planes = reference(h, w)
    with hip.Context(0) as ctx:
        c = _Call(ctx, 3, h, w, 30, response=True)
        d_img = c.upload(frames)
        good = (0, 3, 0, 2000, 0, 6)
        # a context that ran no canny call has no plane
        with pytest.raises(capi.CannyHipError) as ei:
            ctx.dev_corners_plane(0, 3, h, w, *c.tail(*good))
        assert ei.value.status == 1
        d_edges = c.upload(np.zeros((3, h, w), np.int16))
        for u8 in (0, 1):
            ctx.set_option("smoothed_u8", u8)
            ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, 3, d_edges)
            c.refill()
            ctx.dev_corners_plane(0, 3, h, w, *c.tail(*good))
            c.check(reference_corners(h, w, 0, 3, 0), f"the context's plane, smoothed_u8 {u8}")
        c.refill()
        # ... nor one of another shape
        for n2, h2, w2 in ((2, h, w), (3, h - 1, w), (3, w, h)):
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_corners_plane(0, n2, h2, w2, *c.tail(*good))
            assert ei.value.status == 1
        d_plane = c.upload(planes.astype(np.uint8))

        def refused(status, n=3, hh=h, ww=w, args=good, **kw):
            t = list(c.tail(*args))
            for name, i in (("cmax", 6), ("rec", 7), ("cnt", 8), ("resp", 11)):
                if name in kw:
                    t[i] = kw[name]
            for call in (lambda: ctx.dev_corners_plane(d_plane, n, hh, ww, *t),
                         lambda: ctx.dev_canny_corners(d_img, SIGMA, LO, HI, hh, ww, n, *t)):
                with pytest.raises(capi.CannyHipError) as ei:
                    call()
                assert ei.value.status == status, (status, n, hh, ww, args, kw)

        for args in ((2, 3, 0, 0, 0, 0), (-1, 3, 0, 0, 0, 0), (0, 4, 0, 0, 0, 0), (0, 9, 0, 0, 0, 0), (0, 3, 1, 0, 0, 0),
                     (1, 3, 65, 0, 0, 0), (1, 3, -1, 0, 0, 0), (0, 3, 0, -1, 0, 0), (0, 3, 0, 65537, 0, 0),
                     (0, 3, 0, 0, -1, 0), (0, 3, 0, 0, 0, -1)):
            refused(1, args=args)
        refused(1, cmax=0)
        refused(1, rec=0)
        refused(1, cnt=0)
        refused(1, rec=c.d_rec + 4)
        refused(1, resp=c.d_resp + 4)
        refused(1, hh=1)
        refused(1, ww=1)
        refused(1, n=0)
        refused(2, cmax=4097)
        refused(2, hh=65536, ww=2)
        refused(2, hh=2, ww=65536)
        refused(2, hh=65535, ww=32769)
        c.untouched()
        hook = ctx.malloc(64)
        for bad in ((0, 8, 0, 0, hook), (hook, 0, 0, 0, hook), (hook, 8, 2, 0, hook), (hook, 8, 0, 1, hook),
                    (hook, 8, 1, 65, hook), (hook, 8, 0, 0, 0), (hook, 2, 0, 0, hook + 4)):
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_corners_arith(*bad)
            assert ei.value.status == 1
        ctx.free(hook)
        c.free()


# ---- past the cap of the capped grids ---------------------------------------------------------------------------------------
def test_the_tile_passes_take_a_second_trip(hip):
    """The maximum pass, the histogram passes and the collect pass share one plan: the 64 x 16 tiles of ONE frame, 1024
    workgroups at most -- so a frame of 33 x 32 tiles is the smallest that sends workgroups into a second trip.  Frame 0
    has few candidates: its later digit passes and its collect walk the key list of the first pass.  Frame 1 is noise with
    more candidates than the list's 16384 keys: every one of its passes computes the responses again, past the cap."""
    n, h, w = 2, 33 * TILE_Y, 32 * TILE_X
    assert capi.corners_plan("tiles", n, h - TILE_Y, w)[0].trips == 1
    plan, chunk = capi.corners_plan("tiles", n, h, w)
    assert chunk == n and (plan.units, plan.grid, plan.per_group, plan.trips) == (33 * 32, 1024, 1, 2)
    rng = np.random.default_rng(12)
    P = np.zeros((h, w), np.uint8)
    for _ in range(300):                                      # blocks everywhere ...
        y, x = rng.integers(0, h - 8), rng.integers(0, w - 8)
        P[y:y + 6, x:x + 7] = rng.integers(100, 200)
    for x in range(10, w - 10, 50):                           # ... and the strongest corners in the second trip's tiles
        P[32 * TILE_Y + 3:32 * TILE_Y + 10, x:x + 9] = 255
    planes = np.stack([P, rng.integers(0, 256, (h, w), dtype=np.uint8)])
    with hip.Context(0) as ctx:
        for (mode, block, k_q8), cmax in (((0, 7, 0), 1024), ((1, 3, 10), 100)):
            want = want_of(planes, mode, block, k_q8, 1000, 0, 3, cmax)
            assert want[0][1] > cmax or cmax == 1024          # frame 0: every candidate goes on, or the cut is inside
            assert want[0][1] < 16384 < want[1][1], "frame 0 is listed in full, frame 1 is not"
            assert (want[0][0][:20, 1] >= 32 * TILE_Y).all(), "the first corners lie in the second trip"
            assert (want[1][0][:, 1] >= 32 * TILE_Y).any(), "some corners of the noise lie in the second trip"
            c = _Call(ctx, n, h, w, cmax, response=True)
            ctx.dev_corners_plane(c.upload(planes), n, h, w, *c.tail(mode, block, k_q8, 1000, 0, 3))
            assert c.check(want, f"mode {mode} block {block}") >= 100
            c.free()


def test_a_batch_walked_in_two_chunks(hip):
    """A chunk holds 1024 frames at most: 1030 small frames are walked as 1024 + 6, and frame f's outputs still land in
    frame f's slots."""
    n, h, w = 1030, 5, 7
    assert capi.corners_plan("tiles", n, h, w)[1] == 1024
    planes = np.random.default_rng(31).integers(0, 256, (n, h, w), dtype=np.uint8)
    planes[1027] = 9                                         # a flat frame in the second chunk
    want = want_of(planes, 0, 3, 0, 20000, 0, 2, 3)
    with hip.Context(0) as ctx:
        c = _Call(ctx, n, h, w, 3, response=True)
        ctx.dev_corners_plane(c.upload(planes), n, h, w, *c.tail(0, 3, 0, 20000, 0, 2))
        assert c.check(want, "1024 + 6 frames") > n
        c.free()


_TRIPLES = []


def triples():
    if not _TRIPLES:
        t = cr.arith_triples()
        t.setflags(write=False)
        _TRIPLES.append(t)
    return _TRIPLES[0]


@pytest.mark.parametrize("mode,k_q8", [(0, 0), (1, 10), (1, 64), (1, 0)])
def test_the_device_arithmetic_on_the_cpu_tests_triples(hip, mode, k_q8):
    t = triples()
    n = len(t)
    plan, _ = capi.corners_plan("arith", n=n)
    assert plan.grid == 1024 and plan.trips >= 2, "the hook's grid is past its cap"
    want = cr.response_array(t[:, 0], t[:, 1], t[:, 2], mode, k_q8)
    with hip.Context(0) as ctx:
        d_in, d_out = ctx.malloc(t.nbytes), ctx.malloc(8 * n + 4 * N_GUARD)
        ctx.h2d(d_in, t)
        ctx.h2d(d_out, np.full(2 * n + N_GUARD, SENT, np.uint32))
        ctx.dev_corners_arith(d_in, n, mode, k_q8, d_out)
        out = np.empty(2 * n + N_GUARD, np.uint32)
        ctx.d2h(out, d_out)
        ctx.free(d_in)
        ctx.free(d_out)
    assert (out[2 * n:] == SENT).all()
    got = out[:2 * n].view(np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {n} differ, first {t[bad[0]].tolist()}: {got[bad[0]]} != {want[bad[0]]}"


# ---- host buffers, the CLI ---------------------------------------------------------------------------------------------------
def test_the_host_buffer_form(hip):
    h, w = 70, 77
    frames, _, planes = reference(h, w)
    with hip.Context(0) as ctx:
        for mode, block, k_q8 in ((0, 3, 0), (1, 7, 10)):
            got, cands, rmax = ctx.canny_corners(frames, SIGMA, LO, HI, mode, block, k_q8, quality_q16=2000, min_dist=6,
                                                 corners_max=40)
            want = reference_corners(h, w, mode, block, k_q8)
            assert cands.tolist() == [k for _, k, _, _ in want] and rmax.tolist() == [m for _, _, m, _ in want]
            for f in range(3):
                assert np.array_equal(got[f].view(np.int64).reshape(-1, 4), want[f][0]), f"frame {f}"
        one, cands, _ = ctx.canny_corners(frames[0], SIGMA, LO, HI, corners_max=1)
        assert len(one) == 1 and len(one[0]) == 1 and cands[0] > 1


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.parametrize("spec,args", [("2000,6,40", (0, 3, 0)), ("2000,6,40,7", (0, 7, 0)), ("2000,6,40,5,10", (1, 5, 10))])
def test_main_q_writes_the_corners_of_the_rule(tmp_path, spec, args):
    frame = reference(70, 128)[0][0]
    _write_pgm(tmp_path / "frame.pgm", frame)
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, str(SIGMA), str(LO), str(HI), "-i", str(tmp_path / "frame.pgm"), "-o", str(tmp_path), "-q", spec],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = reference_corners(70, 128, *args)[0][0]
    assert len(want) >= 3
    lines = (tmp_path / "canny_corners.txt").read_text().splitlines()
    assert lines == [f"0 {x} {y} {v} {rank}" for x, y, v, rank in want.tolist()]
