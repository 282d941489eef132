"""Every entry point on a context whose device workspaces hold another call's words.

A canny_hip_ctx keeps its workspaces from call to call (DevBuf::ensure keeps a buffer that is large enough), so from the
second call on every kernel runs on memory that is not zero.  DESIGN.md section 20 lists, per workspace, which launch
initialises it and why nothing reads a word before it is written; this module runs each entry point on a context where
that has to be true.  Every test goes through the same steps on ONE context:

  1. warm:    the call under test once, on other data of the target's shape, so that its workspaces exist;
  2. dirty:   "leftover" -- primer calls of the same entry point at a larger geometry (3 x 200 x 328: 4 x 6 tiles of 64 x 64
              with padding rows and columns) on the densest legal input -- and, in the "ones" / "zeros" modes, 0xFF / 0x00
              bytes written over every workspace of kind DATA afterwards.  Workspaces of kind INDEX only ever hold what the
              library itself left there (in bounds for the allocation by construction), CACHE workspaces are never written;
  3. the precondition: every workspace the call uses is allocated and really holds the dirt;
  4. target:  the call, every output against the oracle / the numpy rules, bit for bit;
  5. reuse:   no workspace has moved or grown during the target call, else the test did not test what it claims.

The targets are the smallest shapes at which the tile layout moves: 2 x 100 x 200 (a shrunk frame, other tiles_x), 1 x 65 x 72
(one image row in the second tile row), 3 x 37 x 77 (width % 8 != 0: the unfused classify route), 2 x 130 x 264 and
3 x 200 x 360 (larger than the primer, inside the 1/8 head-room of the allocation).  An empty map and a map whose only pixel
is the last one of the frame follow: there "nothing was written" and "the leftover shows through" look alike."""
import numpy as np
import pytest

import components_rule
import contours_rule
import edt_rule
import hist_rule
import hough_circles_rule as circles_rule
import hough_rule
import hough_segments_rule as segments_rule
import oracle
import polygons_rule
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

PI = float(np.pi)
PRIMER = (3, 200, 328)
TARGETS = [(2, 100, 200), (1, 65, 72), (3, 37, 77), (2, 130, 264), (3, 200, 360)]
MODES = ("leftover", "ones", "zeros")
SIGMA, LO, HI = 1.4, 50, 150
N_GUARD = 64
FILL = {1: 0xA5, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0xEEEEEEEEEEEEEEEE}   # what an output holds before the call, by word size
PLANES = ("smoothed", "plane_s", "plane_c", "stamps", "flags")   # what every route through dev_canny uses
LINES_MAX, LINE_THRESHOLD = 7, 25
SEG_MIN_LENGTH, SEG_MAX_GAP = 5, 2
CIRCLES = (5, 20, 1, 12, 8, 6, 32)   # min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max
TOLERANCE = (384, 655)               # epsilon_q8, ratio_q16 of the polygon stage
MIN_AREA = 2

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- the workspaces ---------------------------------------------------------------------------------------------------
def _snapshot(ctx):
    return {name: (ptr, size, kind) for name, ptr, size, kind in ctx.selftest_workspaces()}


def _synthetic(hip, ctx, mode):
    """0xFF or 0x00 bytes over the whole of every allocated DATA workspace.  INDEX and CACHE workspaces are left alone: a
    word that some kernel turns into an address only ever holds what the library itself wrote."""
    value = 0xFF if mode == "ones" else 0x00
    for ptr, size, kind in _snapshot(ctx).values():
        if kind == hip.WS_DATA and ptr:
            ctx.h2d(ptr, np.full(size, value, np.uint8))
    ctx.synchronize()


def _precondition(hip, ctx, used, mode, what):
    """The enumerator's list before the target call; every used workspace exists and holds the dirt of `mode`."""
    snap = _snapshot(ctx)
    for name in used:
        assert name in snap, f"{what}: no workspace called {name}"
        ptr, size, kind = snap[name]
        assert ptr and size, f"{what}: {name} is not allocated, so the call under test does not run on it"
        got = np.empty(size, np.uint8)
        ctx.d2h(got, ptr)
        if kind == hip.WS_CACHE:
            continue
        # An allocation is the need of the call that made it plus an eighth.  Only the need was ever written by the
        # library, so leftover dirt is looked for there and not in the head-room, which holds whatever the allocator gave.
        need = size * 8 // 9
        if mode != "leftover" and kind == hip.WS_DATA:
            assert (got == (0xFF if mode == "ones" else 0x00)).all(), f"{what}: {name} does not hold the pattern"
        elif name.split(".")[-1] != "flags":
            # (flags: the last sweep that changed something and the domain flag.  A primer that converges in sweep 0
            # leaves both zero; their non-zero dirt is the "ones" mode's)
            assert got[:need].any(), f"{what}: the primer left {name} all zero"
    return snap


def _check_reuse(ctx, before, used, what):
    after = _snapshot(ctx)
    for name in used:
        assert after[name][:2] == before[name][:2], f"{what}: {name} was reallocated: the call ran on fresh memory"
    moved = [name for name in before if after[name][:2] != before[name][:2]]
    assert not moved and len(after) == len(before), f"{what}: {moved} appeared or moved during the target call"


def _dirty_cycle(hip, ctx, mode, used, warm, primers, target, what):
    warm()
    for primer in primers:
        primer()
    if mode != "leftover":
        _synthetic(hip, ctx, mode)
    before = _precondition(hip, ctx, used, mode, what)
    target()
    _check_reuse(ctx, before, used, what)


class _Bufs:
    """Caller-side device buffers of one call: inputs, and outputs pre-filled with a sentinel and followed by guard words."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.meta = ctx, [], {}

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def out(self, key, count, dtype):
        count, size = int(count), np.dtype(dtype).itemsize
        a = np.full(count + N_GUARD, FILL[size], f"u{size}").view(dtype)
        self.meta[key] = (self.up(a), count, np.dtype(dtype), a[0])
        return self.meta[key][0]

    def get(self, key):
        ptr, count, dtype, fill = self.meta[key]
        a = np.empty(count + N_GUARD, dtype)
        self.ctx.d2h(a, ptr)
        assert (a[count:].view(np.uint8) == np.full(N_GUARD, fill).view(np.uint8)).all(), f"written past the end of {key}"
        return a[:count]

    def untouched(self, key, part):
        """part of an output still holds the sentinel (compared as bytes, so float NaN patterns work too)"""
        fill = self.meta[key][3]
        return (np.ascontiguousarray(part).ravel().view(np.uint8) == np.full(part.size, fill).view(np.uint8)).all()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _frames(g, seed):
    n, h, w = g
    return np.stack([synth_frame(h, w, seed + i) for i in range(n)])


def _texture(g, seed):
    """The densest legal input of the forms behind dev_canny: noise, to be run with min_val 1 and max_val 2."""
    return np.random.default_rng(seed).integers(0, 256, g, dtype=np.uint8)


def _weak_chains(g):
    """Frames whose weak edges hang on strong ones far away: horizontal steps of 30 gray levels every 15 rows (a row of
    intermediate value on one side, so that the gradient has one maximum and survives the suppression) that are steps of
    140 levels in the first 24 columns only.  At (1, 150) the strong left ends pull every step in, tile by tile."""
    n, h, w = g
    p = np.arange(h)[:, None] % 30
    s = np.where(p < 14, 0.0, np.where(p == 14, 0.3, np.where(p < 29, 1.0, 0.7)))
    img = np.where(np.arange(w)[None, :] < 24, 60 + 140 * s, 100 + 30 * s).astype(np.uint8)
    return np.broadcast_to(img, g).copy()


def _canny_primers(g=PRIMER, colour=False):
    """(frames, min_val, max_val) of the primer calls of a form behind dev_canny.  Noise at (1, 2) gives the densest planes
    and maps, but nearly every candidate is strong at once and no tile border changes during the sweeps: the scheduling
    words stay as hyst_prepare zeroed them.  So a second call follows that is reached over many sweeps and tiles and
    leaves tile stamps, queue entries and counters behind."""
    noise, chains = _texture(g, 1), _weak_chains(g)
    reached = _cached(("chains", g[1:]), lambda: oracle.canny(chains[0], SIGMA, 1, 150))
    strong = oracle.canny(chains[0], SIGMA, 150, 150)
    assert reached[:, -8:].any() and not strong[:, 64:].any(), "the weak chains cross every tile column from the first"
    if colour:
        return [(np.repeat(noise[..., None], 3, axis=-1) ^ np.array([0, 85, 170], np.uint8), 1, 2),
                (np.repeat(chains[..., None], 3, axis=-1), 1, 150)]
    return [(noise, 1, 2), (chains, 1, 150)]


def _maps(frames, lo=LO, hi=HI, sigma=SIGMA):
    return _cached(("maps", frames.shape, frames.tobytes(), lo, hi, sigma),
                   lambda: np.stack([oracle.canny(f, sigma, lo, hi) for f in frames]))


def _grads(frames):
    def make():
        pairs = [circles_rule.sobel(oracle.gaussian(f, SIGMA)) for f in frames]
        return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return _cached(("grads", frames.shape, frames.tobytes()), make)


def _primer_masks():
    """Two stacks of designed maps at the primer geometry.  Frames 0 and 1 hold complementary column-alternating maps in
    the two calls, so between them every pixel has been the start of a run and every entry of a parent array holds a
    plausible parent; frame 2 is all ones, then a map whose last row and last column are fully set."""
    n, h, w = PRIMER
    even = np.zeros((h, w), bool)
    even[:, 0::2] = True
    last = np.zeros((h, w), bool)
    last[h - 1, :] = True
    last[:, w - 1] = True
    return np.stack([even, ~even, np.ones((h, w), bool)]), np.stack([~even, even, last])


class _Case:
    """The inputs of one call in both forms: frames for the forms behind dev_canny, and their oracle map as packed bits
    (with the gradient planes the circle stage takes) for the *_bits forms, so that both forms have one expected value."""

    def __init__(self, g, frames=None, masks=None, lo=LO, hi=HI):
        self.g, self.lo, self.hi = g, lo, hi
        self.frames = frames
        if masks is None:
            self.maps = _maps(frames, lo, hi)
            masks = self.maps != 0
        else:
            self.maps = np.where(masks, 255, 0).astype(np.int16)
        self.masks = masks
        self.bits = np.packbits(masks, axis=-1)
        if frames is not None:
            self.gx, self.gy = _grads(frames)
        else:   # the bits form takes any gradient planes: a slope that turns with the position
            n, h, w = g
            y, x = np.mgrid[0:h, 0:w]
            self.gx = np.broadcast_to((x - w // 2).astype(np.int16), g).copy()
            self.gy = np.broadcast_to((y - h // 2).astype(np.int16), g).copy()
        self.key = (g, self.bits.tobytes(), self.gx.tobytes(), self.gy.tobytes())


def _target_cases(g, src):
    """(name, case to warm with, case to check) of a geometry: a textured batch, an empty map, and -- where the map can
    be designed -- a single set pixel in the last row and column."""
    n, h, w = g
    out = [("texture", _Case(g, _frames(g, 7000 + h)), _Case(g, _frames(g, 100 + h + w)))]
    if g in (TARGETS[0], TARGETS[2]):
        flat = np.full(g, 90, np.uint8)
        out.append(("empty", out[0][1], _Case(g, flat)))
        assert not out[-1][2].masks.any()
        if src == "bits":
            corner = np.zeros(g, bool)
            corner[:, h - 1, w - 1] = True
            out.append(("corner", out[0][1], _Case(g, None, corner)))
    return out


def _primer_cases(src):
    if src == "bits":
        a, b = _cached("primer masks", _primer_masks)
        return [_Case(PRIMER, None, a), _Case(PRIMER, None, b)]
    return [_Case(PRIMER, frames, lo=lo, hi=hi) for frames, lo, hi in _canny_primers()]


# ---- the analysis stages: launch, expected value, comparison ---------------------------------------------------------------
# launch(ctx, B, src, case, caps, null, opt) queues the call with guarded outputs in B; want(hip, case, opt) is the rule's
# value; check(B, case, want, caps, null, what) compares every output that exists.  caps: the capacities of the call.
def _source(B, src, case):
    return B.up(case.bits if src == "bits" else case.frames)


def _edges_out(B, src, case, null):
    """the optional s16 map of the forms behind dev_canny: present, or null (the edges16 workspace)"""
    return B.out("edges", case.maps.size, np.int16) if src == "canny" and not null else 0


def _check_edges(B, case, what):
    if "edges" in B.meta:
        assert np.array_equal(B.get("edges").reshape(case.maps.shape), case.maps), f"{what}: the s16 map"


def _points_want(hip, case, opt):
    lists = [np.flatnonzero(m).astype(np.uint32) for m in case.masks]
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in lists])
    return np.concatenate(lists), off


def _points_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    cap = 0 if null else caps["points"]
    d_pts = B.out("points", cap, np.uint32) if cap else 0
    d_off = B.out("offsets", n + 1, np.uint64)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_points_from_bits(d_src, h, w, n, d_pts, cap, d_off)
    else:
        ctx.dev_canny_points(d_src, SIGMA, case.lo, case.hi, h, w, n, d_pts, cap, d_off, _edges_out(B, src, case, null))


def _points_check(B, case, want, caps, null, what):
    pts, off = want
    assert np.array_equal(B.get("offsets"), off), f"{what}: offsets"
    if "points" in B.meta:
        got = B.get("points")
        assert np.array_equal(got[:pts.size], pts), f"{what}: points"
        assert B.untouched("points", got[pts.size:]), f"{what}: written past the points"
    _check_edges(B, case, what)


def _hough_want(hip, case, opt):
    n, h, w = case.g
    rho, theta, lo_t, hi_t = opt.get("hough", (1.0, PI / 180, 0.0, PI))
    na, nr = hip.hough_geometry(h, w, rho, theta, lo_t, hi_t)
    tabs = hip.hough_tables(rho, theta, lo_t, na)
    acc = np.stack([hough_rule.accumulate(np.flatnonzero(m), w, nr, *tabs) for m in case.masks])
    return dict(acc=acc, numrho=nr, tabs=tabs, args=(rho, theta, lo_t, hi_t),
                lines=[hough_rule.lines(a, LINE_THRESHOLD, LINES_MAX, rho, theta, lo_t) for a in acc])


def _lines_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    rho, theta, lo_t, hi_t = opt.get("hough", (1.0, PI / 180, 0.0, PI))
    slots = n * LINES_MAX
    d = [B.out("lines", 2 * slots, np.uint32), B.out("votes", slots, np.uint32), B.out("bases", slots, np.uint32),
         B.out("counts", n, np.uint32)]
    d_accum = 0 if null else B.out("accum", caps["accum"], np.uint32)
    d_src = _source(B, src, case)
    tail = (rho, theta, LINE_THRESHOLD, LINES_MAX, lo_t, hi_t, *d, d_accum)
    if src == "bits":
        ctx.dev_hough_bits(d_src, n, h, w, *tail)
    else:
        ctx.dev_canny_hough(d_src, SIGMA, case.lo, case.hi, h, w, n, *tail, d_edges=_edges_out(B, src, case, null))


def _lines_check(B, case, want, caps, null, what):
    n = case.g[0]
    if "accum" in B.meta:
        got = B.get("accum").view(np.int32).reshape(want["acc"].shape)
        assert np.array_equal(got, want["acc"]), f"{what}: {int((got != want['acc']).sum())} accumulator cells differ"
    counts = B.get("counts").view(np.int32)
    lines, votes = B.get("lines").reshape(n, LINES_MAX, 2), B.get("votes").reshape(n, LINES_MAX)
    bases = B.get("bases").reshape(n, LINES_MAX)
    for f, (wl, wv, wb, wc) in enumerate(want["lines"]):
        k = min(LINES_MAX, wc)
        assert counts[f] == wc, f"{what} frame {f}: count {counts[f]} != {wc}"
        assert np.array_equal(bases[f, :k], wb), f"{what} frame {f}: bases"
        assert np.array_equal(votes[f, :k].view(np.int32), wv), f"{what} frame {f}: votes"
        assert np.array_equal(lines[f, :k], wl.view(np.uint32)), f"{what} frame {f}: (rho, theta) bit patterns"
        assert B.untouched("bases", bases[f, k:]) and B.untouched("votes", votes[f, k:]) and \
            B.untouched("lines", lines[f, k:]), f"{what} frame {f}: slots past the count were written"
    _check_edges(B, case, what)


def _segments_want(hip, case, opt):
    hw = _hough_want(hip, case, opt)
    hw["segments"] = [segments_rule.segments(case.masks[f], hw["lines"][f][2], hw["numrho"], *hw["tabs"], SEG_MIN_LENGTH,
                                             SEG_MAX_GAP, opt["exclusive"]) for f in range(case.g[0])]
    return hw


def _segments_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    rho, theta, lo_t, hi_t = opt.get("hough", (1.0, PI / 180, 0.0, PI))
    cap = caps["segments"]
    d_seg, d_cnt = B.out("segments", n * cap * 6, np.uint32), B.out("seg_counts", n, np.uint32)
    d_src = _source(B, src, case)
    if src == "bits":
        # the lines come from the device's own transform of the same map (compared in _segments_check)
        d_bases, d_counts = B.out("bases", n * LINES_MAX, np.uint32), B.out("counts", n, np.uint32)
        ctx.dev_hough_bits(d_src, n, h, w, rho, theta, LINE_THRESHOLD, LINES_MAX, lo_t, hi_t, 0, 0, d_bases, d_counts, 0)
        ctx.dev_hough_segments_bits(d_src, n, h, w, rho, theta, lo_t, hi_t, d_bases, d_counts, LINES_MAX, SEG_MIN_LENGTH,
                                    SEG_MAX_GAP, opt["exclusive"], d_seg, cap, d_cnt)
    else:
        # null: neither the line outputs nor the accumulator nor the map (seg_lines, hough_accum, edges16)
        d_bases = 0 if null else B.out("bases", n * LINES_MAX, np.uint32)
        d_counts = 0 if null else B.out("counts", n, np.uint32)
        d_accum = 0 if null else B.out("accum", caps["accum"], np.uint32)
        ctx.dev_canny_hough_segments(d_src, SIGMA, case.lo, case.hi, h, w, n, rho, theta, LINE_THRESHOLD, LINES_MAX, lo_t,
                                     hi_t, SEG_MIN_LENGTH, SEG_MAX_GAP, opt["exclusive"], d_seg, cap, d_cnt, d_bases=d_bases,
                                     d_line_counts=d_counts, d_accum=d_accum, d_edges=_edges_out(B, src, case, null))


def _segments_check(B, case, want, caps, null, what):
    n, cap = case.g[0], caps["segments"]
    if "bases" in B.meta:
        counts, bases = B.get("counts").view(np.int32), B.get("bases").reshape(n, LINES_MAX)
        for f, (_, _, wb, wc) in enumerate(want["lines"]):
            assert counts[f] == wc and np.array_equal(bases[f, :min(LINES_MAX, wc)], wb), f"{what} frame {f}: the lines"
    if "accum" in B.meta:
        assert np.array_equal(B.get("accum").view(np.int32).reshape(want["acc"].shape), want["acc"]), f"{what}: accumulators"
    seg, cnt = B.get("segments").reshape(n, cap, 6), B.get("seg_counts").view(np.int32)
    for f, ws in enumerate(want["segments"]):
        k = min(cap, len(ws))
        assert cnt[f] == len(ws), f"{what} frame {f}: segment count {cnt[f]} != {len(ws)}"
        assert np.array_equal(seg[f, :k].view(np.int32), ws[:k]), f"{what} frame {f}: segment records"
        assert B.untouched("segments", seg[f, k:]), f"{what} frame {f}: slots past the count were written"
    _check_edges(B, case, what)


def _circles_want(hip, case, opt):
    lo_r, hi_r, shift, thr, support, min_dist, cm = CIRCLES
    acc = np.stack([circles_rule.accumulate(m, x, y, lo_r, hi_r, shift) for m, x, y in zip(case.masks, case.gx, case.gy)])
    return acc, [circles_rule.circles(m, a, lo_r, hi_r, shift, thr, support, min_dist, cm) for m, a in zip(case.masks, acc)]


def _circles_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    cm = CIRCLES[6]
    d_rec, d_cnt = B.out("circles", n * cm * 6, np.uint32), B.out("counts", n, np.uint32)
    d_peaks = 0 if null else B.out("peaks", n, np.uint32)
    d_accum = 0 if null else B.out("accum", caps["accum"], np.uint32)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_hough_circles_bits(d_src, B.up(case.gx), B.up(case.gy), n, h, w, *CIRCLES, d_rec, d_cnt, d_peaks, d_accum)
    else:
        ctx.dev_canny_hough_circles(d_src, SIGMA, case.lo, case.hi, h, w, n, *CIRCLES, d_rec, d_cnt, d_peaks, d_accum,
                                    d_edges=_edges_out(B, src, case, null))


def _circles_check(B, case, want, caps, null, what):
    acc, per = want
    n, cm = case.g[0], CIRCLES[6]
    if "accum" in B.meta:
        got = B.get("accum").view(np.int32).reshape(acc.shape)
        assert np.array_equal(got, acc), f"{what}: {int((got != acc).sum())} accumulator cells differ"
    counts, rec = B.get("counts").view(np.int32), B.get("circles").reshape(n, cm, 6)
    for f, (wr, n_peaks) in enumerate(per):
        assert counts[f] == len(wr), f"{what} frame {f}: count {counts[f]} != {len(wr)}"
        if "peaks" in B.meta:
            assert B.get("peaks").view(np.int32)[f] == n_peaks, f"{what} frame {f}: peak count"
        assert np.array_equal(rec[f, :len(wr)].view(np.int32), wr), f"{what} frame {f}: records"
        assert B.untouched("circles", rec[f, len(wr):]), f"{what} frame {f}: slots past the count were written"
    _check_edges(B, case, what)


def _components_want(hip, case, opt):
    return components_rule.csr(case.masks, MIN_AREA)


def _components_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    cap = caps["records"]
    d_labels = 0 if null else B.out("labels", n * h * w, np.int32)   # null: the parent array is the cc_parent workspace
    d_kept = B.out("kept", n * h * w, np.uint8)
    d_stats, d_off = B.out("stats", cap * 6, np.int32), B.out("offsets", n + 1, np.uint64)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_components_bits(d_src, h, w, n, MIN_AREA, d_labels, d_kept, d_stats, cap, d_off)
    else:
        ctx.dev_canny_components(d_src, SIGMA, case.lo, case.hi, h, w, n, MIN_AREA, d_labels, d_kept, d_stats, cap, d_off,
                                 _edges_out(B, src, case, null))


def _components_check(B, case, want, caps, null, what):
    labels, stats, off = want
    assert np.array_equal(B.get("offsets"), off), f"{what}: offsets"
    if "labels" in B.meta:
        assert np.array_equal(B.get("labels").reshape(labels.shape), labels), f"{what}: labels"
    assert np.array_equal(B.get("kept").reshape(labels.shape), np.where(labels != 0, 255, 0)), f"{what}: kept_u8"
    got, k = B.get("stats").reshape(-1, 6), min(caps["records"], stats.shape[0])
    assert np.array_equal(got[:k], stats[:k]), f"{what}: stats"
    assert B.untouched("stats", got[k:]), f"{what}: written past the records"
    _check_edges(B, case, what)


def _contours_want(hip, case, opt):
    return contours_rule.csr(case.masks, MIN_AREA)


def _contour_outputs(B, n, caps, null):
    cap, pcap = caps["records"], caps["chain_points"]
    return (0 if null else B.out("stats", cap * 6, np.int32), cap, B.out("offsets", n + 1, np.uint64),
            B.out("chain_offsets", cap + 1, np.uint64), B.out("points", pcap, np.int32), pcap,
            B.out("point_offsets", n + 1, np.uint64))


def _contours_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    outs = _contour_outputs(B, n, caps, null)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_contours_bits(d_src, h, w, n, MIN_AREA, *outs)
    else:
        ctx.dev_canny_contours(d_src, SIGMA, case.lo, case.hi, h, w, n, MIN_AREA, *outs, _edges_out(B, src, case, null))


def _contours_check(B, case, want, caps, null, what):
    stats, off, chain, points, poff = want
    fit = min(int(off[-1]), caps["records"])
    assert np.array_equal(B.get("offsets"), off), f"{what}: offsets"
    assert np.array_equal(B.get("point_offsets"), poff), f"{what}: point_offsets"
    got = B.get("chain_offsets")
    assert np.array_equal(got[:fit + 1], chain[:fit + 1]), f"{what}: chain_offsets"
    assert B.untouched("chain_offsets", got[fit + 1:]), f"{what}: written past the chain offsets"
    got, pfit = B.get("points"), min(caps["chain_points"], int(chain[fit]))
    assert np.array_equal(got[:pfit], points[:pfit]), f"{what}: chain points"
    assert B.untouched("points", got[pfit:]), f"{what}: written past the chain points"
    if "stats" in B.meta:
        got = B.get("stats").reshape(-1, 6)
        assert np.array_equal(got[:fit], stats[:fit]) and B.untouched("stats", got[fit:]), f"{what}: stats"
    _check_edges(B, case, what)


def _polygons_want(hip, case, opt):
    ct = contours_rule.csr(case.masks, MIN_AREA)
    return ct, polygons_rule.csr(ct[2], ct[3], ct[3].size, case.g[2], *TOLERANCE)


def _polygons_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    cap, pcap = caps["records"], caps["chain_points"]
    outs = _contour_outputs(B, n, caps, True)
    d_voff = B.out("vertex_offsets", cap + 1, np.uint64)
    d_verts = B.out("vertices", pcap, np.int32)
    d_meas = 0 if null else B.out("measures", cap * 4, np.int64)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_polygons_bits(d_src, h, w, n, MIN_AREA, *outs, *TOLERANCE, d_voff, d_verts, pcap, d_meas)
    else:
        ctx.dev_canny_polygons(d_src, SIGMA, case.lo, case.hi, h, w, n, MIN_AREA, *outs, *TOLERANCE, d_voff, d_verts, pcap,
                               d_meas, _edges_out(B, src, case, null))


def _polygons_check(B, case, want, caps, null, what):
    ct, (voff, verts, meas) = want
    _contours_check(B, case, ct, caps, True, what)
    fit = ct[0].shape[0]
    assert fit <= caps["records"] and ct[3].size <= caps["chain_points"]
    got = B.get("vertex_offsets")
    assert np.array_equal(got[:fit + 1], voff) and B.untouched("vertex_offsets", got[fit + 1:]), f"{what}: vertex_offsets"
    got = B.get("vertices")
    assert np.array_equal(got[:verts.size], verts) and B.untouched("vertices", got[verts.size:]), f"{what}: vertices"
    if "measures" in B.meta:
        got = B.get("measures").reshape(-1, 4)
        assert np.array_equal(got[:fit], meas) and B.untouched("measures", got[fit:]), f"{what}: measures"


def _edt_want(hip, case, opt):
    return edt_rule.stack(case.masks)


def _edt_launch(ctx, B, src, case, caps, null, opt):
    n, h, w = case.g
    d_d2 = 0 if null else B.out("dist2", n * h * w, np.int32)   # null: the column scan's stack is the edt_stack workspace
    d_d, d_nn = B.out("dist", n * h * w, np.float32), B.out("nearest", n * h * w, np.int32)
    d_src = _source(B, src, case)
    if src == "bits":
        ctx.dev_edt_bits(d_src, h, w, n, d_d2, d_d, d_nn)
    else:
        ctx.dev_canny_edt(d_src, SIGMA, case.lo, case.hi, h, w, n, d_d2, d_d, d_nn, _edges_out(B, src, case, null))


def _edt_check(B, case, want, caps, null, what):
    d2, d, nn = want
    if "dist2" in B.meta:
        assert np.array_equal(B.get("dist2").reshape(d2.shape), d2), f"{what}: dist2"
    assert np.array_equal(B.get("dist").view(np.uint32).reshape(d.shape), d.view(np.uint32)), f"{what}: dist bit patterns"
    assert np.array_equal(B.get("nearest").reshape(nn.shape), nn), f"{what}: nearest"
    _check_edges(B, case, what)


def _accum_cells(hip, g, opt):
    n, h, w = g
    rho, theta, lo_t, hi_t = opt.get("hough", (1.0, PI / 180, 0.0, PI))
    na, nr = hip.hough_geometry(h, w, rho, theta, lo_t, hi_t)
    return n * (na + 2) * (nr + 2)


def _circle_cells(g):
    n, h, w = g
    c = 1 << CIRCLES[2]
    return n * ((h + c - 1) // c + 2) * ((w + c - 1) // c + 2)


# name -> launch, want, check, options, the workspaces of the *_bits form (present, extra when null), the extra ones of
# the stage behind dev_canny (present, extra when null; PLANES and, without d_edges, edges16 are added to these)
STAGES = {
    "points": (_points_launch, _points_want, _points_check, {}, (("points",), ()), (("points",), ())),
    "lines_atomics": (_lines_launch, _hough_want, _lines_check, {"hough_path": 1},
                      (("hough_ws", "hough_tab"), ("hough_accum",)), (("hough_ws", "hough_tab"), ("hough_accum",))),
    "lines_lds": (_lines_launch, _hough_want, _lines_check, {"hough_path": 2},
                  (("hough_ws", "hough_tab"), ("hough_accum",)), (("hough_ws", "hough_tab"), ("hough_accum",))),
    "segments": (_segments_launch, _segments_want, _segments_check, {"exclusive": 0},
                 (("hough_ws", "hough_tab", "hough_accum", "seg_ws"), ()),
                 (("hough_ws", "hough_tab", "seg_ws"), ("hough_accum", "seg_lines"))),
    "segments_exclusive": (_segments_launch, _segments_want, _segments_check, {"exclusive": 1},
                           (("hough_ws", "hough_tab", "hough_accum", "seg_work"), ()),
                           (("hough_ws", "hough_tab", "seg_work"), ("hough_accum", "seg_lines"))),
    "circles": (_circles_launch, _circles_want, _circles_check, {}, (("circ_ws",), ("circ_accum",)),
                (("circ_ws",), ("circ_accum",))),
    "components": (_components_launch, _components_want, _components_check, {}, (("cc_ws",), ("cc_parent",)),
                   (("cc_ws",), ("cc_parent",))),
    "contours": (_contours_launch, _contours_want, _contours_check, {}, (("cc_parent", "cc_ws", "ct_ws"), ()),
                 (("cc_parent", "cc_ws", "ct_ws"), ())),
    "polygons": (_polygons_launch, _polygons_want, _polygons_check, {}, (("cc_parent", "cc_ws", "ct_ws", "pg_ws"), ()),
                 (("cc_parent", "cc_ws", "ct_ws", "pg_ws"), ())),
    "edt": (_edt_launch, _edt_want, _edt_check, {}, (("edt_cols",), ("edt_stack",)), (("edt_cols",), ("edt_stack",))),
}


def _caps(hip, stage, g, opt, want=None):
    """The capacities of a call: what the expected value needs (exactly, so that a count one too high writes a guard), or
    for a primer, whose result nobody computes, a generous fixed share of the frame."""
    n, h, w = g
    caps = dict(accum=_circle_cells(g) if stage == "circles" else _accum_cells(hip, g, opt))
    if want is None:
        caps.update(points=n * h * w, records=n * h * w // 4, chain_points=2 * n * h * w, segments=512)
    elif stage == "points":
        caps.update(points=max(int(want[0].size), 1))
    elif stage == "components":
        caps.update(records=max(want[1].shape[0], 1))
    elif stage == "contours":
        caps.update(records=max(want[0].shape[0], 1), chain_points=max(want[3].size, 1))
    elif stage == "polygons":
        caps.update(records=max(want[0][0].shape[0], 1), chain_points=max(want[0][3].size, 1))
    elif stage.startswith("segments"):
        caps.update(segments=max(len(s) for s in want["segments"]) + 2)
    return caps


def _used(stage, src, null):
    bits_used, canny_used = STAGES[stage][4], STAGES[stage][5]
    present, extra = bits_used if src == "bits" else canny_used
    used = tuple(present) + (tuple(extra) if null else ())
    if src == "canny":
        used += PLANES + (("edges16",) if null else ())
    return used


def _stage_want(hip, stage, case, opt):
    return _cached(("want", stage, case.key, tuple(sorted(opt.items()))), lambda: STAGES[stage][1](hip, case, opt))


def _run_stage(hip, ctx, stage, src, case, null, opt, check=True, what=""):
    launch, _, checker = STAGES[stage][:3]
    want = _stage_want(hip, stage, case, opt) if check else None
    caps = _caps(hip, stage, case.g, opt, want)
    with _Bufs(ctx) as B:
        launch(ctx, B, src, case, caps, null, opt)
        if check:
            checker(B, case, want, caps, null, what)
        else:
            ctx.synchronize()


def _warm_stage(hip, ctx, stage, src, warm_case, case, null, opt):
    """the target's launch -- same shape, same capacities -- on other data, unchecked"""
    want = _stage_want(hip, stage, case, opt)
    with _Bufs(ctx) as B:
        STAGES[stage][0](ctx, B, src, warm_case, _caps(hip, stage, case.g, opt, want), null, opt)
        ctx.synchronize()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("null", [False, True], ids=["outputs_present", "outputs_null"])
@pytest.mark.parametrize("src", ["bits", "canny"])
@pytest.mark.parametrize("stage", list(STAGES))
def test_analysis_stage_on_dirty_workspaces(hip, stage, src, null, mode):
    """Each stage in its dev_*_bits form and behind dev_canny, optional outputs present and null (a null output moves the
    work into a workspace: labels -> cc_parent, dist2 -> edt_stack, the accumulators -> hough_accum / circ_accum, the
    line lists -> seg_lines, the s16 map -> edges16)."""
    opt = STAGES[stage][3]
    used = _used(stage, src, null)
    primers = _primer_cases(src)
    with hip.Context(0) as ctx:
        if "hough_path" in opt:
            ctx.set_option("hough_path", opt["hough_path"])
        for g in TARGETS:
            for name, warm_case, case in _target_cases(g, src):
                what = f"{stage} {src} {g} {name} null={null} {mode}"
                if stage == "polygons" and g == TARGETS[4] and name == "texture":
                    chain = _stage_want(hip, stage, case, opt)[0][2]
                    assert np.diff(chain.astype(np.int64)).max() > 64, "a chain long enough to need the flag bytes of pg_ws"
                _dirty_cycle(hip, ctx, mode, used,
                             lambda: _warm_stage(hip, ctx, stage, src, warm_case, case, null, opt),
                             [lambda p=p: _run_stage(hip, ctx, stage, src, p, null, opt, check=False) for p in primers],
                             lambda: _run_stage(hip, ctx, stage, src, case, null, opt, what=what), what)


def test_canny_polygons_keeps_the_chains_in_a_dirty_pg_points(hip):
    """The host form keeps the chains on the device (pg_points) and stages everything else through io[]."""
    used = ("cc_parent", "cc_ws", "ct_ws", "pg_ws", "pg_points", "io0", "io1") + PLANES
    with hip.Context(0) as ctx:
        for g in TARGETS:
            case, warm_case = _Case(g, _frames(g, 100 + g[1] + g[2])), _Case(g, _frames(g, 7000 + g[1]))
            ct, (voff, verts, meas) = _stage_want(hip, "polygons", case, {})
            what = f"canny_polygons {g}"

            def target():
                polygons, got_meas, off, extra = ctx.canny_polygons(case.frames, SIGMA, LO, HI, MIN_AREA,
                                                                    TOLERANCE[0] / 256, TOLERANCE[1] / 65536)
                assert np.array_equal(off, ct[1]) and np.array_equal(extra["point_offsets"], ct[4]), f"{what}: offsets"
                assert np.array_equal(extra["chain_offsets"], ct[2]), f"{what}: chain_offsets"
                assert np.array_equal(extra["vertex_offsets"], voff), f"{what}: vertex_offsets"
                assert np.array_equal(extra["vertices"], verts), f"{what}: vertices"
                assert np.array_equal(got_meas, meas), f"{what}: measures"

            _dirty_cycle(hip, ctx, "leftover", used,
                         lambda: ctx.canny_polygons(warm_case.frames, SIGMA, LO, HI, MIN_AREA, 1.5, 0.01),
                         [lambda p=p: ctx.canny_polygons(p[0], SIGMA, p[1], p[2], MIN_AREA, 1.5, 0.01) for p in _canny_primers()],
                         target, what)


# ---- the core path ----------------------------------------------------------------------------------------------------
CONFIGS = {"defaults": {}, "unfused_classify": {"fuse_classify": 0}, "s16_smoothed": {"smoothed_u8": 0},
           "no_tail": {"hysteresis_tail": 0}, "overlap": {"overlap_hysteresis": 1}, "generic_gaussian": {"gaussian_path": 1}}


def _core_call(ctx, entry, frames, lo, hi):
    """One device-pointer call of the core path on frames [n, h, w]; returns the map as the entry point writes it."""
    n, h, w = frames.shape
    with _Bufs(ctx) as B:
        d_in = B.up(frames)
        if entry == "dev_canny_bits":
            d_out = B.out("map", n * h * ((w + 7) // 8), np.uint8)
            ctx.dev_canny_bits(d_in, SIGMA, lo, hi, h, w, n, d_out)
            return np.unpackbits(B.get("map").reshape(n, h, -1), axis=-1)[..., :w].astype(np.int16) * 255
        if entry == "dev_canny_u8":
            d_out = B.out("map", n * h * w, np.uint8)
            ctx.dev_canny_u8(d_in, SIGMA, lo, hi, h, w, n, d_out)
            return B.get("map").reshape(n, h, w).astype(np.int16)
        d_out = B.out("map", n * h * w, np.int16)
        if entry == "dev_canny_stream":
            ctx.dev_canny_stream(d_in, SIGMA, lo, hi, h, w, n, d_out)
            ctx.dev_canny_stream_flush()
        else:
            ctx.dev_canny(d_in, SIGMA, lo, hi, h, w, n, d_out)
        return B.get("map").reshape(n, h, w)


def _core_targets(n_frames=None):
    for g in TARGETS:
        g = (n_frames or g[0],) + g[1:]
        yield g, "texture", _frames(g, 7000 + g[1]), _frames(g, 100 + g[1] + g[2])
        if g[1:] in (TARGETS[0][1:], TARGETS[2][1:]):
            yield g, "empty", _frames(g, 7000 + g[1]), np.full(g, 90, np.uint8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("entry", ["dev_canny", "dev_canny_u8", "dev_canny_bits"])
def test_dev_canny_forms_on_dirty_workspaces(hip, entry, config, mode):
    """All-ones and all-zero bit-planes, flags and smoothed plane, and the scheduling words (queue entries: leftover only)
    of a denser, larger batch, under every route through dev_canny.  overlap_hysteresis splits a batch of 16 or more:
    17 frames, primer and targets alike."""
    n_frames = 17 if config == "overlap" else None
    primer_g = (n_frames or PRIMER[0],) + PRIMER[1:]
    used = PLANES + (("edges16",) if entry != "dev_canny" else ()) + (("tmp_f32",) if config == "generic_gaussian" else ())
    with hip.Context(0) as ctx:
        for name, value in CONFIGS[config].items():
            ctx.set_option(name, value)
        for g, kind, warm_frames, frames in _core_targets(n_frames):
            what = f"{entry} {config} {g} {kind} {mode}"
            want = _maps(frames)

            def target():
                got = _core_call(ctx, entry, frames, LO, HI)
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} pixels differ from the oracle"

            _dirty_cycle(hip, ctx, mode, used, lambda: _core_call(ctx, entry, warm_frames, LO, HI),
                         [lambda p=p: _core_call(ctx, entry, *p) for p in _canny_primers(primer_g)], target, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("overlap", [0, 1])
def test_dev_canny_stream_on_dirty_workspaces(hip, overlap, mode):
    """Without the tail kernel a streamed call leaves its sweeps in flight; the enumerator refuses to look at the planes
    until they are flushed."""
    used = PLANES
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", 0)
        ctx.set_option("stream_overlap", overlap)
        for g, kind, warm_frames, frames in _core_targets():
            what = f"dev_canny_stream overlap={overlap} {g} {kind} {mode}"
            want = _maps(frames)

            def target():
                got = _core_call(ctx, "dev_canny_stream", frames, LO, HI)
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} pixels differ from the oracle"

            _dirty_cycle(hip, ctx, mode, used, lambda: _core_call(ctx, "dev_canny_stream", warm_frames, LO, HI),
                         [lambda p=p: _core_call(ctx, "dev_canny_stream", *p) for p in _canny_primers()], target, what)
        # a pending batch: the fused route only (width % 8 == 0), and the hook says so instead of reading the planes
        n, h, w = TARGETS[0]
        frames = _frames(TARGETS[0], 31)
        with _Bufs(ctx) as B:
            d_in, d_out = B.up(frames), B.out("map", frames.size, np.int16)
            ctx.dev_canny_stream(d_in, SIGMA, LO, HI, h, w, n, d_out)
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.selftest_workspaces()
            assert ei.value.status == 1
            ctx.dev_canny_stream_flush()
            assert len(ctx.selftest_workspaces()) >= 30
            assert np.array_equal(B.get("map").reshape(frames.shape), _maps(frames))


def _candidates(h, w, seed, density=0.3):
    rng = np.random.default_rng(seed)
    cand = rng.integers(0, 256, size=(h, w), dtype=np.int16)
    cand[rng.random((h, w)) > density] = 0
    return cand


def _host_stage(ctx, entry, frame, seed, lo=LO, hi=HI, cand=None):
    """(got, want) of one host-pointer stage call on a frame (each stage fed with the oracle's plane of the one before)."""
    h, w = frame.shape
    if entry == "gaussian":
        return ctx.gaussian(frame, SIGMA), oracle.gaussian(frame, SIGMA)
    if entry == "canny":
        return ctx.canny(frame, SIGMA, lo, hi), oracle.canny(frame, SIGMA, lo, hi)
    smoothed = oracle.gaussian(frame, SIGMA)
    if entry == "sobel":
        return np.stack(ctx.sobel(smoothed)), np.stack(oracle.sobel(smoothed))
    mag, ang = oracle.sobel(smoothed)
    if entry == "nms":
        return ctx.nms(mag, ang), oracle.nms(mag, ang)
    given, cand = cand, (_candidates(h, w, seed) if cand is None else cand)
    if entry == "hysteresis":
        return ctx.hysteresis(cand, lo, hi), oracle.hysteresis(cand, lo, hi)
    if entry == "dev_hysteresis":
        with _Bufs(ctx) as B:
            d = B.out("cand", cand.size, np.int16)
            ctx.h2d(d, cand)
            ctx.dev_hysteresis(d, h, w, 1, lo, hi)
            return B.get("cand").reshape(h, w), oracle.hysteresis(cand, lo, hi)
    assert entry == "find_edge_pixels"
    small = np.minimum(_candidates(h, w, seed, 0.55) if given is None else cand, 40).astype(np.int16)
    visited = (np.random.default_rng(seed + 1).random((h, w)) < 0.1).astype(np.uint8)
    start = int(np.flatnonzero((small.ravel() >= 10) & (visited.ravel() == 0))[0]) if lo <= 40 else 0
    return np.stack(ctx.find_edge_pixels(small, visited, start, 10, 30)).astype(np.int16), \
        np.stack(oracle.find_edge_pixels(small, visited, start, 10, 30)).astype(np.int16)


HOST_USED = {"gaussian": ("io0", "io1"), "sobel": ("io0", "io1", "io2"), "nms": ("io0", "io1", "io2"),
             "hysteresis": ("io0", "plane_s", "plane_c", "stamps", "flags"),
             "dev_hysteresis": ("plane_s", "plane_c", "stamps", "flags"),
             "find_edge_pixels": ("io0", "io1", "plane_s", "plane_c", "stamps", "flags"),
             "canny": ("io0", "io1") + PLANES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", list(HOST_USED))
def test_stage_calls_on_dirty_workspaces(hip, entry, mode):
    """dev_hysteresis and the host-pointer stage calls, which stage their planes through io[] (one frame per call)."""
    (noise, _, _), (blocks, lo_p, hi_p) = _canny_primers()
    dense = _candidates(*PRIMER[1:], 5, density=0.95)   # at (1, 2) all strong at once, at (1, 250) reached over many sweeps
    with hip.Context(0) as ctx:
        for g in TARGETS:
            h, w = g[1:]
            cases = [("texture", dict(frame=synth_frame(h, w, 100 + h + w), seed=h))]
            if entry in ("hysteresis", "dev_hysteresis") and g in (TARGETS[0], TARGETS[2]):
                corner = np.zeros((h, w), np.int16)
                corner[h - 1, w - 1] = 200
                cases += [("empty", dict(frame=None, seed=0, cand=np.zeros((h, w), np.int16))),
                          ("corner", dict(frame=None, seed=0, cand=corner))]
            if entry in ("canny", "gaussian") and g in (TARGETS[0], TARGETS[2]):
                cases.append(("empty", dict(frame=np.full((h, w), 90, np.uint8), seed=0)))
            for name, kw in cases:
                what = f"{entry} {h}x{w} {name} {mode}"
                if kw["frame"] is None:
                    kw["frame"] = np.zeros((h, w), np.uint8)

                def target():
                    got, want = _host_stage(ctx, entry, **kw)
                    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} values differ from the oracle"

                _dirty_cycle(hip, ctx, mode, HOST_USED[entry], lambda: _host_stage(ctx, entry, synth_frame(h, w, 7000 + h), 77),
                             [lambda: _host_stage(ctx, entry, noise[0], 9, 1, 2, cand=dense),
                              lambda: _host_stage(ctx, entry, blocks[0], 9, lo_p, hi_p, cand=dense)], target, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", ["s16", "u8", "bits"])
def test_canny_batch_on_dirty_cached_pipelines(hip, fmt, mode):
    """Two pipelines of one-frame chunks: pipeline 0 computes on the context itself, pipeline 1 on a sub-context; the
    staging of both and the sub-context's workspaces are listed with a pipeN. prefix and are dirty like the rest."""
    kw = dict(u8=fmt == "u8", bits=fmt == "bits")
    primer_g = (6,) + PRIMER[1:]
    with hip.Context(0) as ctx:
        ctx.set_option("tune_batch_workers", 2)
        ctx.set_option("tune_batch_chunk_frames", 1)
        for g in TARGETS:
            g = (4,) + g[1:]
            frames = _frames(g, 100 + g[1] + g[2])
            want = _maps(frames)
            want = np.packbits(want != 0, axis=-1) if fmt == "bits" else want.astype(np.uint8 if fmt == "u8" else np.int16)
            what = f"canny_batch {fmt} {g} {mode}"
            staging = [f"pipe{p}.slot{s}.{b}" for p in (0, 1) for s in (0, 1) for b in ("d_in", "d_out", "d_out8")]
            used = tuple(staging) + PLANES + tuple("pipe1." + name for name in PLANES)

            def target():
                got = ctx.canny_batch(frames, SIGMA, LO, HI, **kw)
                assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: the maps differ from the oracle"

            _dirty_cycle(hip, ctx, mode, used, lambda: ctx.canny_batch(_frames(g, 7000 + g[1]), SIGMA, LO, HI, **kw),
                         [lambda p=p: ctx.canny_batch(p[0], SIGMA, p[1], p[2], **kw) for p in _canny_primers(primer_g)],
                         target, what)


# ---- colour input and automatic thresholds: gray, hist, thr --------------------------------------------------------------
GRAY_WEIGHTS = (1868, 9617, 4899, 14)   # (wb, wg, wr, shift) of the default rule (OpenCV's)


def _gray(rgb):
    wb, wg, wr, s = GRAY_WEIGHTS
    c = rgb.astype(np.uint32)
    return ((wb * c[..., 2] + wg * c[..., 1] + wr * c[..., 0] + (1 << (s - 1))) >> s).astype(np.uint8)


def _rgb(g, seed):
    return np.stack([_frames(g, seed + 50 * k) for k in range(3)], axis=-1)


@pytest.mark.parametrize("mode", MODES)
def test_dev_canny_color_through_the_dirty_gray_plane(hip, mode):
    """fuse_gray 0: the standalone conversion writes the gray workspace and the gray path runs on it."""
    used = ("gray",) + PLANES
    with hip.Context(0) as ctx:
        ctx.set_option("fuse_gray", 0)

        def call(rgb, lo, hi):
            n, h, w = rgb.shape[:3]
            with _Bufs(ctx) as B:
                d_out = B.out("map", n * h * w, np.int16)
                ctx.dev_canny_color(B.up(rgb), hip.LAYOUT_RGB8, SIGMA, lo, hi, h, w, n, d_out)
                return B.get("map").reshape(n, h, w)

        for g in TARGETS:
            rgb = _rgb(g, 100 + g[1])
            want = _maps(_gray(rgb))
            what = f"dev_canny_color {g} {mode}"

            def target():
                got = call(rgb, LO, HI)
                assert ctx.get_option("last_canny_fused_gray") == 0
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} pixels differ from the oracle"

            _dirty_cycle(hip, ctx, mode, used, lambda: call(_rgb(g, 7000 + g[1]), LO, HI),
                         [lambda p=p: call(*p) for p in _canny_primers(colour=True)], target, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("thresholds_out", [True, False], ids=["pairs_returned", "pairs_null"])
@pytest.mark.parametrize("rule,low,high", [("median", 0.67, 1.33), ("quantile", 0.7, 0.9)])
def test_dev_canny_auto_on_dirty_histograms(hip, rule, low, high, thresholds_out, mode):
    """The histograms are summed with atomics into hist, which only the memset in front of them makes zero; without a
    caller's array the selected pairs live in thr."""
    used = ("hist",) + (() if thresholds_out else ("thr",)) + PLANES
    # The rules choose the primers' thresholds themselves, and at those the weak chains are no candidates: nothing is
    # scheduled.  A plain dev_canny of the chains at (1, 150) therefore runs last; it leaves hist and thr as they are.
    chains = _canny_primers()[1]
    with hip.Context(0) as ctx:

        def call(frames):
            n, h, w = frames.shape
            with _Bufs(ctx) as B:
                d_out = B.out("map", frames.size, np.int16)
                d_thr = B.out("pairs", 2 * n, np.int32) if thresholds_out else 0
                ctx.dev_canny_auto(B.up(frames), SIGMA, rule, low, high, h, w, n, d_out, d_thr)
                return B.get("map").reshape(frames.shape), (B.get("pairs").reshape(n, 2) if thresholds_out else None)

        for g in TARGETS:
            frames = _frames(g, 100 + g[1] + g[2])
            frames[-1] = (frames[-1] * 0.4 + 60).astype(np.uint8)   # another contrast: another pair
            what = f"dev_canny_auto {rule} {g} {mode}"
            pairs = []
            for f in frames:
                st = oracle.canny(f, SIGMA, 1, 1, stages=True)
                plane = st["smoothed"] if rule == "median" else np.minimum(st["magnitude"], 256)
                pairs.append(hist_rule.np_rule(np.bincount(plane.ravel().astype(np.int64), minlength=257), rule, low, high))
            want = np.stack([oracle.canny(f, SIGMA, *p) for f, p in zip(frames, pairs)])

            def target():
                got, got_pairs = call(frames)
                if thresholds_out:
                    assert got_pairs.tolist() == [list(p) for p in pairs], f"{what}: the selected pairs"
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} pixels differ from the oracle"

            _dirty_cycle(hip, ctx, mode, used, lambda: call(_frames(g, 7000 + g[1])),
                         [lambda p=p: call(p[0]) for p in _canny_primers()] + [lambda: _core_call(ctx, "dev_canny", *chains)],
                         target, what)


# ---- the stages share cc_parent, cc_ws, points, edges16 and io[] ---------------------------------------------------------
def test_stages_in_one_order_and_its_reverse_on_one_context(hip):
    order = [(stage, src, null) for stage in STAGES for src, null in (("canny", True), ("bits", False))]
    g = TARGETS[3]
    case, big = _Case(g, _frames(g, 100 + g[1] + g[2])), _Case(TARGETS[4], _frames(TARGETS[4], 100 + 200 + 360))
    with hip.Context(0) as ctx:
        for stage, src, null in order + order[::-1]:
            opt = STAGES[stage][3]
            ctx.set_option("hough_path", opt.get("hough_path", 0))
            # a larger batch first, so that the stage before and the stage after work in each other's leftovers
            _run_stage(hip, ctx, stage, src, big, null, opt, what=f"{stage} {src} {big.g} in a chain of stages")
            _run_stage(hip, ctx, stage, src, case, null, opt, what=f"{stage} {src} {g} in a chain of stages")


# ---- the one workspace that is meant to survive: the vote tables, with their key -------------------------------------------
A = dict(rho=1.0, theta=PI / 180, lo=0.0, hi=PI, g=TARGETS[3])
CACHE_PAIRS = {"rho": dict(A, rho=2.0), "theta": dict(A, theta=PI / 90), "min_theta": dict(A, lo=PI / 180, hi=PI),
               "shape": dict(A, g=(2, 130, 72))}
# (min_theta: one step further, so numangle stays 180 - 1 and only the table's first entry moves; shape: same rho, theta and
# min_theta, hence the same table -- only numrho changes)


@pytest.mark.parametrize("differs", list(CACHE_PAIRS))
@pytest.mark.parametrize("stage", ["lines_lds", "segments"])
def test_vote_table_cache_follows_every_part_of_its_key(hip, stage, differs):
    b = CACHE_PAIRS[differs]
    with hip.Context(0) as ctx:
        for k, p in enumerate((A, b, A, b)):
            case = _Case(p["g"], _frames(p["g"], 100 + p["g"][1] + p["g"][2]))
            opt = dict(STAGES[stage][3], hough=(p["rho"], p["theta"], p["lo"], p["hi"]))
            for src in ("bits", "canny"):
                _run_stage(hip, ctx, stage, src, case, False, opt, what=f"{stage} {src} call {k} of A B A B, {differs} differs")


# ---- the 8-row patch finalize (tune_finalize_mode 1), reachable through the ABI and never run ------------------------------
FINALIZE_SHAPES = [(2, 2), (2, 9), (9, 2), (3, 3), (5, 7), (16, 16), (31, 33), (64, 64), (65, 63), (97, 131), (128, 192),
                   (200, 257), (240, 320), (1, 1), (1, 70), (70, 1), (63, 129), (129, 65), (100, 200), (37, 77)]


@pytest.mark.parametrize("lohi", [(50, 150), (1, 2), (10, 10), (0, 1), (100, 300), (200, 100)])
@pytest.mark.parametrize("shape", FINALIZE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hysteresis_with_the_patch_finalize(hip, shape, lohi):
    """The shapes and pairs of test_hysteresis_parity, then a width that is a multiple of 8 (100 x 200) and one that is not
    (37 x 77): launch_hyst_finalize takes the patch kernel only for the former.  The switch is process-wide."""
    h, w = shape
    lo, hi = lohi
    rng = np.random.default_rng(9)
    with hip.Context(0) as ctx:
        ctx.set_option("tune_finalize_mode", 1)
        try:
            for density in (0.05, 0.3, 0.9):
                cand = rng.integers(0, 256, size=(h, w), dtype=np.int16)
                cand[rng.random((h, w)) > density] = 0
                assert np.array_equal(ctx.hysteresis(cand, lo, hi), oracle.hysteresis(cand, lo, hi)), (shape, lohi, density)
        finally:
            ctx.set_option("tune_finalize_mode", 0)
