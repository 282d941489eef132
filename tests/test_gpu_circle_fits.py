"""Sub-pixel circle fits on the GPU (canny_hip_dev_canny_hough_circle_fits, canny_hip_dev_circle_fits_bits,
canny_hip_canny_hough_circle_fits, canny_hip_dev_circle_fits_arith) against tests/circle_fits_rule.py
applied to the oracle's map and the oracle's smoothed plane, behind tests/hough_circles_rule.py.  Every comparison is exact
equality on whole arrays; every output buffer is sentinel-filled with guard words behind it, and every case checks that
the slots past the count are untouched."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import circle_fits_rule as cf
import oracle
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
SIGMA, LO, HI = 1.0, 50, 150
MIN_R, MAX_R, THRESHOLD, SUPPORT, MIN_DIST, CENTRES_MAX = 5, 45, 20, 15, 10, 16


class _Bufs:
    """Sentinel-filled device arrays of uint32 words with guard words behind them."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.words = ctx, [], {}

    def filled(self, words):
        p = self.ctx.malloc(4 * (words + N_GUARD))
        self.ptrs.append(p)
        self.words[p] = words
        self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def get(self, p, what=""):
        out = np.empty(self.words[p] + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[self.words[p]:] == SENT).all(), f"guard words overwritten {what}"
        return out[:self.words[p]]

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


# ---- the reference: oracle map and plane, then the two rules; every stage computed once and never modified --------------
def disks(h, w, *spec):
    """A frame of blurred bright disks (cx, cy, R) on the dark ground; the brightest wins where two overlap."""
    out = np.full((h, w), 40, np.uint8)
    for cx, cy, R in spec:
        out = np.maximum(out, cf.disk_plane(h, w, cx, cy, R))
    return out


def _wide(h, w):
    return [disks(h, w, (40.25, 48.4, 20.3), (100.5, 20.2, 8.3)), np.full((h, w), 90, np.uint8), disks(h, w, (63.6, 47.9, 30.7))]


def _narrow(h, w):
    return [disks(h, w, (30.25, 48.4, 20.3), (62.5, 20.2, 8.3)), np.full((h, w), 90, np.uint8), disks(h, w, (38.6, 47.9, 30.7))]


def _tall(h, w):
    return [disks(h, w, (48.3, 120.4, 14.6), (30.2, 40.7, 22.4))]


KINDS = {"wide": _wide, "narrow": _narrow, "tall": _tall}
_FRAMES, _RECS, _FITS = {}, {}, {}


def frames_of(key):
    """key = (h, w, kind): (frames, masks, planes)."""
    if key not in _FRAMES:
        h, w, kind = key
        frames = np.stack(KINDS[kind](h, w))
        masks = np.stack([oracle.canny(f, SIGMA, LO, HI) != 0 for f in frames])
        planes = [oracle.gaussian(f, SIGMA) for f in frames]
        for a in (frames, masks, *planes):
            a.setflags(write=False)
        _FRAMES[key] = (frames, masks, planes)
    return _FRAMES[key]


def want_of(key, cell_shift, band, trim_q8, options, centres_max=CENTRES_MAX):
    """Per frame (circle records, fits) by the rules.  centres_max cuts the CANDIDATE list of the circle rule, so the
    reference is always computed with the capacity of the call it is compared with."""
    full = (key, cell_shift, band, trim_q8, options, centres_max)
    if full not in _FITS:
        _, masks, planes = frames_of(key)
        out = []
        for f, (m, P) in enumerate(zip(masks, planes)):
            rk = (key, cell_shift, f, centres_max)
            if rk not in _RECS:
                _RECS[rk] = cf.hough_records(m, P, MIN_R, MAX_R, cell_shift, THRESHOLD, SUPPORT, MIN_DIST, centres_max)
            out.append((_RECS[rk], cf.fits_of(m, P, _RECS[rk], band, trim_q8, options)))
        _FITS[full] = out
    return _FITS[full]


def run_fits(ctx, b, d_img, n, h, w, cell_shift, band, trim_q8, options, centres_max, hi=HI, own_records=False):
    """One guarded dev_canny_hough_circle_fits call -> (records [n, max, 6], counts [n], fits [n, max, 8]), uint32."""
    d_rec, d_cnt, d_fit = b.filled(n * centres_max * 6), b.filled(n), b.filled(n * centres_max * 8)
    ctx.dev_canny_hough_circle_fits(d_img, SIGMA, LO, hi, h, w, n, MIN_R, MAX_R, cell_shift, THRESHOLD, SUPPORT, MIN_DIST,
                                    centres_max, band, trim_q8, options, d_fit, 0 if own_records else d_rec, d_cnt)
    return (b.get(d_rec, "behind the records").reshape(n, centres_max, 6), b.get(d_cnt).view(np.int32),
            b.get(d_fit, "behind the fits").reshape(n, centres_max, 8))


def check(got, want, centres_max, what="", own_records=False):
    rec, cnt, fit = got
    for f, (wrec, wfit) in enumerate(want):
        k = len(wrec)
        assert cnt[f] == k <= centres_max, f"{what} frame {f}: {cnt[f]} circles, the rule has {k}"
        if not own_records:
            assert np.array_equal(rec[f, :k].view(np.int32), wrec[:k]), f"{what} frame {f}: records differ"
        else:
            assert (rec[f] == SENT).all()
        bad = np.flatnonzero((fit[f, :k].view(np.int32) != wfit[:k]).any(axis=1))
        assert bad.size == 0, (f"{what} frame {f}: {bad.size} of {k} fits differ, first {bad[0]} (circle {wrec[bad[0]]}): "
                               f"{fit[f, bad[0]].view(np.int32)} != {wfit[bad[0]]}")
        assert (fit[f, k:] == SENT).all() and (own_records or (rec[f, k:] == SENT).all()), f"{what} frame {f}: slots past the count written"


SWEEP = list(itertools.product((0, 1, 4), (0, 64), range(4), (0, 1)))  # band, trim_q8, options, cell_shift: 48


# ---- routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("h,w,kind", [(96, 128, "wide"), (96, 77, "narrow")], ids=["96x128", "96x77"])
def test_behind_the_circles_equals_the_rule_on_the_oracles_planes(hip, h, w, kind, u8, fuse, tail):
    """Two blurred-disk frames around an empty one; the big disks cross the row-64 boundary of the strong plane's tiles."""
    key = (h, w, kind)
    frames, masks, planes = frames_of(key)
    assert masks[0].any() and masks[2].any() and not masks[1].any()
    route = 4 * u8 + 2 * fuse + tail
    with hip.Context(0) as ctx:
        ctx.set_option("smoothed_u8", u8)
        ctx.set_option("fuse_classify", fuse)
        ctx.set_option("hysteresis_tail", tail)
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        for band, trim_q8, options, cell_shift in SWEEP[route::8]:  # six combinations per route, all 48 over the routes
            want = want_of(key, cell_shift, band, trim_q8, options)
            most = max(len(x[0]) for x in want)
            assert most >= 1 and len(want[1][0]) == 0
            assert any(r[1] - 2 * r[2] < 128 < r[1] + 2 * r[2] for x in want for r in x[0].tolist()), "no circle through row 64"
            check(run_fits(ctx, b, d_img, 3, h, w, cell_shift, band, trim_q8, options, CENTRES_MAX), want, CENTRES_MAX,
                  f"band {band} trim {trim_q8} options {options} shift {cell_shift}")
        assert ctx.get_option("last_canny_smoothed_u8") == (1 if u8 and fuse and w % 8 == 0 else 0)
        b.free()


def test_parameter_sweep_and_capacities(hip):
    key = (96, 128, "wide")
    frames, masks, planes = frames_of(key)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        for band, trim_q8, options, cell_shift in SWEEP:
            want = want_of(key, cell_shift, band, trim_q8, options)
            most = max(len(x[0]) for x in want)
            assert 2 <= most < CENTRES_MAX
            check(run_fits(ctx, b, d_img, 3, 96, 128, cell_shift, band, trim_q8, options, CENTRES_MAX), want, CENTRES_MAX,
                  f"band {band} trim {trim_q8} options {options} shift {cell_shift}")
        # the invariant of the issue: band 0, options 0, no trim: n == support, for every record the circle call produced
        for cell_shift in (0, 1):
            for rec, fit in want_of(key, cell_shift, 0, 0, 0):
                assert np.array_equal(fit[:, 3], rec[:, 4])
        # capacity: exact (every slot of the fullest frame filled), one short and 1
        most = max(len(x[0]) for x in want_of(key, 0, 1, 64, 2))
        assert most >= 2
        for cap in sorted({most, most - 1, 1}, reverse=True):
            want = want_of(key, 0, 1, 64, 2, cap)
            if cap == most:
                assert max(len(x[0]) for x in want) == cap, "no frame fills every slot"
            check(run_fits(ctx, b, d_img, 3, 96, 128, 0, 1, 64, 2, cap), want, cap, f"centres_max {cap}")
        # the records in the context's workspace: the caller's record buffer stays untouched, the fits are the same
        check(run_fits(ctx, b, d_img, 3, 96, 128, 0, 1, 0, 2, CENTRES_MAX, own_records=True), want_of(key, 0, 1, 0, 2),
              CENTRES_MAX, "own records", own_records=True)
        b.free()


def test_a_circle_through_row_128(hip):
    key = (140, 96, "tall")
    frames, masks, planes = frames_of(key)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        for band, trim_q8, options in ((1, 0, 2), (4, 64, 0), (0, 0, 0)):
            want = want_of(key, 0, band, trim_q8, options)
            assert any(r[1] - 2 * r[2] < 256 < r[1] + 2 * r[2] for r in want[0][0].tolist()), "no circle through row 128"
            check(run_fits(ctx, b, d_img, 1, 140, 96, 0, band, trim_q8, options, CENTRES_MAX), want, CENTRES_MAX)
        b.free()


# ---- device bit maps, caller's planes, caller-made records ------------------------------------------------------------------
def run_bits(ctx, b, masks, planes, lists, band, trim_q8, options, centres_max, d_plane=None):
    """dev_circle_fits_bits on caller-made arrays: lists = per frame circle records.  -> fits [n, centres_max, 8]."""
    n, (h, w) = len(masks), masks[0].shape
    recs = np.full((n, centres_max, 6), 0x7FFFFFF0, np.int32)  # unused slots hold records that must never be read
    cnt = np.zeros(n, np.int32)
    for f, r in enumerate(lists):
        recs[f, :min(len(r), centres_max)], cnt[f] = r[:centres_max], len(r)
    d_bits = b.upload(np.stack([np.packbits(m, axis=-1) for m in masks]))
    if d_plane is None:
        d_plane = b.upload(np.stack(planes))
    d_fit = b.filled(n * centres_max * 8)
    ctx.dev_circle_fits_bits(d_bits, d_plane, planes[0].dtype == np.uint8, n, h, w, b.upload(recs), b.upload(cnt), centres_max,
                             band, trim_q8, options, d_fit)
    return b.get(d_fit, "behind the fits").reshape(n, centres_max, 8)


def check_bits(got, masks, planes, lists, band, trim_q8, options, what=""):
    for f, (m, P, recs) in enumerate(zip(masks, planes, lists)):
        want = cf.fits_of(m, P, recs, band, trim_q8, options)
        bad = np.flatnonzero((got[f, :len(recs)].view(np.int32) != want).any(axis=1))
        assert bad.size == 0, (f"{what} band {band} trim {trim_q8} options {options} frame {f}: {bad.size} differ, first "
                               f"{recs[bad[0]]}: {got[f, bad[0]].view(np.int32)} != {want[bad[0]]}")
        assert (got[f, len(recs):] == SENT).all(), f"{what} frame {f}: slots past the count written"


def made(*rows):
    return np.array([list(r) + [0, 0, 0] for r in rows], np.int32)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_bits_form_on_the_cpu_tests_drawn_masks(hip, dtype):
    rng = np.random.default_rng(5)
    full = np.iinfo(dtype)
    h, w = 97, 161
    kinds = cf.mask_kinds(h, w, 5)
    masks = [kinds[k] for k in ("rings", "empty", "arcs", "twin", "crossed", "random")]
    planes = [rng.integers(full.min, full.max + 1, (h, w)).astype(dtype) for _ in masks]
    planes[3] = (cf.disk_plane(h, w, w / 2.0 + 0.25, h / 2.0 - 0.25, min(h, w) * 0.4).astype(np.int32) * (1 if dtype == np.uint8 else 100)).astype(dtype)
    s, cx2, cy2 = min(h, w), 2 * (w // 2) + 1, 2 * (h // 2) - 1
    lists = []
    for m, P in zip(masks, planes):
        hough = cf.hough_records(m, P, 3, 45, 0, 2, 3, 4, 4)
        lists.append(np.concatenate([hough, made((cx2, cy2, int(s * 0.4)), (cx2, cy2, int(s * 0.2)), (4, cy2, int(s * 0.2)),
                                                 (2 * w - 6, 2 * h - 6, int(s * 0.4)), (0, 0, 1), (2 * w - 1, 2 * h - 1, 1024),
                                                 (cx2, cy2, 0), (cx2, cy2, 1025), (-1, cy2, 5), (2 * w, cy2, 5), (cx2, -1, 5),
                                                 (cx2, 2 * h, 5), (2 ** 31 - 1, -2 ** 31, 5))]).astype(np.int32))
    most = max(len(r) for r in lists)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for band, trim_q8, options in ((0, 0, 0), (1, 64, 2), (2, 0, 1), (4, 128, 3), (3, 64, 0)):
            got = run_bits(ctx, b, masks, planes, lists, band, trim_q8, options, most + 2)
            check_bits(got, masks, planes, lists, band, trim_q8, options, "drawn masks")
            f0 = got[0, :len(lists[0])].view(np.int32)
            assert (f0[-7:, 4].view(np.uint32) == cf.INVALID).all() and not f0[-7:, [0, 1, 2, 3, 5, 6, 7]].any()
            assert np.array_equal(f0, hip.circle_fits_from_plane(np.packbits(masks[0], axis=-1), planes[0], lists[0], band,
                                                                 trim_q8, options)), "the host function differs"
        b.free()


def test_bits_form_where_the_row_walk_can_slip(hip):
    """All-set and ring maps on a random plane, caller-made records: a centre 2 px from each border in turn; rings of
    radius 3 to 5 whose two intervals share a bit word; intervals that start at bit 0 and end at bit 31 and bit 63 of a
    word; width 77 with its partial last word; the smallest radius; a centre on the last pixel."""
    rng = np.random.default_rng(9)
    for h, w in ((60, 200), (61, 77)):
        P = rng.integers(0, 256, (h, w)).astype(np.uint8)
        full = np.ones((h, w), bool)
        rings = np.zeros((h, w), bool)
        for cx, cy, r in ((2, h // 2, 12), (w - 3, h // 2, 12), (w // 2, 2, 12), (w // 2, h - 3, 12), (20, 20, 3), (40, 20, 4),
                          (70, 40, 5), (w - 6, 8, 5)):
            rings |= cf.ring(h, w, cx, cy, r)
        recs = [(4, h, 12), (2 * w - 6, h, 12), (w, 4, 12), (w, 2 * h - 6, 12),          # 2 px from each border
                (40, 40, 3), (80, 40, 4), (140, 80, 5), (2 * w - 12, 16, 5), (41, 41, 3),  # both intervals in one word
                (2 * (64 + 11), 60, 10), (2 * (63 - 11), 60, 10), (2 * (31 - 11), 60, 10),  # band 1: from bit 0, to bit 63, 31
                (2 * (w - 1 - 11), 60, 10), (2 * (w - 1), 2 * (h - 1), 7), (0, 0, 1), (1, 1, 1), (w, h, 1)]
        recs = made(*[r for r in recs if 0 <= r[0] < 2 * w])
        with hip.Context(0) as ctx:
            b = _Bufs(ctx)
            for band, trim_q8, options in ((1, 0, 0), (0, 0, 0), (4, 64, 2), (2, 128, 1)):
                for m in (full, rings):
                    got = run_bits(ctx, b, [m, m[::-1].copy()], [P, P], [recs, recs[:5]], band, trim_q8, options, len(recs))
                    check_bits(got, [m, m[::-1].copy()], [P, P], [recs, recs[:5]], band, trim_q8, options, f"{h}x{w}")
            b.free()
        # the word edges are what they claim to be: on the all-set map the centre row's pixels of band 1
        if w == 200:
            for x2, first, last in ((2 * 75, 64, 86), (2 * 52, 41, 63), (2 * 20, 9, 31)):
                idx = cf.band_pixels(full, (x2, 60, 10), 1)
                xs = idx[idx // w == 30] % w
                assert xs.min() == first and xs.max() == last


def test_more_pixels_than_the_queue_holds(hip):
    h = w = 200
    rng = np.random.default_rng(11)
    full = np.ones((h, w), bool)
    recs = made((200, 200, 90), (201, 199, 60), (200, 200, 20))
    capacity = hip.circle_fits_queue_capacity()
    assert len(cf.band_pixels(full, recs[0], 4)) > capacity >= len(cf.band_pixels(full, recs[2], 4)), capacity
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for dtype in (np.uint8, np.int16):
            info = np.iinfo(dtype)
            P = rng.integers(info.min, info.max + 1, (h, w)).astype(dtype)
            for band, trim_q8, options in ((4, 0, 0), (4, 64, 0), (4, 128, 2)):
                got = run_bits(ctx, b, [full], [P], [recs], band, trim_q8, options, 4)
                check_bits(got, [full], [P], [recs], band, trim_q8, options, f"overflow {dtype.__name__}")
                assert got[0, 0, 3] > (capacity if not options and not trim_q8 else 100)
        b.free()


def test_bits_form_statuses_and_the_contexts_own_plane(hip):
    key = (96, 128, "wide")
    frames, masks, planes = frames_of(key)
    want = want_of(key, 0, 1, 64, 3)
    lists = [x[0] for x in want]
    most = max(len(r) for r in lists)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        # a fresh context has no plane to offer: INVALID, nothing written; neither has one that ran another shape
        for first in (None, frames[:, :64, :64].copy()):
            if first is not None:
                ctx.canny_points(first, SIGMA, LO, HI)
            with pytest.raises(hip.CannyHipError) as ei:
                run_bits(ctx, b, masks, planes, lists, 1, 64, 3, most, d_plane=0)
            assert ei.value.status == 1
            assert all((b.get(p) == SENT).all() for p in b.words)
        d_img = b.upload(frames)
        d_out = b.filled(frames.size // 2)
        ctx.dev_canny(d_img, SIGMA, LO, HI, 96, 128, 3, d_out)
        got = run_bits(ctx, b, masks, planes, lists, 1, 64, 3, most + 1, d_plane=0)
        for f, (rec, fit) in enumerate(want):
            assert np.array_equal(got[f, :len(rec)].view(np.int32), fit) and (got[f, len(rec):] == SENT).all()
        # statuses: nothing is written
        d_fit = b.filled(64)
        d_any = b.upload(np.zeros(4096, np.uint32))
        ok = dict(d_bits=d_any, n=1, h=40, w=64, d_rec=d_any, d_cnt=d_any, cmax=4, band=1, trim=0, options=0, d_fits=d_fit)
        for kw, status in ((dict(options=4), 1), (dict(options=-1), 1), (dict(d_fits=d_fit + 4), 1), (dict(d_fits=0), 1),
                           (dict(d_rec=0), 1), (dict(d_cnt=0), 1), (dict(d_bits=0), 1), (dict(cmax=0), 1), (dict(band=-1), 1),
                           (dict(trim=-1), 1), (dict(h=1, w=2048), 1), (dict(band=5), 2), (dict(h=2, w=16385), 2),
                           (dict(h=16385, w=2), 2)):
            a = dict(ok)
            a.update(kw)
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_circle_fits_bits(a["d_bits"], d_any, True, a["n"], a["h"], a["w"], a["d_rec"], a["d_cnt"], a["cmax"],
                                         a["band"], a["trim"], a["options"], a["d_fits"])
            assert ei.value.status == status, kw
            assert (b.get(d_fit) == SENT).all(), kw
        b.free()


# ---- determinism on a long-lived context -------------------------------------------------------------------------------------
def test_same_bytes_on_every_run_on_a_context_with_dirty_workspaces(hip):
    key = (96, 128, "wide")
    frames, masks, planes = frames_of(key)
    want = want_of(key, 0, 1, 64, 2)
    cap = CENTRES_MAX
    other = np.stack([synth_frame(96, 200, s) for s in (5, 6, 7, 8)])
    with hip.Context(0) as ctx:
        ctx.canny_hough_line_fits(other, 1.4, LO, HI, threshold=20, lines_max=16, min_length=8, max_gap=2, segments_max=64)
        ctx.canny_hough_circles(other, 1.4, LO, HI, 5, 30, threshold=15, support_threshold=10, min_dist=8, centres_max=32)
        ctx.canny_edgels(other, 1.0, 20, 60)
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        ctx.profile_enable(True)
        ctx.profile_reset()
        runs = []
        for _ in range(3):
            got = run_fits(ctx, b, d_img, 3, 96, 128, 0, 1, 64, 2, cap)
            check(got, want, cap)
            runs.append(tuple(a.tobytes() for a in got))
        assert runs[0] == runs[1] == runs[2]
        ms, launches = ctx.circle_fits_profile_get(hip.CIRCLE_FIT_PART_FIT)
        assert launches == 3 and ms > 0.0
        assert ctx.hough_circles_profile_get(0)[1] == 3 and ctx.line_fits_profile_get(0)[1] == 0
        ctx.profile_enable(False)
        with pytest.raises(hip.CannyHipError):
            ctx.circle_fits_profile_get(1)
        # max_val > 255 empties the map: no circle, no fit
        rec, cnt, fit = run_fits(ctx, b, d_img, 3, 96, 128, 0, 1, 64, 2, cap, hi=300)
        assert not cnt.any() and (fit == SENT).all() and (rec == SENT).all()
        b.free()


# ---- the device arithmetic ------------------------------------------------------------------------------------------------
def test_device_finishing_arithmetic(hip):
    """The designed sets of the CPU test (limits of the sums, Suz past 64 bits, determinants at and beside 0, moves at and
    beyond the limit, halves, the largest shift) against Python ints, and 2^16 random point sets against the int64
    restatement, which the CPU test pins to the Python ints."""
    designed = cf.designed_moments()
    want_d = cf.finish_words(designed)
    rnd = cf.random_moments(np.random.default_rng(29), 1 << 16)
    want_r = cf.finish_np(rnd)
    sample = slice(0, 1 << 16, 499)
    assert np.array_equal(want_r[sample], cf.finish_words([tuple(x) for x in rnd[sample].tolist()]))
    packed_r = np.zeros((len(rnd), cf.MOMENT_WORDS), np.int64)
    packed_r[:, :7], packed_r[:, 7], packed_r[:, 8] = rnd[:, :7], rnd[:, 7], rnd[:, 7] >> 63
    packed_r[:, 9], packed_r[:, 10], packed_r[:, 11] = rnd[:, 8], rnd[:, 8] >> 63, rnd[:, 9]
    assert np.array_equal(packed_r[sample], cf.pack_moments([tuple(x) for x in rnd[sample].tolist()]))
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for sets, want in ((cf.pack_moments(designed), want_d), (packed_r, want_r)):
            d_out = b.filled(4 * len(sets))
            ctx.dev_circle_fits_arith(b.upload(sets), len(sets), d_out)
            got = b.get(d_out).view(np.int32).reshape(-1, 4)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"{bad.size} sets differ, first {bad[0]}: {sets[bad[0]]} -> {got[bad[0]]} != {want[bad[0]]}"
            assert np.array_equal(hip.circle_fits_finish(sets[:4096]), want[:4096])
        with pytest.raises(hip.CannyHipError):
            ctx.dev_circle_fits_arith(0, 4, d_out)
        b.free()


# ---- host buffers and the command line -----------------------------------------------------------------------------------
def test_host_buffer_form_equals_the_rule(hip):
    key = (96, 77, "narrow")
    frames, masks, planes = frames_of(key)
    with hip.Context(0) as ctx:
        for cell_shift, band, trim_q8, options in ((0, 1, 0, 2), (1, 4, 64, 3), (0, 0, 0, 0)):
            want = want_of(key, cell_shift, band, trim_q8, options)
            recs, counts, peaks, fits = ctx.canny_hough_circle_fits(frames, SIGMA, LO, HI, MIN_R, MAX_R, cell_shift, THRESHOLD,
                                                                    SUPPORT, MIN_DIST, CENTRES_MAX, band, trim_q8, options)
            for f, (wrec, wfit) in enumerate(want):
                assert counts[f] == len(wrec) and np.array_equal(recs[f], wrec) and np.array_equal(fits[f], wfit)
        u = hip.circle_fits_unpack(fits[0])  # band 0, every pixel of the bin: the small disk's ring leaves sectors empty
        assert (u["n"] >= 16).all() and (u["sector_count"] >= 8).all() and not u["degenerate"].any()


def test_cli_writes_the_circle_fits_of_a_frame(hip, tmp_path):
    key = (96, 128, "wide")
    frames, masks, planes = frames_of(key)
    pgm = tmp_path / "in.pgm"
    pgm.write_bytes(b"P5\n%d %d\n255\n" % (128, 96) + frames[0].tobytes())
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, str(SIGMA), str(LO), str(HI), "-i", str(pgm), "-o", str(tmp_path), "-r",
                        f"{MIN_R},{MAX_R},{THRESHOLD},{SUPPORT},{MIN_DIST}", "-k", "1,64,2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    m, P = masks[0], planes[0]
    rec = cf.hough_records(m, P, MIN_R, MAX_R, 0, THRESHOLD, SUPPORT, MIN_DIST, 256)
    fit = cf.fits_of(m, P, rec, 1, 64, 2)
    cx, cy, rad, n, maxd, rms, _, failed, deg, _ = cf.unpack(fit)
    rows = (tmp_path / "canny_circle_fits.txt").read_text().splitlines()
    want = ["0 %.4f %.4f %.4f %d %.4f %.4f %04x %d %d" % (cx[j], cy[j], rad[j], n[j], rms[j], maxd[j], fit[j, 5] & 0xFFFF,
                                                           failed[j], deg[j]) for j in range(len(fit))]
    assert rows == want and len(rows) >= 2
    assert (tmp_path / "canny_circles.txt").read_text().splitlines() == [
        "0 %.1f %.1f %d %d %d" % (c[0] * 0.5, c[1] * 0.5, c[2], c[3], c[4]) for c in rec]
