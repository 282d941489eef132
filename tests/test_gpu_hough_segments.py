"""Hough line segments on the GPU (canny_hip_dev_hough_segments_bits / canny_hip_dev_canny_hough_segments /
canny_hip_canny_hough_segments) against the numpy restatement of the rule (tests/hough_segments_rule.py), which looks at
the FULL plane for every line -- the kernels search a window around the line, so this is also the proof that the window
loses nothing (rho 0.5 and 2.5 included) -- and against the library's own host walk.  The numpy side is fed with the
library's vote tables and with the bases the device's Hough call left behind.  Every comparison is exact equality on whole
arrays; every output buffer is pre-filled with a sentinel and followed by a guard region."""
import os
import subprocess

import numpy as np
import pytest

import hough_rule as hr
import hough_segments_rule as sr
from canny_edge_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = float(np.pi)
SENT = 0xA5A5A5A5
N_GUARD = 64
LINES = 12


class _Dev:
    """Device buffers of one context, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def filled(self, words):
        p = self.malloc(4 * (words + N_GUARD))
        self.fill(p, words)
        return p

    def fill(self, p, words):
        self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def get(self, p, words, what):
        out = np.empty(words + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[words:] == SENT).all(), f"{what}: guard overwritten"
        return out[:words]

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def _check_frames(got_seg, got_cnt, want, cap, what):
    """got_seg uint32 [n, cap, 6], got_cnt [n]; want: the rule's records per frame."""
    for f, w in enumerate(want):
        k = min(cap, len(w))
        assert int(got_cnt[f]) == len(w), f"{what} frame {f}: count {int(got_cnt[f])} != {len(w)}"
        assert np.array_equal(got_seg[f, :k].view(np.int32), w[:k]), f"{what} frame {f}: records differ"
        assert (got_seg[f, k:] == SENT).all(), f"{what} frame {f}: slots past the count were written"


@pytest.mark.parametrize("rho", sr.RHOS)
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_segments_equal_the_rule_and_the_host_walk(hip, shape, rho):
    h, w = shape
    kinds = sr.mask_kinds(h, w, seed=h * 31 + w)
    batches = [np.stack([kinds["all"]]), np.stack([kinds["drawn"], kinds["empty"], kinds["random"]])]  # no lines in the middle
    with hip.Context(0) as ctx:
        dev = _Dev(ctx)
        for masks in batches:
            n = len(masks)
            bits = np.packbits(masks, axis=-1)
            d_bits = dev.upload(bits)
            d_bases, d_counts = dev.filled(n * LINES), dev.filled(n)
            for theta, lo, hi in sr.ANGLES:
                numangle, numrho = hip.hough_geometry(h, w, rho, theta, lo, hi)
                tabs = hip.hough_tables(rho, theta, lo, numangle)
                dev.fill(d_bases, n * LINES)
                ctx.dev_hough_bits(d_bits, n, h, w, rho, theta, 0, LINES, lo, hi, 0, 0, d_bases, d_counts)
                bases = dev.get(d_bases, n * LINES, "bases").reshape(n, LINES)
                counts = dev.get(d_counts, n, "line counts").view(np.int32)
                lines = []
                for f in range(n):  # the lines are the rule's own peaks, and some frame has more of them than lines_max
                    acc = hr.accumulate(np.flatnonzero(masks[f]), w, numrho, *tabs)
                    wb = hr.peaks(acc, 0)[0]
                    assert counts[f] == wb.size and np.array_equal(bases[f, :min(LINES, wb.size)], wb[:LINES])
                    lines.append(wb[:LINES])
                if n == 3 and h * w > 100:
                    assert counts[1] == 0 and counts[0] > 0 and counts[2] > LINES
                for min_length, max_gap in sr.parameter_sets(h, w):
                    for exclusive in (0, 1):
                        what = f"{shape} n={n} rho={rho} theta={theta:.4f} [{lo:.2f},{hi:.2f}] {min_length}/{max_gap}/{exclusive}"
                        want = [sr.segments(masks[f], lines[f], numrho, *tabs, min_length, max_gap, exclusive)
                                for f in range(n)]
                        caps = [max(len(x) for x in want) + 2]
                        if (min_length, max_gap) == (0, 0):
                            caps.append(2)  # smaller than the total: true counts, later slots untouched
                        for cap in caps:
                            d_seg, d_cnt = dev.filled(n * cap * 6), dev.filled(n)
                            ctx.dev_hough_segments_bits(d_bits, n, h, w, rho, theta, lo, hi, d_bases, d_counts, LINES,
                                                        min_length, max_gap, exclusive, d_seg, cap, d_cnt)
                            got = dev.get(d_seg, n * cap * 6, what).reshape(n, cap, 6)
                            cnt = dev.get(d_cnt, n, what).view(np.int32)
                            _check_frames(got, cnt, want, cap, what)
                            for f in range(n):  # device and host agree byte for byte
                                hs, hc = hip.hough_segments_from_bits(bits[f], h, w, lines[f], rho, theta, lo, hi, min_length,
                                                                      max_gap, exclusive, segments_max=cap)
                                assert hc == cnt[f] and np.array_equal(hs, got[f, :len(hs)].view(np.int32)), what
            back = np.empty_like(bits)
            ctx.d2h(back, d_bits)
            assert np.array_equal(back, bits), "the caller's bit maps were written"
        dev.free()


def _plain_hough(ctx, dev, d_img, n, h, w, thr, lines_max, max_val=150):
    """A plain dev_canny_hough call: (edges, lines, votes, bases, counts) as raw arrays."""
    d_edges = dev.upload(np.full((n, h, w), 0x5A5A, np.int16))
    sizes = dict(lines=2 * n * lines_max, votes=n * lines_max, bases=n * lines_max, counts=n)
    d = {k: dev.filled(v) for k, v in sizes.items()}
    ctx.dev_canny_hough(d_img, 1.4, 50, max_val, h, w, n, 1.0, PI / 180, thr, lines_max, 0.0, PI, d["lines"], d["votes"],
                        d["bases"], d["counts"], d_edges=d_edges)
    edges = np.empty((n, h, w), np.int16)
    ctx.d2h(edges, d_edges)
    return edges, {k: dev.get(d[k], sizes[k], k) for k in sizes}


@pytest.mark.parametrize("tail", [0, 1])
def test_whole_pipeline_segments_equal_the_rule_on_dev_cannys_map(hip, tail):
    n, h, w, lm, cap = 16, 480, 640, 7, 64
    frames = synth_batch(n, h, w)
    numangle, numrho = hip.hough_geometry(h, w, 1.0, PI / 180)
    tabs = hip.hough_tables(1.0, PI / 180, 0.0, numangle)
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", tail)
        dev = _Dev(ctx)
        d_img = dev.upload(frames)
        thr = 60
        edges, plain = _plain_hough(ctx, dev, d_img, n, h, w, thr, lm)
        counts = plain["counts"].view(np.int32)
        assert np.count_nonzero(edges) > 0 and counts.max() > 0
        bases = plain["bases"].reshape(n, lm)
        for exclusive in (0, 1):
            want = [sr.segments(edges[f] != 0, bases[f, :min(lm, counts[f])], numrho, *tabs, 10, 2, exclusive)
                    for f in range(n)]
            assert sum(len(x) for x in want) > 0
            # every output given: the map and the lines are those of the plain call
            d_edges = dev.upload(np.full((n, h, w), 0x5A5A, np.int16))
            d = {k: dev.filled(v) for k, v in dict(lines=2 * n * lm, votes=n * lm, bases=n * lm, counts=n).items()}
            d_seg, d_cnt = dev.filled(n * cap * 6), dev.filled(n)
            ctx.dev_canny_hough_segments(d_img, 1.4, 50, 150, h, w, n, 1.0, PI / 180, thr, lm, 0.0, PI, 10, 2, exclusive,
                                         d_seg, cap, d_cnt, d_lines=d["lines"], d_votes=d["votes"], d_bases=d["bases"],
                                         d_line_counts=d["counts"], d_edges=d_edges)
            got_edges = np.empty((n, h, w), np.int16)
            ctx.d2h(got_edges, d_edges)
            assert np.array_equal(got_edges, edges), "d_edges differs from the plain call's map"
            for k, words in dict(lines=2 * n * lm, votes=n * lm, bases=n * lm, counts=n).items():
                assert np.array_equal(dev.get(d[k], words, k), plain[k]), f"{k} differ from the plain call's"
            _check_frames(dev.get(d_seg, n * cap * 6, "segments").reshape(n, cap, 6), dev.get(d_cnt, n, "counts"), want,
                          cap, f"all outputs, exclusive={exclusive}")
            # every optional pointer NULL
            dev.fill(d_seg, n * cap * 6)
            dev.fill(d_cnt, n)
            ctx.dev_canny_hough_segments(d_img, 1.4, 50, 150, h, w, n, 1.0, PI / 180, thr, lm, 0.0, PI, 10, 2, exclusive,
                                         d_seg, cap, d_cnt)
            got = dev.get(d_seg, n * cap * 6, "segments").reshape(n, cap, 6)
            cnt = dev.get(d_cnt, n, "counts")
            _check_frames(got, cnt, want, cap, f"optional pointers NULL, exclusive={exclusive}")
            # the host flavour equals the device flavour
            res_l, lc, res_s, sc = ctx.canny_hough_segments(frames, 1.4, 50, 150, threshold=thr, lines_max=lm, min_length=10,
                                                            max_gap=2, exclusive=exclusive, segments_max=cap)
            assert np.array_equal(lc, counts) and np.array_equal(sc, cnt.view(np.int32))
            for f in range(n):
                k = min(lm, counts[f])
                assert np.array_equal(res_l[f][2], bases[f, :k])
                assert res_l[f][0].tobytes() == plain["lines"].reshape(n, lm, 2)[f, :k].tobytes()
                assert np.array_equal(res_s[f], got[f, :len(res_s[f])].view(np.int32)) and len(res_s[f]) == min(cap, sc[f])
            # max_val > 255: the map is empty by rule, all counts 0, no record written
            dev.fill(d_seg, n * cap * 6)
            dev.fill(d_cnt, n)
            ctx.dev_canny_hough_segments(d_img, 1.4, 50, 300, h, w, n, 1.0, PI / 180, 0, lm, 0.0, PI, 0, 0, exclusive,
                                         d_seg, cap, d_cnt)
            assert (dev.get(d_cnt, n, "counts") == 0).all() and (dev.get(d_seg, n * cap * 6, "segments") == SENT).all()
        dev.free()


def _points(ctx, dev, d_img, n, h, w):
    cap = n * h * w
    d_pts, d_off = dev.filled(cap), dev.filled(2 * (n + 1))
    ctx.dev_canny_points(d_img, 1.4, 50, 150, h, w, n, d_pts, cap, d_off)
    return dev.get(d_pts, cap, "points").tobytes(), dev.get(d_off, 2 * (n + 1), "offsets").tobytes()


def test_exclusive_mode_with_frames_that_do_not_end_on_a_word(hip):
    """Exclusive mode clears bits in 32-bit words of a private copy, one workgroup per frame.  97 x 161 frames are 2037
    packed bytes each, so in the caller's layout every frame boundary falls inside a 32-bit word (at three different
    byte offsets over four frames); the copy must give each frame words of its own.  The maps are all set around the
    boundaries: the last rows of one frame and the first rows of the next hold set pixels that lines claim."""
    n, h, w, lm = 4, 97, 161, 64
    assert (h * ((w + 7) // 8)) % 4 == 1
    rng = np.random.default_rng(21)
    masks = np.stack([np.ones((h, w), bool), sr.drawn(h, w) | (rng.random((h, w)) < 0.05), np.ones((h, w), bool),
                      rng.random((h, w)) < 0.3])
    masks[:, :3, :] = True   # the bytes on both sides of every boundary are full
    masks[:, -3:, :] = True
    bits = np.packbits(masks, axis=-1)
    numangle, numrho = hip.hough_geometry(h, w, 1.0, PI / 180)
    tabs = hip.hough_tables(1.0, PI / 180, 0.0, numangle)
    with hip.Context(0) as ctx:
        dev = _Dev(ctx)
        d_bits = dev.upload(bits)
        d_bases, d_counts = dev.filled(n * lm), dev.filled(n)
        ctx.dev_hough_bits(d_bits, n, h, w, 1.0, PI / 180, 0, lm, 0.0, PI, 0, 0, d_bases, d_counts)
        bases = dev.get(d_bases, n * lm, "bases").reshape(n, lm)
        counts = dev.get(d_counts, n, "line counts").view(np.int32)
        assert (counts >= lm).all()
        for min_length, max_gap in ((0, 0), (5, 3)):
            want = [sr.segments(masks[f], bases[f], numrho, *tabs, min_length, max_gap, 1) for f in range(n)]
            plain = [sr.segments(masks[f], bases[f], numrho, *tabs, min_length, max_gap, 0) for f in range(n)]
            assert all(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(want, plain))  # pixels were claimed
            for f in range(n):  # ... in the first and in the last rows of every frame, beside the boundaries
                claimed_rows = {int(r[1]) for r in want[f]} | {int(r[3]) for r in want[f]}
                assert min(claimed_rows) <= 2 and max(claimed_rows) >= h - 3
            cap = max(len(x) for x in want) + 2
            d_seg, d_cnt = dev.filled(n * cap * 6), dev.filled(n)
            for _ in range(2):
                dev.fill(d_seg, n * cap * 6)
                ctx.dev_hough_segments_bits(d_bits, n, h, w, 1.0, PI / 180, 0.0, PI, d_bases, d_counts, lm, min_length,
                                            max_gap, 1, d_seg, cap, d_cnt)
                _check_frames(dev.get(d_seg, n * cap * 6, "segments").reshape(n, cap, 6), dev.get(d_cnt, n, "counts"),
                              want, cap, f"4 x 97x161 exclusive {min_length}/{max_gap}")
        back = np.empty_like(bits)
        ctx.d2h(back, d_bits)
        assert np.array_equal(back, bits), "the caller's bit maps were written"
        dev.free()


def test_exclusive_mode_leaves_the_plane_alone_and_runs_repeat(hip):
    """Repeatability of both modes on one context, in any order, and d_bits untouched by exclusive calls.
    What this test can NOT show is that the context's strong plane stays unwritten: every dev_canny_hough_segments and
    every dev_canny_points call runs dev_canny first, which rebuilds the plane before it is read.  That guarantee rests on
    the code: the exclusive kernel is handed the private copy alone (the source pointers of its SegSrc are null, and they
    are pointers to const), and the copy is made by a device-to-device copy whose source is const."""
    n, h, w, lm, cap = 3, 130, 333, 40, 512
    frames = synth_batch(n, h, w)
    with hip.Context(0) as ctx:
        dev = _Dev(ctx)
        d_img = dev.upload(frames)
        d_seg, d_cnt = dev.filled(n * cap * 6), dev.filled(n)

        def run(exclusive):
            dev.fill(d_seg, n * cap * 6)
            dev.fill(d_cnt, n)
            ctx.dev_canny_hough_segments(d_img, 1.4, 50, 150, h, w, n, 1.0, PI / 180, 20, lm, 0.0, PI, 3, 1, exclusive,
                                         d_seg, cap, d_cnt)
            return dev.get(d_seg, n * cap * 6, "segments").tobytes(), dev.get(d_cnt, n, "counts").tobytes()

        plain = run(0)
        points = _points(ctx, dev, d_img, n, h, w)
        excl = run(1)
        assert excl != plain and np.frombuffer(excl[1], np.int32).sum() > 0
        assert run(0) == plain, "a non-exclusive call after an exclusive one differs"
        assert _points(ctx, dev, d_img, n, h, w) == points
        assert run(1) == excl and run(1) == excl and run(0) == plain, "the bytes differ between runs"
        # the same on caller bit maps
        masks = np.stack([sr.drawn(97, 161), np.random.default_rng(4).random((97, 161)) < 0.03])
        d_bits = dev.upload(np.packbits(masks, axis=-1))
        d_bases, d_counts = dev.filled(2 * lm), dev.filled(2)
        ctx.dev_hough_bits(d_bits, 2, 97, 161, 1.0, PI / 180, 0, lm, 0.0, PI, 0, 0, d_bases, d_counts)
        d_seg2, d_cnt2 = dev.filled(2 * cap * 6), dev.filled(2)
        runs = []
        for exclusive in (0, 1, 1, 0):
            dev.fill(d_seg2, 2 * cap * 6)
            ctx.dev_hough_segments_bits(d_bits, 2, 97, 161, 1.0, PI / 180, 0.0, PI, d_bases, d_counts, lm, 0, 1, exclusive,
                                        d_seg2, cap, d_cnt2)
            runs.append((dev.get(d_seg2, 2 * cap * 6, "segments").tobytes(), dev.get(d_cnt2, 2, "counts").tobytes()))
        assert runs[0] == runs[3] and runs[1] == runs[2] and runs[0] != runs[1]
        dev.free()


def test_argument_errors_write_nothing_and_leave_the_context_usable(hip):
    mask = sr.drawn(64, 96)[None]
    with hip.Context(0) as ctx:
        dev = _Dev(ctx)
        d_bits = dev.upload(np.packbits(mask, axis=-1))
        d_bases, d_counts = dev.filled(LINES), dev.filled(1)
        ctx.dev_hough_bits(d_bits, 1, 64, 96, 1.0, PI / 180, 0, LINES, 0.0, PI, 0, 0, d_bases, d_counts)
        d_seg, d_cnt = dev.filled(8 * 6), dev.filled(1)
        ok = dict(bits=d_bits, rho=1.0, theta=PI / 180, lo=0.0, hi=PI, bases=d_bases, counts=d_counts, lm=LINES, ml=0, mg=0,
                  ex=0, seg=d_seg, cap=8, cnt=d_cnt)
        bad = [dict(ml=-1), dict(mg=-1), dict(ex=2), dict(cap=0), dict(lm=0), dict(bits=0), dict(bases=0), dict(counts=0),
               dict(seg=0), dict(cnt=0), dict(rho=0.0), dict(theta=float("nan")), dict(lo=1.0, hi=1.0), dict(hi=3.2)]
        for b in bad + [dict(cap=(2 ** 31 + 5) // 6), dict(lm=hip.HOUGH_MAX_LINES + 1)]:
            a = dict(ok, **b)
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_hough_segments_bits(a["bits"], 1, 64, 96, a["rho"], a["theta"], a["lo"], a["hi"], a["bases"],
                                            a["counts"], a["lm"], a["ml"], a["mg"], a["ex"], a["seg"], a["cap"], a["cnt"])
            assert ei.value.status == (1 if b in bad else 2), b
            assert (dev.get(d_seg, 8 * 6, "segments") == SENT).all() and (dev.get(d_cnt, 1, "counts") == SENT).all(), b
        a = ok
        ctx.dev_hough_segments_bits(a["bits"], 1, 64, 96, a["rho"], a["theta"], a["lo"], a["hi"], a["bases"], a["counts"],
                                    a["lm"], a["ml"], a["mg"], a["ex"], a["seg"], a["cap"], a["cnt"])
        assert dev.get(d_cnt, 1, "counts").view(np.int32)[0] > 0
        dev.free()


def test_segment_profile_parts_are_timed(hip):
    mask = sr.drawn(128, 128)[None]
    with hip.Context(0) as ctx:
        dev = _Dev(ctx)
        d_bits = dev.upload(np.packbits(mask, axis=-1))
        d_bases, d_counts = dev.filled(LINES), dev.filled(1)
        ctx.dev_hough_bits(d_bits, 1, 128, 128, 1.0, PI / 180, 0, LINES, 0.0, PI, 0, 0, d_bases, d_counts)
        d_seg, d_cnt = dev.filled(64 * 6), dev.filled(1)
        ctx.set_option("profile_stage_mask", 0b111 << 19)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for exclusive in (0, 0, 1):
            ctx.dev_hough_segments_bits(d_bits, 1, 128, 128, 1.0, PI / 180, 0.0, PI, d_bases, d_counts, LINES, 0, 0, exclusive,
                                        d_seg, 64, d_cnt)
        ctx.dev_hough_bits(d_bits, 1, 128, 128, 1.0, PI / 180, 0, LINES, 0.0, PI, 0, 0, d_bases, d_counts)  # masked out
        for part, launches in enumerate((2, 2, 1)):
            ms, got = ctx.hough_segments_profile_get(part)
            assert got == launches and ms > 0.0, hip.SEGMENT_PARTS[part]
        assert all(ctx.hough_profile_get(p)[1] == 0 for p in range(3))
        assert all(ctx.components_profile_get(p)[1] == 0 for p in range(4))
        assert all(ctx.edt_profile_get(p)[1] == 0 for p in range(2))
        assert all(ctx.profile_get(s)[1] == 0 for s in range(10))
        with pytest.raises(hip.CannyHipError):
            ctx.hough_profile_get(3)
        with pytest.raises(hip.CannyHipError):
            ctx.hough_segments_profile_get(3)
        ctx.profile_enable(False)
        dev.free()


def test_cli_writes_the_segments_of_a_drawn_frame(hip, tmp_path):
    h, w = 240, 320
    img = np.full((h, w), 40, np.int32)
    img[60:180, 80:240] = 200  # a bright rectangle: four straight edges; a little noise, or the reference's NMS
    img = np.clip(img + np.random.default_rng(1).integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)  # drops the plateaus
    pgm = tmp_path / "in.pgm"
    pgm.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    theta = float(np.float32(1.0 * np.pi / 180.0))  # -l takes degrees
    with hip.Context(0) as ctx:
        edges = ctx.canny(img, 1.0, 50, 150)
    numangle, numrho = hip.hough_geometry(h, w, 1.0, theta)
    tabs = hip.hough_tables(1.0, theta, 0.0, numangle)
    acc = hr.accumulate(np.flatnonzero(edges), w, numrho, *tabs)
    wl, wv, wb, wc = hr.lines(acc, 30, 16, 1.0, theta)
    for g, exclusive in (("10,2", 0), ("10,2,1", 1)):
        r = subprocess.run([exe, "1.0", "50", "150", "-i", str(pgm), "-o", str(tmp_path), "-l", "1,1,30,16", "-g", g],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        rows = [[int(v) for v in l.split()] for l in (tmp_path / "canny_segments.txt").read_text().splitlines()]
        want = sr.segments(edges != 0, wb, numrho, *tabs, 10, 2, exclusive)
        assert len(want) >= 4 and rows == want.tolist()
        lines = [l.split() for l in (tmp_path / "canny_lines.txt").read_text().splitlines()]
        assert lines == [["%.9g" % l[0], "%.9g" % l[1], str(int(v))] for l, v in zip(wl, wv)]
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(pgm), "-o", str(tmp_path), "-g", "10,2"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "-g" in r.stderr
