"""Hough lines on the GPU (canny_hip_dev_hough_bits / _points / canny_hip_dev_canny_hough / canny_hip_canny_hough)
against the numpy restatement of the rule (tests/hough_rule.py), fed with the LIBRARY's own vote tables so that no libm
difference can enter: every comparison is exact equality on whole arrays -- the accumulators cell for cell with their
border, bases, votes, counts, and the (rho, theta) pairs as raw 32-bit patterns.  Every output buffer is pre-filled with
a sentinel and followed by a guard region; slots past min(lines_max, counts[f]) must keep the sentinel."""
import os
import subprocess

import numpy as np
import pytest

import hough_rule as hr
from canny_edge_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = float(np.pi)
SENT = 0xA5A5A5A5
N_GUARD = 64
PATHS = (1, 2)  # "hough_path": 1 global atomics, 2 LDS rows


def _csr(masks):
    lists = [np.flatnonzero(m).astype(np.uint32) for m in masks]
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([l.size for l in lists], dtype=np.uint64)
    return np.concatenate(lists + [np.empty(0, np.uint32)]), off


class _Call:
    """Guarded device outputs of one Hough call on n frames of h x w."""

    def __init__(self, hip, ctx, n, h, w, rho, theta, lines_max, lo=0.0, hi=PI, with_accum=True):
        self.hip, self.ctx, self.n, self.h, self.w = hip, ctx, n, h, w
        self.rho, self.theta, self.lm, self.lo, self.hi = rho, theta, lines_max, lo, hi
        self.numangle, self.numrho = hip.hough_geometry(h, w, rho, theta, lo, hi)
        self.tabs = hip.hough_tables(rho, theta, lo, self.numangle)
        self.cells = (self.numangle + 2) * (self.numrho + 2)
        self.slots = n * lines_max
        self.ptrs = []
        self.sizes = dict(lines=2 * self.slots, votes=self.slots, bases=self.slots, counts=n,
                          accum=n * self.cells if with_accum else 0)
        self.d = {k: (self._filled(v) if v else 0) for k, v in self.sizes.items()}

    def _malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def _filled(self, words):
        p = self._malloc(4 * (words + N_GUARD))
        self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self._malloc(a.nbytes)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def refill(self):
        for k, v in self.sizes.items():
            if v:
                self.ctx.h2d(self.d[k], np.full(v + N_GUARD, SENT, np.uint32))

    def _tail(self, threshold):
        d = self.d
        return (self.rho, self.theta, threshold, self.lm, self.lo, self.hi, d["lines"], d["votes"], d["bases"],
                d["counts"], d["accum"])

    def bits(self, d_bits, threshold):
        self.ctx.dev_hough_bits(d_bits, self.n, self.h, self.w, *self._tail(threshold))

    def points(self, d_pts, d_off, threshold):
        self.ctx.dev_hough_points(d_pts, d_off, self.n, self.h, self.w, *self._tail(threshold))

    def canny(self, d_img, sigma, lo, hi, threshold, d_edges=0):
        self.ctx.dev_canny_hough(d_img, sigma, lo, hi, self.h, self.w, self.n, *self._tail(threshold), d_edges=d_edges)

    def get(self, key):
        """(payload, guard intact) of an output array as uint32 words."""
        words = self.sizes[key]
        out = np.empty(words + N_GUARD, np.uint32)
        self.ctx.d2h(out, self.d[key])
        return out[:words], bool((out[words:] == SENT).all())

    def outputs(self):
        return {k: self.get(k) for k, v in self.sizes.items() if v}

    def want_accum(self, masks):
        return np.stack([hr.accumulate(np.flatnonzero(m), self.w, self.numrho, *self.tabs) for m in masks])

    def check_accum(self, want, what):
        got, guard = self.get("accum")
        assert guard, f"{what}: guard behind the accumulators overwritten"
        got = got.view(np.int32).reshape(want.shape)
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} accumulator cells differ"

    def check_lines(self, want_acc, threshold, what):
        out = self.outputs()
        for k, (_, guard) in out.items():
            assert guard, f"{what}: guard behind {k} overwritten"
        counts = out["counts"][0].view(np.int32)
        lines = out["lines"][0].reshape(self.n, self.lm, 2)
        votes, bases = out["votes"][0].reshape(self.n, self.lm), out["bases"][0].reshape(self.n, self.lm)
        for f in range(self.n):
            wl, wv, wb, wc = hr.lines(want_acc[f], threshold, self.lm, self.rho, self.theta, self.lo)
            k = min(self.lm, wc)
            assert counts[f] == wc, f"{what} frame {f}: count {counts[f]} != {wc}"
            assert np.array_equal(bases[f, :k], wb), f"{what} frame {f}: bases"
            assert np.array_equal(votes[f, :k].view(np.int32), wv), f"{what} frame {f}: votes"
            assert np.array_equal(lines[f, :k], wl.view(np.uint32)), f"{what} frame {f}: (rho, theta) bit patterns"
            assert (bases[f, k:] == SENT).all() and (votes[f, k:] == SENT).all() and (lines[f, k:] == SENT).all(), \
                f"{what} frame {f}: slots past the count were written"

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def _both_kinds_and_paths(hip, masks, rho, theta, what, lo=0.0, hi=PI, thresholds=(), lines_max=7):
    """Accumulators (and, for the given thresholds, lines) of a stack of masks through bits and points, paths 1 and 2."""
    masks = np.asarray(masks, bool)
    n, h, w = masks.shape
    with hip.Context(0) as ctx:
        c = _Call(hip, ctx, n, h, w, rho, theta, lines_max, lo, hi)
        want = c.want_accum(masks)
        d_bits = c.upload(np.packbits(masks, axis=-1))
        pts, off = _csr(masks)
        d_pts, d_off = c.upload(pts), c.upload(off)
        seen = []
        for path in PATHS:
            ctx.set_option("hough_path", path)
            for kind in ("bits", "points"):
                for thr in (thresholds or (0,)):
                    c.refill()
                    c.bits(d_bits, thr) if kind == "bits" else c.points(d_pts, d_off, thr)
                    tag = f"{what} rho={rho} theta=pi/{PI / theta:.0f} path={path} {kind} thr={thr}"
                    c.check_accum(want, tag)
                    if thresholds:
                        c.check_lines(want, thr, tag)
                seen.append(c.get("accum")[0].copy())
        assert all(np.array_equal(seen[0], s) for s in seen[1:]), f"{what}: the paths / sources differ from each other"
        c.free()
    return want


def _drawn(h, w):
    m = np.zeros((h, w), bool)
    d = min(h, w)
    m[h // 3, :] = True                                   # horizontal
    m[:, w // 4] = True                                   # vertical
    m[np.arange(d), np.arange(d)] = True                  # diagonal through the corner pixel (0, 0)
    m[h - 1 - np.arange(d), w - d + np.arange(d)] = True  # anti-diagonal ending in column w - 1
    m[h - 1 - np.arange(d // 2), w - 1 - np.arange(d // 2)] = True  # through (H - 1, W - 1)
    return m


def _bernoulli_batch(h, w, seed):
    """Five frames: densities 0.1 %, 1 %, an EMPTY third frame, 20 %, all set."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random((h, w)) < 0.001, rng.random((h, w)) < 0.01, np.zeros((h, w), bool),
                     rng.random((h, w)) < 0.2, np.ones((h, w), bool)])


@pytest.mark.parametrize("theta", [PI / 90, PI / 180, PI / 360], ids=["pi/90", "pi/180", "pi/360"])
@pytest.mark.parametrize("rho", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (77, 77), (256, 256), (480, 640)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulators_of_random_masks_cell_for_cell(hip, shape, rho, theta):
    _both_kinds_and_paths(hip, _bernoulli_batch(*shape, seed=shape[0] * 7 + shape[1]), rho, theta, f"bernoulli {shape}")


@pytest.mark.parametrize("shape", [(77, 77), (256, 256), (480, 640)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulators_of_drawn_lines(hip, shape):
    for rho, theta in [(1.0, PI / 180), (0.5, PI / 360), (2.0, PI / 90)]:
        _both_kinds_and_paths(hip, _drawn(*shape)[None], rho, theta, f"drawn lines {shape}")


def test_accumulators_theta_sub_range(hip):
    masks = np.stack([_drawn(256, 256), np.random.default_rng(5).random((256, 256)) < 0.01])
    want = _both_kinds_and_paths(hip, masks, 1.0, PI / 180, "theta in [pi/4, 3pi/4]", lo=PI / 4, hi=3 * PI / 4,
                                 thresholds=(0, 60), lines_max=7)
    assert want.shape[1] == hip.hough_geometry(256, 256, 1.0, PI / 180, PI / 4, 3 * PI / 4)[0] + 2 < 100


def test_accumulators_of_the_canny_map_of_the_fixture(hip, fixture_image):
    with hip.Context(0) as ctx:
        edges = ctx.canny(fixture_image, 1.0, 50, 150)
    assert np.count_nonzero(edges) > 500
    _both_kinds_and_paths(hip, (edges != 0)[None], 1.0, PI / 180, "canny map of the fixture", thresholds=(0, 40))


@pytest.mark.parametrize("shape,rho,theta", [((1080, 1920), 1.0, PI / 180), ((2160, 3840), 1.0, PI / 180),
                                             ((2160, 3840), 0.5, PI / 360)],
                         ids=["1080p", "4k", "4k_rho0.5_pi/360"])
def test_accumulators_and_lines_of_large_frames(hip, shape, rho, theta):
    """One frame; the 4K frame at rho 0.5 has rows of 24001 ints, more than the 64 KiB a kernel gets without asking."""
    mask = np.random.default_rng(shape[0]).random(shape) < 0.012
    mask |= _drawn(*shape)
    _both_kinds_and_paths(hip, mask[None], rho, theta, f"{shape}", thresholds=(0,), lines_max=4096)


@pytest.mark.parametrize("lines_max", [1, 7, 4096])
def test_lines_thresholds_ties_and_truncation(hip, lines_max):
    """threshold 0 gives thousands of tied peaks (ties decide the order and the truncation falls inside a run of ties);
    threshold max(accum) gives no peak at all and must leave every slot untouched."""
    masks = np.stack([_drawn(256, 256), np.random.default_rng(11).random((256, 256)) < 0.01, np.zeros((256, 256), bool),
                      np.random.default_rng(14).random((256, 256)) < 0.001])
    numangle, numrho = hr.geometry(256, 256, 1.0, PI / 180)
    acc = np.stack([hr.accumulate(np.flatnonzero(m), 256, numrho, *hip.hough_tables(1.0, PI / 180, 0.0, numangle))
                    for m in masks])
    top = int(acc.max())
    base, votes = hr.peaks(acc[3], 0)  # the sparse frame: thousands of tied peaks, the cut falls inside a run of ties
    assert base.size > lines_max and votes[lines_max - 1] == votes[lines_max]
    assert np.count_nonzero(votes == votes[-1]) > 3000
    _both_kinds_and_paths(hip, masks, 1.0, PI / 180, f"lines_max={lines_max}", thresholds=(0, top // 2, top - 1, top),
                          lines_max=lines_max)


def test_lines_of_a_4k_frame_at_threshold_0(hip):
    """~90 000 tied peaks on one 4K frame: the cut-off falls deep inside a run of ties."""
    shape = (2160, 3840)
    mask = np.random.default_rng(3).random(shape) < 0.012
    with hip.Context(0) as ctx:
        for lines_max in (7, 4096):
            c = _Call(hip, ctx, 1, *shape, 1.0, PI / 180, lines_max)
            want = c.want_accum(mask[None])
            c.bits(c.upload(np.packbits(mask[None], axis=-1)), 0)
            c.check_accum(want, "4K")
            c.check_lines(want, 0, f"4K threshold 0 lines_max={lines_max}")
            assert hr.peaks(want[0], 0)[0].size > 20000
            c.free()


def _dev_canny_map(ctx, frames, sigma, lo, hi):
    d_in, d_out = ctx.malloc(frames.nbytes), ctx.malloc(frames.nbytes * 2)
    ctx.h2d(d_in, frames)
    ctx.dev_canny(d_in, sigma, lo, hi, frames.shape[1], frames.shape[2], frames.shape[0], d_out)
    out = np.empty(frames.shape, np.int16)
    ctx.d2h(out, d_out)
    ctx.free(d_in)
    ctx.free(d_out)
    return out


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("n,h,w", [(16, 480, 640), (3, 130, 77), (2, 130, 4096)], ids=["16x480x640", "w77", "w4096"])
def test_whole_pipeline_equals_the_rule_on_dev_cannys_map(hip, n, h, w, tail):
    frames = synth_batch(n, h, w)
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", tail)
        edges = _dev_canny_map(ctx, frames, 1.4, 50, 150)
        assert np.count_nonzero(edges) > 0
        c = _Call(hip, ctx, n, h, w, 1.0, PI / 180, 7)
        want = c.want_accum(edges != 0)
        thr = int(want.max()) // 2
        d_img = c.upload(frames)
        d_edges = c.upload(np.full(frames.shape, 0x5A5A, np.int16))
        c.canny(d_img, 1.4, 50, 150, thr, d_edges=d_edges)
        got_edges = np.empty(frames.shape, np.int16)
        ctx.d2h(got_edges, d_edges)
        assert np.array_equal(got_edges, edges), "d_edges differs from dev_canny's map"
        c.check_accum(want, "dev_canny_hough")
        c.check_lines(want, thr, "dev_canny_hough")
        c.refill()
        c.canny(d_img, 1.4, 50, 150, thr)  # d_edges = NULL
        c.check_accum(want, "dev_canny_hough without d_edges")
        c.check_lines(want, thr, "dev_canny_hough without d_edges")
        # host path
        res, counts = ctx.canny_hough(frames, 1.4, 50, 150, threshold=thr, lines_max=7)
        for f in range(n):
            wl, wv, wb, wc = hr.lines(want[f], thr, 7, 1.0, PI / 180)
            assert counts[f] == wc and np.array_equal(res[f][2], wb) and np.array_equal(res[f][1], wv)
            assert res[f][0].tobytes() == wl.tobytes()
        c.free()


def test_whole_pipeline_follows_the_map_and_dev_cannys_statuses(hip):
    frames = synth_batch(3, 120, 200)
    with hip.Context(0) as ctx:
        c = _Call(hip, ctx, 3, 120, 200, 1.0, PI / 180, 7)
        d_img = c.upload(frames)
        c.canny(d_img, 1.0, 50, 300, 0)  # max_val > 255: the map is empty by rule
        out = c.outputs()
        assert (out["counts"][0] == 0).all() and (out["accum"][0] == 0).all()
        assert all((out[k][0] == SENT).all() for k in ("lines", "votes", "bases")) and all(g for _, g in out.values())
        for lo, hi in [(0, 100), (-5, 100), (300, 100)]:  # dev_canny's own status; on any but OK nothing is written
            c.refill()
            plain, edges = 0, None
            try:
                edges = _dev_canny_map(ctx, frames, 1.0, lo, hi)
            except hip.CannyHipError as e:
                plain = e.status
            if (lo, hi) == (300, 100):
                assert plain == 5  # CANNY_HIP_ERR_DOMAIN
            if plain == 0:  # min_val <= 0 is accepted on a whole pipeline (every pixel connectable): the rule on its map
                c.canny(d_img, 1.0, lo, hi, 20)
                want = c.want_accum(edges != 0)
                c.check_accum(want, f"thresholds {lo}/{hi}")
                c.check_lines(want, 20, f"thresholds {lo}/{hi}")
            else:
                with pytest.raises(hip.CannyHipError) as ei:
                    c.canny(d_img, 1.0, lo, hi, 0)
                assert ei.value.status == plain
                assert all((a == SENT).all() and g for a, g in c.outputs().values())
        c.free()


def test_same_bytes_on_every_run(hip):
    masks = np.stack([_drawn(256, 320), np.random.default_rng(2).random((256, 320)) < 0.02])
    other = synth_batch(2, 100, 333)
    with hip.Context(0) as ctx:
        c = _Call(hip, ctx, 2, 256, 320, 1.0, PI / 180, 300)
        d_bits = c.upload(np.packbits(masks, axis=-1))
        runs = []
        for i in range(3):
            if i == 2:
                _dev_canny_map(ctx, other, 1.0, 40, 120)  # an unrelated call on another shape in between
            c.refill()
            c.bits(d_bits, 0)
            runs.append({k: v[0].tobytes() for k, v in c.outputs().items()})
        assert len(runs[0]) == 5 and runs[0] == runs[1] == runs[2]
        c.free()


def test_argument_errors_write_nothing_and_leave_the_context_usable(hip):
    mask = _drawn(64, 96)[None]
    with hip.Context(0) as ctx:
        c = _Call(hip, ctx, 1, 64, 96, 1.0, PI / 180, 7)
        d_bits = c.upload(np.packbits(mask, axis=-1))
        bad = [dict(rho=0.0), dict(rho=-1.0), dict(rho=float("nan")), dict(rho=float("inf")), dict(theta=0.0),
               dict(theta=float("nan")), dict(theta=float("inf")), dict(lo=-0.1), dict(lo=1.0, hi=1.0), dict(hi=3.2),
               dict(lm=0), dict(lm=-3), dict(counts=0)]
        for b in bad + [dict(lm=hip.HOUGH_MAX_LINES + 1)]:
            a = dict(rho=1.0, theta=PI / 180, lo=0.0, hi=PI, lm=7, counts=c.d["counts"])
            a.update(b)
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_hough_bits(d_bits, 1, 64, 96, a["rho"], a["theta"], 0, a["lm"], a["lo"], a["hi"], c.d["lines"],
                                   c.d["votes"], c.d["bases"], a["counts"], c.d["accum"])
            assert ei.value.status == (2 if a["lm"] > hip.HOUGH_MAX_LINES else 1), b
            assert all((v == SENT).all() and g for v, g in c.outputs().values()), b
        want = c.want_accum(mask)
        c.bits(d_bits, 10)
        c.check_accum(want, "after the errors")
        c.check_lines(want, 10, "after the errors")
        c.free()


def test_hough_profile_parts_are_timed(hip):
    mask = _drawn(128, 128)[None]
    with hip.Context(0) as ctx:
        c = _Call(hip, ctx, 1, 128, 128, 1.0, PI / 180, 7)
        d_bits = c.upload(np.packbits(mask, axis=-1))
        ctx.profile_enable(True)
        ctx.profile_reset()
        c.bits(d_bits, 10)
        c.bits(d_bits, 10)
        for part in range(3):
            ms, launches = ctx.hough_profile_get(part)
            assert launches == 2 and ms > 0.0
        assert ctx.profile_get(9)[1] == 0  # the map's stages are untouched
        ctx.profile_enable(False)
        with pytest.raises(hip.CannyHipError):
            ctx.hough_profile_get(3)
        c.free()


def test_cli_writes_the_lines_of_a_drawn_frame(hip, tmp_path):
    h, w = 240, 320
    img = np.full((h, w), 40, np.int32)
    img[60:180, 80:240] = 200  # a bright rectangle: four straight edges; a little noise, or the reference's NMS
    img = np.clip(img + np.random.default_rng(1).integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)  # drops the plateaus
    pgm = tmp_path / "in.pgm"
    pgm.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(pgm), "-o", str(tmp_path), "-l", "1,1,30,16"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in (tmp_path / "canny_lines.txt").read_text().splitlines()]
    theta = float(np.float32(1.0 * np.pi / 180.0))  # -l takes degrees
    with hip.Context(0) as ctx:
        edges = ctx.canny(img, 1.0, 50, 150)
    numangle, numrho = hip.hough_geometry(h, w, 1.0, theta)
    acc = hr.accumulate(np.flatnonzero(edges), w, numrho, *hip.hough_tables(1.0, theta, 0.0, numangle))
    wl, wv, _, wc = hr.lines(acc, 30, 16, 1.0, theta)
    assert wc >= 4 and len(rows) == min(wc, 16)
    want = [["%.9g" % l[0], "%.9g" % l[1], str(int(v))] for l, v in zip(wl, wv)]
    assert rows == want
