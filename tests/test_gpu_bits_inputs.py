"""The promise of include/canny_hip.h for a caller's packed bit maps -- any byte address, the padding bits of a row ignored
whatever they hold -- for the entry points whose own tests only ever hand over np.packbits(...) at the address the allocator
returned: dev_hough_bits (every hough_path), dev_hough_segments_bits (exclusive 0 and 1), dev_line_fits_bits and
dev_circle_fits_bits (u8 and s16 planes), dev_hough_circles_bits, dev_polygons_bits, dev_shapes_bits and dev_chamfer_bits
(d_dist2 given and NULL).

Per (stage, shape), see tests/bits_inputs.py for the shapes, masks and placements:

  * the expected value is the stage's numpy rule on the masks, computed once;
  * the CPU control, before any GPU call: the same rule on the same data with the pad columns counted as pixels (the mask
    widened to 8 * row_bytes columns, planes widened by edge replication) differs from the expected value, so that a reader
    that trusts a pad bit cannot pass.  Results at two widths are compared in a form that does not depend on the width (pixel
    indices as (row, column), no accumulator cells).  The shape without pad bits has nothing to widen and no control;
  * every placement (shift 0, 1, 3, 7; filler 0xFF and once 0x00; pad bits clean, all set, random) runs on ONE context,
    the aligned clean one first, so that the later calls reuse the workspaces it sized;
  * every output the call writes is compared byte for byte with the rule's, unused slots and guard words included, so the
    bytes are the same under every placement; after each call the map and both filler regions hold what was uploaded.

The global-vote fallback of hough_path 0 needs an accumulator row that does not fit in LDS (a frame of several thousand
columns) and is not reached at these shapes; paths 0, 1 and 2 are."""
import numpy as np
import pytest

import bits_inputs as bi
import chamfer_rule
import circle_fits_rule
import contours_rule
import hough_circles_rule
import hough_rule
import hough_segments_rule
import line_fits_rule
import polygons_rule
import shapes_rule
from components_rule import FIRST

pytestmark = pytest.mark.gpu

PI = float(np.pi)
RHO, THETA, LINES_MAX = 1.0, PI / 180, 16
MIN_LENGTH, MAX_GAP = 3, 1
MIN_AREA, TOLERANCE = 2, (384, 655)
U32, I32, I64, U64 = np.uint32, np.int32, np.int64, np.uint64


def _concat(arrays, width):
    arrays = [np.asarray(a).reshape(-1, width) for a in arrays]
    return np.concatenate(arrays) if arrays else np.zeros((0, width), I64)


class Stage:
    """One entry point at one shape: the masks, the rule's value for each variant of the call, its width-free form for the
    control, the expected bytes of every output and the launch."""
    variants = ("only",)

    def __init__(self, hip, shape):
        self.hip, self.shape = hip, shape
        self.n, self.h, self.w = shape
        self.masks = self.make_masks()
        self.masks.setflags(write=False)
        self.prepare()
        self.value = {v: self.rule(v, self.masks, self.w) for v in self.variants}

    def prepare(self):
        pass

    def setup(self, ctx, variant):
        pass

    def control(self):
        """The widened rule differs from the expected value under both dirty pad settings, for every variant."""
        if not bi.pad_bits(self.w):
            return 0
        done = 0
        for pad in bi.PADS[1:]:
            wide = bi.widened(bi.packed(self.masks, pad, seed=self.h))
            assert wide.shape[-1] == 8 * bi.row_bytes(self.w) and np.array_equal(wide[..., :self.w], self.masks)
            assert all(wide[f, :, self.w:].any() for f in range(self.n)), "a frame without a set pad bit"
            for v in self.variants:
                got = self.portable(self.rule(v, wide, wide.shape[-1]), wide.shape[-1])
                want = self.portable(self.value[v], self.w)
                assert bi.differ(got, want), (f"{type(self).__name__} {self.shape} {v}, pad bits {pad}: counting the pad "
                                              f"columns as pixels changes nothing, the case cannot see a slip")
                done += 1
        return done

    def host_forms(self):
        pass

    def tables(self, width):
        """(numrho, tab_cos, tab_sin) of the library for a frame of this height and `width`."""
        na, nr = self.hip.hough_geometry(self.h, width, RHO, THETA)
        return (nr, *self.hip.hough_tables(RHO, THETA, 0.0, na))

    def line_threshold(self):
        """At most the pad bits of a frame (h per pad column), so that a phantom column is a detected line; a frame of two
        columns has no long lines and takes every cell with two votes."""
        return 2 * self.h // 3 if self.w >= 9 else 1

    def line_lists(self):
        """Per frame the rule's lines of the real masks (bases uint32, stored count), as a Hough call would leave them."""
        nr, tc, ts = self.tables(self.w)
        out = []
        for m in self.masks:
            acc = hough_rule.accumulate(np.flatnonzero(m), self.w, nr, tc, ts)
            out.append(hough_rule.lines(acc, self.line_threshold(), LINES_MAX, RHO, THETA)[2])
        assert all(len(b) >= 1 for b in out)
        return out

    def upload_lines(self, outs):
        bases = np.zeros((self.n, LINES_MAX), U32)
        counts = np.zeros(self.n, I32)
        for f, b in enumerate(self.lines):
            bases[f, :len(b)], counts[f] = b, len(b)
        return outs.up("bases", bases), outs.up("line_counts", counts)


# ---- dev_hough_bits ------------------------------------------------------------------------------------------------------
class Hough(Stage):
    variants = ("path0", "path1", "path2")

    def make_masks(self):
        return bi.line_masks(*self.shape)

    def setup(self, ctx, variant):
        ctx.set_option("hough_path", int(variant[-1]))

    def rule(self, variant, masks, width):
        key = ("rule", width, masks.tobytes())
        if getattr(self, "_memo", (None,))[0] != key:   # the three paths have one value
            nr, tc, ts = self.tables(width)
            acc = np.stack([hough_rule.accumulate(np.flatnonzero(m), width, nr, tc, ts) for m in masks])
            self._memo = (key, (acc, [hough_rule.lines(a, self.line_threshold(), LINES_MAX, RHO, THETA) for a in acc]))
        return self._memo[1]

    def portable(self, value, width):
        _, lines = value
        return (np.array([l[3] for l in lines]), _concat([l[1] for l in lines], 1),
                _concat([l[0].view(U32) for l in lines], 2))

    def alloc(self, ctx, variant):
        acc, lines = self.value[variant]
        slots = self.n * LINES_MAX
        outs = bi.Outputs(ctx)
        d = [outs.add("lines", 2 * slots, U32), outs.add("votes", slots, I32), outs.add("bases", slots, U32),
             outs.add("counts", self.n, I32), outs.add("accum", acc.size, I32)]
        want = dict(lines=bi.expected_bytes(2 * slots, U32, []), votes=bi.expected_bytes(slots, I32, []),
                    bases=bi.expected_bytes(slots, U32, []), counts=bi.expected_bytes(self.n, I32, [l[3] for l in lines]),
                    accum=bi.expected_bytes(acc.size, I32, acc))
        for f, (wl, wv, wb, _) in enumerate(lines):
            bi.put(want["lines"], U32, 2 * f * LINES_MAX, wl.view(U32))
            bi.put(want["votes"], I32, f * LINES_MAX, wv)
            bi.put(want["bases"], U32, f * LINES_MAX, wb)
        self.d = d
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_hough_bits(d_bits, self.n, self.h, self.w, RHO, THETA, self.line_threshold(), LINES_MAX, 0.0, PI, *self.d)


# ---- dev_hough_segments_bits -----------------------------------------------------------------------------------------------
class Segments(Stage):
    variants = ("exclusive0", "exclusive1")

    def make_masks(self):
        return bi.line_masks(*self.shape)

    def prepare(self):
        self.lines = self.line_lists()
        self.geom = self.tables(self.w)

    def rule(self, variant, masks, width):
        """The lines and their cells are the caller's data and stay; the map is what widens."""
        return [hough_segments_rule.segments(m, b, *self.geom, MIN_LENGTH, MAX_GAP, int(variant[-1]))
                for m, b in zip(masks, self.lines)]

    def portable(self, value, width):
        return (np.array([len(s) for s in value]), _concat(value, 6))

    def alloc(self, ctx, variant):
        segs = self.value[variant]
        assert sum(len(s) for s in segs) >= self.n
        self.cap = max(len(s) for s in segs) + 2
        outs = bi.Outputs(ctx)
        self.d_lines = self.upload_lines(outs)
        self.d = (outs.add("segments", self.n * self.cap * 6, I32), outs.add("seg_counts", self.n, I32))
        want = dict(segments=bi.expected_bytes(self.n * self.cap * 6, I32, []),
                    seg_counts=bi.expected_bytes(self.n, I32, [len(s) for s in segs]))
        for f, s in enumerate(segs):
            bi.put(want["segments"], I32, f * self.cap * 6, s)
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_hough_segments_bits(d_bits, self.n, self.h, self.w, RHO, THETA, 0.0, PI, *self.d_lines, LINES_MAX, MIN_LENGTH,
                                    MAX_GAP, int(variant[-1]), self.d[0], self.cap, self.d[1])

    def host_forms(self):
        pass   # hough_segments_from_bits needs no GPU: tests/test_hough_segments_rule.py


# ---- dev_line_fits_bits ----------------------------------------------------------------------------------------------------
class LineFits(Stage):
    variants = ("u8-options0", "u8-options3", "s16-options0", "s16-options3")

    def make_masks(self):
        return bi.line_masks(*self.shape)

    def prepare(self):
        self.lines = self.line_lists()
        self.geom = self.tables(self.w)
        self.segs = [hough_segments_rule.segments(m, b, *self.geom, MIN_LENGTH, MAX_GAP, 0)
                     for m, b in zip(self.masks, self.lines)]
        assert sum(len(s) for s in self.segs) >= self.n
        self.cap = max(len(s) for s in self.segs) + 2
        self.planes = {"u8": bi.planes_for(self.masks, np.uint8), "s16": bi.planes_for(self.masks, np.int16)}

    @staticmethod
    def _split(variant):
        kind, options = variant.split("-options")
        return kind, int(options)

    def rule(self, variant, masks, width):
        kind, options = self._split(variant)
        planes = bi.widened_plane(self.planes[kind], width)
        return [line_fits_rule.line_fits(m, P, b, *self.geom, s, options)
                for m, P, b, s in zip(masks, planes, self.lines, self.segs)]

    def portable(self, value, width):
        return (_concat(value, 12),)

    def alloc(self, ctx, variant):
        kind, _ = self._split(variant)
        outs = bi.Outputs(ctx)
        self.d_lines = self.upload_lines(outs)
        segs = np.full((self.n, self.cap, 6), 0x7FFFFFF0, I32)   # unused slots: records that must never be read as valid
        for f, s in enumerate(self.segs):
            segs[f, :len(s)] = s
        self.d_in = (outs.up("plane", self.planes[kind]), outs.up("segs", segs),
                     outs.up("seg_counts", np.array([len(s) for s in self.segs], I32)))
        self.d_fits = outs.add("fits", self.n * self.cap * 12, I32)
        want = dict(fits=bi.expected_bytes(self.n * self.cap * 12, I32, []))
        for f, fit in enumerate(self.value[variant]):
            bi.put(want["fits"], I32, f * self.cap * 12, fit)
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        kind, options = self._split(variant)
        ctx.dev_line_fits_bits(d_bits, self.d_in[0], kind == "u8", self.n, self.h, self.w, RHO, THETA, 0.0, PI, *self.d_lines,
                               LINES_MAX, self.d_in[1], self.d_in[2], self.cap, options, self.d_fits)

    def host_forms(self):
        """line_fits_from_plane on a host map with dirty pad bits."""
        for pad in bi.PADS[1:]:
            bits = bi.packed(self.masks, pad, seed=self.h)
            for v in self.variants:
                kind, options = self._split(v)
                for f in range(self.n):
                    got = self.hip.line_fits_from_plane(bits[f], self.planes[kind][f], self.lines[f], self.segs[f], rho=RHO,
                                                        options=options)
                    assert np.array_equal(got, self.value[v][f]), f"line_fits_from_plane, pad bits {pad}, {v}, frame {f}"


# ---- dev_hough_circles_bits ------------------------------------------------------------------------------------------------
class Circles(Stage):
    def make_masks(self):
        return bi.circle_masks(*self.shape)

    def prepare(self):
        cx, cy, r = bi.circle_of(self.h, self.w)
        # min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max
        self.args = (max(1, r - 5), r + 2, 1 if r >= 8 else 0, max(1, r // 2), max(1, r // 3), max(1, r // 4), 24)
        y, x = np.mgrid[0:self.h, 0:self.w]
        # gradients that point away from the designed centre: every ring pixel votes for it
        self.gx = np.broadcast_to(((x - cx) * 8).astype(np.int16), self.shape).copy()
        self.gy = np.broadcast_to(((y - cy) * 8).astype(np.int16), self.shape).copy()

    def rule(self, variant, masks, width):
        gx, gy = bi.widened_plane(self.gx, width), bi.widened_plane(self.gy, width)
        acc = np.stack([hough_circles_rule.accumulate(m, a, b, *self.args[:3]) for m, a, b in zip(masks, gx, gy)])
        return acc, [hough_circles_rule.circles(m, a, *self.args) for m, a in zip(masks, acc)]

    def portable(self, value, width):
        _, per = value
        return (np.array([len(r) for r, _ in per]), np.array([p for _, p in per]), _concat([r[:, :5] for r, _ in per], 5))

    def alloc(self, ctx, variant):
        acc, per = self.value[variant]
        assert sum(len(r) for r, _ in per) >= 1
        cm = self.args[6]
        outs = bi.Outputs(ctx)
        self.d_grad = (outs.up("gx", self.gx), outs.up("gy", self.gy))
        self.d = (outs.add("circles", self.n * cm * 6, I32), outs.add("counts", self.n, I32),
                  outs.add("centre_counts", self.n, I32), outs.add("accum", acc.size, I32))
        want = dict(circles=bi.expected_bytes(self.n * cm * 6, I32, []),
                    counts=bi.expected_bytes(self.n, I32, [len(r) for r, _ in per]),
                    centre_counts=bi.expected_bytes(self.n, I32, [p for _, p in per]),
                    accum=bi.expected_bytes(acc.size, I32, acc))
        for f, (rec, _) in enumerate(per):
            bi.put(want["circles"], I32, f * cm * 6, rec)
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_hough_circles_bits(d_bits, *self.d_grad, self.n, self.h, self.w, *self.args, *self.d)

    def host_forms(self):
        """hough_circles_from_bits on a host map with dirty pad bits."""
        acc, per = self.value["only"]
        for pad in bi.PADS[1:]:
            bits = bi.packed(self.masks, pad, seed=self.h)
            for f in range(self.n):
                rec, peaks, got_acc = self.hip.hough_circles_from_bits(bits[f], self.gx[f], self.gy[f], self.h, self.w,
                                                                       *self.args, want_accum=True)
                what = f"hough_circles_from_bits, pad bits {pad}, frame {f}"
                assert np.array_equal(got_acc, acc[f]), what + ": accumulator"
                assert peaks == per[f][1] and np.array_equal(rec, per[f][0]), what + ": records"


# ---- dev_circle_fits_bits ----------------------------------------------------------------------------------------------------
class CircleFits(Stage):
    variants = ("u8-options0-trim0", "u8-options3-trim192", "s16-options0-trim0", "s16-options1-trim192")
    BAND = 2

    def make_masks(self):
        return bi.circle_masks(*self.shape)

    def prepare(self):
        cx, cy, r = bi.circle_of(self.h, self.w)
        # the caller's records: the designed circle, one half a pixel beside it, a small one centred on the last column
        recs = [(2 * cx, 2 * cy, r), (2 * cx + 1, 2 * cy - 1, r + 1), (2 * (self.w - 1), 2 * cy, max(1, r // 3))]
        self.recs = np.array([rec + (0, 0, 0) for rec in recs], I32)
        self.cm = len(recs) + 1
        self.planes = {"u8": bi.planes_for(self.masks, np.uint8), "s16": bi.planes_for(self.masks, np.int16)}

    @staticmethod
    def _split(variant):
        kind, options, trim = variant.split("-")
        return kind, int(options[len("options"):]), int(trim[len("trim"):])

    def rule(self, variant, masks, width):
        kind, options, trim = self._split(variant)
        planes = bi.widened_plane(self.planes[kind], width)
        return [circle_fits_rule.fits_of(m, P, self.recs, self.BAND, trim, options) for m, P in zip(masks, planes)]

    def portable(self, value, width):
        return (_concat(value, 8),)

    def alloc(self, ctx, variant):
        kind, _, _ = self._split(variant)
        fits = self.value[variant]
        assert not any((f[:, 4].view(U32) & circle_fits_rule.INVALID).any() for f in fits), "the records are valid ones"
        outs = bi.Outputs(ctx)
        recs = np.full((self.n, self.cm, 6), 0x7FFFFFF0, I32)
        recs[:, :len(self.recs)] = self.recs
        self.d_in = (outs.up("plane", self.planes[kind]), outs.up("recs", recs),
                     outs.up("counts", np.full(self.n, len(self.recs), I32)))
        self.d_fits = outs.add("fits", self.n * self.cm * 8, I32)
        want = dict(fits=bi.expected_bytes(self.n * self.cm * 8, I32, []))
        for f, fit in enumerate(fits):
            bi.put(want["fits"], I32, f * self.cm * 8, fit)
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        kind, options, trim = self._split(variant)
        ctx.dev_circle_fits_bits(d_bits, self.d_in[0], kind == "u8", self.n, self.h, self.w, self.d_in[1], self.d_in[2],
                                 self.cm, self.BAND, trim, options, self.d_fits)

    def host_forms(self):
        """circle_fits_from_plane on a host map with dirty pad bits."""
        for pad in bi.PADS[1:]:
            bits = bi.packed(self.masks, pad, seed=self.h)
            for v in self.variants:
                kind, options, trim = self._split(v)
                for f in range(self.n):
                    got = self.hip.circle_fits_from_plane(bits[f], self.planes[kind][f], self.recs, self.BAND, trim, options)
                    assert np.array_equal(got, self.value[v][f]), f"circle_fits_from_plane, pad bits {pad}, {v}, frame {f}"


# ---- dev_polygons_bits, dev_shapes_bits -------------------------------------------------------------------------------------
class _Contours(Stage):
    def make_masks(self):
        return bi.blob_masks(*self.shape)

    def contour_portable(self, ct, width):
        stats, off, chain, points, poff = ct
        return (np.delete(stats, FIRST, axis=1), bi.yx(stats[:, FIRST], width), off, chain, bi.yx(points, width), poff)

    def contour_outputs(self, outs, ct):
        stats, off, chain, points, poff = ct
        assert stats.shape[0] >= self.n and (stats[:, 0] + stats[:, 2] == self.w).any(), "a component on the last column"
        self.cap, self.pcap = stats.shape[0] + 2, points.size + 3
        d = (outs.add("stats", self.cap * 6, I32), self.cap, outs.add("offsets", self.n + 1, U64),
             outs.add("chain_offsets", self.cap + 1, U64), outs.add("points", self.pcap, I32), self.pcap,
             outs.add("point_offsets", self.n + 1, U64))
        want = dict(stats=bi.expected_bytes(self.cap * 6, I32, stats), offsets=bi.expected_bytes(self.n + 1, U64, off),
                    chain_offsets=bi.expected_bytes(self.cap + 1, U64, chain), points=bi.expected_bytes(self.pcap, I32, points),
                    point_offsets=bi.expected_bytes(self.n + 1, U64, poff))
        return d, want


class Polygons(_Contours):
    def rule(self, variant, masks, width):
        ct = contours_rule.csr(masks, MIN_AREA)
        return ct, polygons_rule.csr(ct[2], ct[3], ct[3].size, width, *TOLERANCE)

    def portable(self, value, width):
        ct, (voff, verts, meas) = value
        return self.contour_portable(ct, width) + (voff, bi.yx(verts, width), meas)

    def alloc(self, ctx, variant):
        ct, (voff, verts, meas) = self.value[variant]
        outs = bi.Outputs(ctx)
        self.d, want = self.contour_outputs(outs, ct)
        self.d2 = (outs.add("vertex_offsets", self.cap + 1, U64), outs.add("vertices", self.pcap, I32), self.pcap,
                   outs.add("measures", self.cap * 4, I64))
        want.update(vertex_offsets=bi.expected_bytes(self.cap + 1, U64, voff), vertices=bi.expected_bytes(self.pcap, I32, verts),
                    measures=bi.expected_bytes(self.cap * 4, I64, meas))
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_polygons_bits(d_bits, self.h, self.w, self.n, MIN_AREA, *self.d, *TOLERANCE, *self.d2)


class Shapes(_Contours):
    def rule(self, variant, masks, width):
        ct = contours_rule.csr(masks, MIN_AREA)
        return ct, shapes_rule.csr(ct[2], ct[3], ct[3].size, width)

    def portable(self, value, width):
        ct, (hoff, hull, meas) = value
        return self.contour_portable(ct, width) + (hoff, bi.yx(hull, width), np.delete(meas, shapes_rule.ANCHOR, axis=1),
                                                   bi.yx(meas[:, shapes_rule.ANCHOR], width))

    def alloc(self, ctx, variant):
        ct, (hoff, hull, meas) = self.value[variant]
        outs = bi.Outputs(ctx)
        self.d, want = self.contour_outputs(outs, ct)
        self.d2 = (outs.add("hull_offsets", self.cap + 1, U64), outs.add("hull", self.pcap, I32), self.pcap,
                   outs.add("measures", self.cap * shapes_rule.WORDS, I64))
        want.update(hull_offsets=bi.expected_bytes(self.cap + 1, U64, hoff), hull=bi.expected_bytes(self.pcap, I32, hull),
                    measures=bi.expected_bytes(self.cap * shapes_rule.WORDS, I64, meas))
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_shapes_bits(d_bits, self.h, self.w, self.n, MIN_AREA, *self.d, *self.d2)


# ---- dev_chamfer_bits ------------------------------------------------------------------------------------------------------
class Chamfer(Stage):
    variants = ("dist2-given", "dist2-null")
    ARGS = (160, 24, 2, 48)   # trunc_q4, max_mean_q4, min_dist, matches_max

    def make_masks(self):
        return bi.chamfer_masks(*self.shape)

    def prepare(self):
        self.templates = bi.chamfer_templates(self.h, self.w)

    def rule(self, variant, masks, width):
        key = ("rule", width, masks.tobytes())
        if getattr(self, "_memo", (None,))[0] != key:   # both variants have one value
            d2 = np.stack([chamfer_rule.dist2_of_mask(m) for m in masks])
            self._memo = (key, (d2, [chamfer_rule.matches(d, self.templates, *self.ARGS) for d in d2]))
        return self._memo[1]

    def portable(self, value, width):
        d2, per = value
        return (d2[..., :self.w], np.array([c for _, c, _ in per]), np.array([len(r) for r, _, _ in per]),
                _concat([r[:, :5] for r, _, _ in per], 5), np.stack([S[..., :self.w] for _, _, S in per]))

    def alloc(self, ctx, variant):
        d2, per = self.value[variant]
        best = [r[0] for r, _, _ in per]
        assert all(b[3] == 0 for b in best), "every frame holds the drawn template: a match of score 0"
        T, mm = len(self.templates), self.ARGS[3]
        outs = bi.Outputs(ctx)
        S = np.stack([s for _, _, s in per])
        self.d = (outs.add("matches", self.n * mm * 6, I32), outs.add("counts", self.n, I32),
                  outs.add("cand_counts", self.n, I32), outs.add("scores", S.size, U32))
        want = dict(matches=bi.expected_bytes(self.n * mm * 6, I32, []),
                    counts=bi.expected_bytes(self.n, I32, [len(r) for r, _, _ in per]),
                    cand_counts=bi.expected_bytes(self.n, I32, [c for _, c, _ in per]),
                    scores=bi.expected_bytes(S.size, U32, S))
        for f, (rec, _, _) in enumerate(per):
            bi.put(want["matches"], I32, f * mm * 6, rec)
        self.d_dist2 = 0
        if variant == "dist2-given":
            self.d_dist2 = outs.add("dist2", d2.size, I32)
            want["dist2"] = bi.expected_bytes(d2.size, I32, d2)
        self.cset = ctx.chamfer_set_create(self.templates)
        return outs, want

    def launch(self, ctx, outs, d_bits, variant):
        ctx.dev_chamfer_bits(d_bits, self.n, self.h, self.w, self.cset, *self.ARGS, *self.d, d_dist2=self.d_dist2)


STAGES = {"hough": Hough, "hough_segments": Segments, "line_fits": LineFits, "hough_circles": Circles,
          "circle_fits": CircleFits, "polygons": Polygons, "shapes": Shapes, "chamfer": Chamfer}
# No stage leaves a shape out: at 9 x 2 the circle stages take radii from 1, and the chamfer templates are a few points.


def run_placements(hip, stage):
    """Every variant of the stage under every placement of the map, on one context."""
    with hip.Context(0) as ctx:
        for variant in stage.variants:
            stage.setup(ctx, variant)
            outs, want = stage.alloc(ctx, variant)
            first = None
            try:
                for shift, filler, pad in bi.placements(stage.w):
                    what = f"{type(stage).__name__} {stage.shape} {variant}: shift {shift}, filler {filler:#04x}, pad bits {pad}"
                    placed = bi.Placed(ctx, bi.packed(stage.masks, pad, seed=stage.h), shift, filler)
                    try:
                        outs.refill()
                        stage.launch(ctx, outs, placed.ptr, variant)
                        got = outs.raw()   # (a blocking copy on the context's stream: the call has finished)
                        assert set(got) == set(want)
                        for key in want:
                            bad = np.flatnonzero(got[key] != want[key])
                            assert bad.size == 0, f"{what}: {key} differs from the rule in {bad.size} bytes, first at {bad[0]}"
                        placed.unchanged(what)
                        first = got if first is None else first
                        assert all(np.array_equal(got[k], first[k]) for k in first), f"{what}: other bytes than at shift 0"
                    finally:
                        placed.free()
            finally:
                outs.free()


@pytest.mark.parametrize("shape", bi.SHAPES, ids=bi.SHAPE_IDS)
@pytest.mark.parametrize("name", list(STAGES))
def test_bits_entry_point_at_odd_addresses_with_set_pad_bits(hip, name, shape):
    stage = STAGES[name](hip, shape)
    controls = stage.control()
    assert controls == (2 * len(stage.variants) if bi.pad_bits(shape[2]) else 0)
    stage.host_forms()
    run_placements(hip, stage)
