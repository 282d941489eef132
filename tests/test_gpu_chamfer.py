"""Chamfer template matching on the GPU (canny_hip_dev_chamfer_dist2 / _bits / canny_hip_dev_canny_chamfer /
canny_hip_canny_chamfer / canny_hip_dev_chamfer_costs) against the numpy restatement of the rule (tests/chamfer_rule.py):
every comparison is exact equality on whole arrays -- the score planes, the six-int records, the counts and the candidate
counts -- for both routes of the score kernel, with the scores asked for and not.  Every output buffer is pre-filled with
a sentinel and followed by a guard region; slots past counts[f] must keep the sentinel."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import chamfer_rule as cr
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_batch
from test_chamfer_rule import DISC_RECORDS, boundary_dist2, random_template
from test_hough_circles_rule import disc_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
DIRECT, TILED = 1, 2


def dist2_of(mask):
    h, w = mask.shape
    return capi.edt_from_bits(np.packbits(mask, axis=-1), h, w, True, False, False)[0]


class _Call:
    """Guarded device outputs of one matching call on n frames of h x w with T templates."""

    def __init__(self, ctx, n, h, w, T, matches_max, scores=True):
        self.ctx, self.n, self.h, self.w, self.T, self.mm = ctx, n, h, w, T, matches_max   # mm may be lowered per call
        self.ptrs = []
        self.sizes = dict(matches=n * matches_max * 6, counts=n, cands=n)
        if scores:
            self.sizes.update(scores=n * T * h * w)
        self.d = {k: self._filled(v) for k, v in self.sizes.items()}

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
        self.ctx.h2d(p, a)
        return p

    def refill(self):
        for k, v in self.sizes.items():
            self.ctx.h2d(self.d[k], np.full(v + N_GUARD, SENT, np.uint32))

    def tail(self, trunc, max_mean, min_dist):
        d = self.d
        return (trunc, max_mean, min_dist, self.mm, d["matches"], d["counts"], d["cands"], d.get("scores", 0))

    def get(self, key):
        words = self.sizes[key]
        out = np.empty(words + N_GUARD, np.uint32)
        self.ctx.d2h(out, self.d[key])
        return out[:words], bool((out[words:] == SENT).all())

    def check(self, want, what):
        """want: per frame (records, candidate count, S) of the rule.  -> the number of matches found."""
        out = {k: self.get(k) for k in self.sizes}
        for k, (_, guard) in out.items():
            assert guard, f"{what}: guard behind {k} overwritten"
        counts, cands = out["counts"][0].view(np.int32), out["cands"][0].view(np.int32)
        used = self.n * self.mm * 6
        rec = out["matches"][0][:used].reshape(self.n, self.mm, 6)
        assert (out["matches"][0][used:] == SENT).all(), f"{what}: records written past n_frames * matches_max slots"
        if "scores" in out:
            S = out["scores"][0].reshape(self.n, self.T, self.h, self.w)
            for f in range(self.n):
                assert np.array_equal(S[f], want[f][2]), f"{what} frame {f}: {int((S[f] != want[f][2]).sum())} scores differ"
        found = 0
        for f in range(self.n):
            w_rec, w_cand, _ = want[f]
            assert cands[f] == w_cand, f"{what} frame {f}: candidate count {cands[f]} != {w_cand}"
            assert counts[f] == len(w_rec), f"{what} frame {f}: count {counts[f]} != {len(w_rec)}"
            assert np.array_equal(rec[f, :len(w_rec)].view(np.int32), w_rec), f"{what} frame {f}: records"
            assert (rec[f, len(w_rec):] == SENT).all(), f"{what} frame {f}: slots past the count were written"
            found += len(w_rec)
        return found

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def want_of(d2, templates, trunc, max_mean, min_dist, mm, S_cache=None):
    out = []
    for f in range(len(d2)):
        S = None if S_cache is None else S_cache.get((f, trunc))
        rec, n_cand, S = cr.matches(d2[f], templates, trunc, max_mean, min_dist, mm, S=S)
        if S_cache is not None:
            S_cache[(f, trunc)] = S
        out.append((rec, n_cand, S))
    return out


# ---- the cost arithmetic -----------------------------------------------------------------------------------------------------
def test_cost_hook_at_every_boundary_of_the_root(hip):
    """1.5 M values in one launch: for each q in 1 .. 16 * 46341 the two dist2 around ceil(q^2 / 256), the untruncated
    root (the double root with its correction) and the cost pass's own function at four truncations."""
    d2 = boundary_dist2()
    root = np.array([math.isqrt(int(v) * 256) for v in d2], np.int64)
    with hip.Context(0) as ctx:
        d_in, d_out = ctx.malloc(d2.nbytes), ctx.malloc(4 * (len(d2) + N_GUARD))
        ctx.h2d(d_in, d2)
        for trunc in (0, 4095, 256, 255, 1):
            ctx.h2d(d_out, np.full(len(d2) + N_GUARD, SENT, np.uint32))
            ctx.dev_chamfer_costs(d_in, len(d2), trunc, d_out)
            got = np.empty(len(d2) + N_GUARD, np.uint32)
            ctx.d2h(got, d_out)
            assert (got[len(d2):] == SENT).all()
            want = root if trunc == 0 else np.minimum(root, trunc)
            assert np.array_equal(got[:len(d2)].astype(np.int64), want), f"trunc {trunc}"
        for bad, status in ((-1, 1), (4096, 2)):
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.dev_chamfer_costs(d_in, len(d2), bad, d_out)
            assert ei.value.status == status
        ctx.free(d_in)
        ctx.free(d_out)


# ---- dev_chamfer_dist2 -------------------------------------------------------------------------------------------------------
def _templates(rng, far):
    """K = 1 at the anchor (S is the cost plane); K = 63, 64, 65, 257 with negative offsets and duplicates; one whose dy span
    (and dx span) forces more than one band of the tiled kernel; with `far`, one that reaches +-255."""
    t = [np.array([[0, 0]], np.int16)] + [random_template(rng, k, 9) for k in (63, 64, 65, 257)]
    t.append(np.array([(x, y) for y in range(-60, 61, 5) for x in (-100, 0, 100)], np.int16))
    if far:
        t.append(np.array([(-255, -255), (255, 255), (-255, 255), (255, -255), (0, 0), (0, 0), (1, -1), (-255, 0), (0, 255),
                           (3, 2), (-2, 3), (17, -40)], np.int16))
    return t


def _maps(rng, n, h, w):
    """An empty map, a full map, one pixel in a corner, Bernoulli maps."""
    if n == 1:
        return [rng.random((h, w)) < 0.03]
    m = [np.zeros((h, w), bool), np.ones((h, w), bool), np.zeros((h, w), bool)]
    m[2][h - 1, 0] = True
    return m + [rng.random((h, w)) < d for d in (0.01, 0.2)][:n - 3]


COMBOS = [  # trunc_q4, max_mean_q4, min_dist, matches_max
    (1, 0, 0, 7), (255, 254, 6, 7), (256, 100, 0, 1), (4095, 1500, 1000, 4096), (160, 159, 6, 4096), (160, 40, 0, 5)]


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (70, 1), (33, 65), (97, 131), (64, 128)], ids=lambda v: str(v))
def test_dist2_planes_both_routes_with_and_without_scores(hip, h, w, n):
    rng = np.random.default_rng(1000 * h + w + n)
    templates = _templates(rng, far=(h, w) == (33, 65))
    masks = _maps(rng, n, h, w)
    d2 = np.stack([dist2_of(m) for m in masks])
    bands = [capi.chamfer_bands(templates, t)[0] for t in range(len(templates))]
    assert bands[0] == 1 and bands[5] > 1 and capi.chamfer_bands(templates)[3] == TILED
    cache, found, tied, over = {}, 0, 0, 0
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create(templates)
        calls = {s: _Call(ctx, n, h, w, len(templates), 4096, scores=s) for s in (True, False)}
        d_d2 = calls[True].upload(d2)
        for trunc, max_mean, min_dist, mm in COMBOS:
            want = want_of(d2, templates, trunc, max_mean, min_dist, mm, cache)
            for f in range(n):
                assert np.array_equal(want[f][2][0], cr.cost_plane(d2[f], trunc))     # K = 1 at (0, 0): the cost plane
                cand = cr.candidates(want[f][2], templates, max_mean)
                over += len(cand) > mm
                tied += len(cand) > mm and cand[mm - 1][0] == cand[mm][0]
            for route in (DIRECT, TILED):
                ctx.set_option("chamfer_route", route)
                for with_scores in (True, False):
                    c = calls[with_scores]
                    c.mm = mm
                    c.refill()
                    ctx.dev_chamfer_dist2(d_d2, n, h, w, cset, *c.tail(trunc, max_mean, min_dist))
                    found += c.check(want, f"{n}x{h}x{w} route {route} scores {with_scores} "
                                           f"{trunc}/{max_mean}/{min_dist}/{mm}")
        ctx.chamfer_set_destroy(cset)
        for c in calls.values():
            c.free()
    if h * w > 2000:
        assert found > 0
    if (h, w) in ((97, 131), (64, 128)):
        assert over > 0 and tied > 0, "no case cut inside a run of equal mean_q12"


def test_refused_calls_write_nothing(hip):
    d2 = np.zeros((1, 8, 8), np.int32)
    with hip.Context(0) as ctx, hip.Context(0) as other:
        cset = ctx.chamfer_set_create([np.array([[0, 0], [1, 1]], np.int16)])
        foreign = other.chamfer_set_create([np.array([[0, 0]], np.int16)])
        c = _Call(ctx, 1, 8, 8, 1, 4)
        d_d2 = c.upload(d2)
        ok = dict(d=d_d2, n=1, h=8, w=8, s=cset, trunc=160, mean=24, dist=0)

        def run(**kw):
            a = dict(ok, **kw)
            t = list(c.tail(a["trunc"], a["mean"], a["dist"]))
            if "mm" in a:
                t[3] = a["mm"]
            if a.get("no_counts"):
                t[5] = 0
            ctx.dev_chamfer_dist2(a["d"], a["n"], a["h"], a["w"], a["s"], *t)

        for kw, status in [(dict(d=0), 1), (dict(s=0), 1), (dict(s=foreign), 1), (dict(no_counts=True), 1), (dict(h=0), 1),
                           (dict(n=0), 1), (dict(trunc=0), 1), (dict(mean=160), 1), (dict(mean=-1), 1), (dict(dist=-1), 1),
                           (dict(mm=0), 1), (dict(trunc=4096), 2), (dict(mm=4097), 2), (dict(h=65536, w=1), 2)]:
            with pytest.raises(hip.CannyHipError) as ei:
                run(**kw)
            assert ei.value.status == status, kw
        ctx.synchronize()
        for k in c.sizes:
            got, guard = c.get(k)
            assert guard and (got == SENT).all(), f"a refused call wrote {k}"
        for csr, status in [((np.array([0, 0], np.int32), np.zeros((1, 2), np.int16)), 1),
                            ((np.array([1, 2], np.int32), np.zeros((2, 2), np.int16)), 1),
                            ((np.array([0, 1], np.int32), np.array([[256, 0]], np.int16)), 2),
                            ((np.arange(1026, dtype=np.int32), np.zeros((1025, 2), np.int16)), 2)]:
            with pytest.raises(hip.CannyHipError) as ei:
                ctx.chamfer_set_create(csr=csr)
            assert ei.value.status == status
        with pytest.raises(hip.CannyHipError):
            ctx.chamfer_set_destroy(foreign)
        ctx.chamfer_set_destroy(cset)
        with pytest.raises(hip.CannyHipError):
            ctx.chamfer_set_destroy(cset)    # no longer a set of this context
        with pytest.raises(hip.CannyHipError) as ei:
            run()                            # ... nor one to match with: refused by its address, the handle is not read
        assert ei.value.status == 1
        ctx.synchronize()
        for k in c.sizes:
            got, guard = c.get(k)
            assert guard and (got == SENT).all(), f"a call with a destroyed set wrote {k}"
        c.free()                             # `foreign` dies with its context


# ---- behind the detector -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synth_case(n, h, w):
    frames = synth_batch(n, h, w, seed=7)
    masks = np.stack([oracle.canny(f, 1.4, 50, 150) != 0 for f in frames])
    d2 = np.stack([dist2_of(m) for m in masks])
    rng = np.random.default_rng(h)
    templates = [cr.ring_template(5), cr.ring_template(8), random_template(rng, 64, 7)]
    return frames, masks, d2, templates


@pytest.mark.parametrize("n,h,w", [(3, 97, 131), (1, 270, 480)], ids=lambda v: str(v))
def test_bits_and_canny_forms_against_the_rule_on_the_oracles_map(hip, n, h, w):
    frames, masks, d2, templates = _synth_case(n, h, w)
    args = (160, 60, 8)
    want = want_of(d2, templates, *args, 64)
    assert sum(len(r) for r, _, _ in want) > 0
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create(templates)
        c = _Call(ctx, n, h, w, len(templates), 64)
        d_bits, d_img = c.upload(np.packbits(masks, axis=-1)), c.upload(frames)
        px = n * h * w
        d_edges, d_dist2 = c._filled(px // 2 + 1), c._filled(px)
        ref_edges, ref_dist2 = c._malloc(2 * px), c._malloc(4 * px)
        ctx.dev_canny_edt(d_img, 1.4, 50, 150, h, w, n, ref_dist2, 0, 0, d_edges=ref_edges)
        e_want, d_want = np.empty((n, h, w), np.int16), np.empty((n, h, w), np.int32)
        ctx.d2h(e_want, ref_edges)
        ctx.d2h(d_want, ref_dist2)
        assert np.array_equal(d_want, d2) and np.array_equal(e_want != 0, masks)
        for route in (DIRECT, TILED, 0):
            ctx.set_option("chamfer_route", route)
            c.refill()
            ctx.dev_chamfer_bits(d_bits, n, h, w, cset, *c.tail(*args))
            c.check(want, f"bits route {route}")
            c.refill()
            ctx.dev_chamfer_bits(d_bits, n, h, w, cset, *c.tail(*args), d_dist2=d_dist2)
            c.check(want, f"bits route {route}, caller's dist2")
            got = np.empty((n, h, w), np.int32)
            ctx.d2h(got, d_dist2)
            assert np.array_equal(got, d2)
            c.refill()
            ctx.dev_canny_chamfer(d_img, 1.4, 50, 150, h, w, n, cset, *c.tail(*args))
            c.check(want, f"canny route {route}, workspaces")
            c.refill()
            ctx.h2d(d_dist2, np.full(px, SENT, np.uint32))
            ctx.dev_canny_chamfer(d_img, 1.4, 50, 150, h, w, n, cset, *c.tail(*args), d_edges=d_edges, d_dist2=d_dist2)
            c.check(want, f"canny route {route}, caller's planes")
            e_got = np.empty((n, h, w), np.int16)
            ctx.d2h(got, d_dist2)
            ctx.d2h(e_got, d_edges)
            assert np.array_equal(got, d_want) and np.array_equal(e_got, e_want), "not what dev_canny_edt gives alone"
        # max_val = 300 empties every map: all counts 0, every score trunc_q4 * K
        c.refill()
        ctx.dev_canny_chamfer(d_img, 1.4, 50, 300, h, w, n, cset, *c.tail(*args))
        empty = want_of(np.full((n, h, w), cr.EDT_NONE, np.int32), templates, *args, 64)
        assert all(len(r) == 0 and k == 0 for r, k, _ in empty)
        c.check(empty, "max_val 300")
        ctx.chamfer_set_destroy(cset)
        c.free()


def test_host_form_finds_the_discs(hip):
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create([cr.ring_template(r) for r in (20, 12, 9)])
        for route in (0, DIRECT, TILED):
            ctx.set_option("chamfer_route", route)
            matches, cands = ctx.canny_chamfer(disc_frame(), 1.4, 50, 150, cset, 160, 24, min_dist=8, matches_max=256)
            assert len(matches) == 1 and cands[0] >= 3
            assert matches[0].view(np.int32).reshape(-1, 6).tolist() == DISC_RECORDS
            assert [(int(m["y"]), int(m["x"]), int(m["template"])) for m in matches[0]] == [(60, 96, 1), (20, 100, 2),
                                                                                           (40, 44, 0)]
        batch = np.stack([disc_frame(), np.zeros((96, 128), np.uint8), disc_frame()[::-1].copy()])
        matches, cands = ctx.canny_chamfer(batch, 1.4, 50, 150, cset, 160, 24, min_dist=8, matches_max=2)
        assert [len(m) for m in matches] == [2, 0, 2] and cands[1] == 0
        assert matches[0].view(np.int32).reshape(-1, 6).tolist() == DISC_RECORDS[:2]


# ---- one context, many calls ----------------------------------------------------------------------------------------------------
def test_context_reuse_with_alternating_shapes_and_sets(hip):
    """The dirty-workspace discipline of DESIGN.md section 20: no call may read what an earlier call left.  Shapes and sets
    alternate, a set is destroyed between calls and a larger one created, the routes alternate too."""
    rng = np.random.default_rng(99)
    small = [random_template(rng, 5, 3), np.array([[0, 0]], np.int16)]
    large = [random_template(rng, 200, 30), random_template(rng, 70, 12), cr.ring_template(6), random_template(rng, 9, 60)]
    shapes = [(2, 70, 90), (1, 33, 200), (3, 20, 20), (2, 70, 90)]
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create(small)
        current = small
        for step in range(8):
            n, h, w = shapes[step % len(shapes)]
            if step in (3, 6):
                ctx.chamfer_set_destroy(cset)
                current = large if step == 3 else small
                cset = ctx.chamfer_set_create(current)
            masks = rng.random((n, h, w)) < (0.02 if step % 2 else 0.15)
            d2 = np.stack([dist2_of(m) for m in masks])
            mm = (3, 4096, 17)[step % 3]
            args = ((160, 100, 4), (255, 254, 0), (4095, 900, 9))[step % 3]
            ctx.set_option("chamfer_route", (TILED, DIRECT)[step % 2])
            c = _Call(ctx, n, h, w, len(current), mm, scores=step % 4 == 0)
            d_bits = c.upload(np.packbits(masks, axis=-1))
            ctx.dev_chamfer_bits(d_bits, n, h, w, cset, *c.tail(*args))
            c.check(want_of(d2, current, *args, mm), f"step {step}")
            c.free()


# ---- past the caps of the capped grids ----------------------------------------------------------------------------------------
def test_the_cost_pass_takes_a_second_trip(hip):
    n, h, w = 2, 1500, 1500
    plan, chunk = capi.chamfer_plan("cost", n, h, w, 1)
    assert chunk == n and plan.units == n * h * w and plan.grid == 16384 and plan.trips == 2
    assert plan.units % (plan.grid * plan.per_group) != 0, "the last trip is partial"
    rng = np.random.default_rng(5)
    d2 = rng.integers(0, 40, (n, h, w)).astype(np.int32)
    d2[1, -1, -1] = 0
    templates = [np.array([[0, 0]], np.int16)]
    want = want_of(d2, templates, 90, 50, 3, 64)
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create(templates)
        c = _Call(ctx, n, h, w, 1, 64)
        d_d2 = c.upload(d2)
        for route in (DIRECT, TILED):
            ctx.set_option("chamfer_route", route)
            c.refill()
            ctx.dev_chamfer_dist2(d_d2, n, h, w, cset, *c.tail(90, 50, 3))
            assert c.check(want, f"route {route}") > 100
        c.free()


def test_the_cell_passes_take_a_second_trip(hip):
    """The direct score kernel, the four histogram passes and the collect pass share one plan: T * h * w anchors of a frame."""
    n, h, w, T = 2, 520, 520, 2
    plan, chunk = capi.chamfer_plan("cells", n, h, w, T)
    assert chunk == n and plan.units == T * h * w and plan.grid == 2048 and plan.trips == 2
    assert plan.units % (plan.grid * plan.per_group) != 0
    rng = np.random.default_rng(6)
    masks = rng.random((n, h, w)) < 0.002
    masks[0, :260] = False                      # the matches of frame 0 lie in the second trip's anchors
    d2 = np.stack([dist2_of(m) for m in masks])
    templates = [np.array([[0, 0], [3, 1]], np.int16), np.array([[0, 0], [-2, 2], [0, 0]], np.int16)]
    want = want_of(d2, templates, 160, 30, 5, 300)
    assert all(k > 300 for _, k, _ in want)
    with hip.Context(0) as ctx:
        cset = ctx.chamfer_set_create(templates)
        for with_scores in (True, False):
            c = _Call(ctx, n, h, w, T, 300, scores=with_scores)
            d_d2 = c.upload(d2)
            for route in (DIRECT, TILED):
                ctx.set_option("chamfer_route", route)
                c.refill()
                ctx.dev_chamfer_dist2(d_d2, n, h, w, cset, *c.tail(160, 30, 5))
                assert c.check(want, f"route {route} scores {with_scores}") > 0
            c.free()


def test_a_batch_walked_in_several_chunks(hip):
    """Without d_scores the scores of a chunk of frames live in a workspace; "tune_chamfer_chunk_mb" shrinks its budget
    (256 MiB by default) so that 5 frames are walked as 3 + 2, and frame f's outputs still land in frame f's slots.  A
    chunk never holds more than 4096 frames either: 4100 tiny frames are walked as 4096 + 4."""
    rng = np.random.default_rng(8)
    n, h, w = 5, 97, 131
    templates = _templates(rng, far=False)
    d2 = np.stack([dist2_of(m) for m in _maps(rng, n, h, w)])
    want = want_of(d2, templates, 160, 100, 6, 32)
    with hip.Context(0) as ctx:
        ctx.set_option("tune_chamfer_chunk_mb", 1)
        cset = ctx.chamfer_set_create(templates)
        c = _Call(ctx, n, h, w, len(templates), 32, scores=False)
        d_d2 = c.upload(d2)
        for route in (DIRECT, TILED):
            ctx.set_option("chamfer_route", route)
            c.refill()
            ctx.dev_chamfer_dist2(d_d2, n, h, w, cset, *c.tail(160, 100, 6))
            assert c.check(want, f"3 + 2 frames, route {route}") > 0
        c.free()
        ctx.chamfer_set_destroy(cset)
        ctx.set_option("tune_chamfer_chunk_mb", 0)
        n, h, w = 4100, 2, 2
        assert capi.chamfer_plan("cells", n, h, w, 1)[1] == 4096
        d2 = rng.integers(0, 3, (n, h, w)).astype(np.int32)
        one = [np.array([[0, 0]], np.int16)]
        want = want_of(d2, one, 160, 20, 0, 2)
        cset = ctx.chamfer_set_create(one)
        c = _Call(ctx, n, h, w, 1, 2)
        ctx.dev_chamfer_dist2(c.upload(d2), n, h, w, cset, *c.tail(160, 20, 0))
        assert c.check(want, "4096 + 4 frames") > n
        c.free()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, np.uint8).tobytes())


def test_main_x_writes_the_matches_of_the_rule(tmp_path):
    """Main -x on a PGM written here: the shapes are the non-zero pixels of two PGM files, anchored at the centre."""
    frame = disc_frame()
    shapes = []
    for k, r in enumerate((12, 9)):
        m = np.zeros((2 * r + 3, 2 * r + 5), np.uint8)          # centre (r + 2, r + 1): the anchor is (w // 2, h // 2)
        for dx, dy in cr.ring_template(r):
            m[m.shape[0] // 2 + dy, m.shape[1] // 2 + dx] = 200
        _write_pgm(tmp_path / f"shape{k}.pgm", m)
        shapes.append(capi.chamfer_template_from_mask(m))
        assert sorted(map(tuple, shapes[-1].tolist())) == sorted(map(tuple, cr.ring_template(r).tolist()))
    _write_pgm(tmp_path / "frame.pgm", frame)
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    spec = f"{tmp_path / 'shape0.pgm'}:{tmp_path / 'shape1.pgm'},160,24,8"
    r = subprocess.run([exe, "1.4", "50", "150", "-i", str(tmp_path / "frame.pgm"), "-o", str(tmp_path), "-x", spec],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    mask = oracle.canny(frame, 1.4, 50, 150) != 0
    want, _, _ = cr.matches(dist2_of(mask), shapes, 160, 24, 8, 256)
    assert len(want) == 2
    lines = (tmp_path / "canny_matches.txt").read_text().splitlines()
    assert lines == [f"0 {x} {y} {t} {s} {m / 4096:.4f}" for x, y, t, s, m, _ in want.tolist()]
