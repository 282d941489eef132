"""Corner descriptors and Hamming matching on the GPU (canny_hip_dev_canny_corner_descriptors,
canny_hip_dev_corner_descriptors, canny_hip_canny_corner_descriptors, canny_hip_dev_match_descriptors)
against tests/descriptors_rule.py applied to the oracle's smoothed plane or to the plane and the sets the call is given.
Every comparison is exact equality on whole arrays; every output buffer is sentinel-filled with guard words behind it."""
import os
import subprocess

import numpy as np
import pytest

import corners_rule as cr
import descriptors_rule as dr
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
SIGMA, LO, HI = 1.4, 50, 150
CORNER_ARGS = (0, 5, 0, 2000, 0, 6)   # mode, block, k_q8, quality_q16, min_response, min_dist


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard words behind each, and plain uploads."""

    def __init__(self, ctx):
        self.ctx, self.words, self.ptrs = ctx, {}, []

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

    def refill(self):
        for p, words in self.words.items():
            self.ctx.h2d(p, np.full(words + N_GUARD, SENT, np.uint32))

    def get(self, p, what=""):
        out = np.empty(self.words[p] + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[self.words[p]:] == SENT).all(), f"guard words overwritten behind {what}"
        return out[:self.words[p]]

    def untouched(self):
        for p in self.words:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def raw(self):
        return b"".join(self.get(p).tobytes() for p in self.words)

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def check_descriptors(b, d_desc, d_meta, planes, records, counts, cmax, steered, what=""):
    """The descriptor outputs against the rule on planes[f] for records [n, cmax, 4] and counts; slots past the counts hold
    the sentinel.  Returns the meta words of the filled slots."""
    n = len(planes)
    desc = b.get(d_desc, "the descriptors").view(np.uint64).reshape(n, cmax, 4)
    meta = b.get(d_meta, "the meta words").view(np.int32).reshape(n, cmax)
    metas = []
    for f in range(n):
        k = int(counts[f])
        want, want_meta = dr.describe(planes[f], records[f, :k, :2], steered)
        assert np.array_equal(meta[f, :k], want_meta), f"{what}: frame {f}: meta words differ"
        bad = np.flatnonzero((desc[f, :k] != want).any(1))
        assert bad.size == 0, f"{what}: frame {f}: {bad.size} descriptors differ, first slot {bad[0]}"
        assert (desc[f, k:].view(np.uint32) == SENT).all() and (meta[f, k:].view(np.uint32) == SENT).all(), \
            f"{what}: frame {f}: slots past the count were written"
        metas.append(want_meta)
    return np.concatenate(metas) if metas else np.zeros(0, np.int32)


_REF = {}


def reference(h, w):
    """(frames, maps, the oracle's smoothed planes) of three frames of a shape, one of them flat; computed once, never
    modified."""
    if (h, w) not in _REF:
        frames = np.stack([synth_frame(h, w, s) for s in (1, 2, 3)])
        frames[1 if w == 77 else 2] = 90
        maps = np.stack([oracle.canny(f, SIGMA, LO, HI) for f in frames])
        planes = np.stack([oracle.gaussian(f, SIGMA) for f in frames])
        assert planes.min() >= 0 and planes.max() <= 255
        for a in (frames, maps, planes):
            a.setflags(write=False)
        _REF[(h, w)] = (frames, maps, planes)
    return _REF[(h, w)]


_CORNERS = {}


def reference_corners(h, w, cmax):
    if (h, w, cmax) not in _CORNERS:
        _CORNERS[(h, w, cmax)] = [cr.corners(P, *CORNER_ARGS, cmax) for P in reference(h, w)[2]]
    return _CORNERS[(h, w, cmax)]


# ---- descriptors: routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("h,w", [(70, 128), (70, 77)], ids=["70x128", "70x77"])
def test_behind_dev_canny_equals_the_rule_on_the_oracles_planes(hip, h, w, u8, fuse):
    frames, maps, planes = reference(h, w)
    cmax = 40
    want = reference_corners(h, w, cmax)
    with hip.Context(0) as ctx:
        ctx.set_option("smoothed_u8", u8)
        ctx.set_option("fuse_classify", fuse)
        b = _Bufs(ctx)
        d_img = b.upload(frames)
        # what dev_canny_corners gives: the corner outputs and d_edges must be exactly these
        ref = [b.filled(8 * 3 * cmax), b.filled(3), b.filled(3), b.filled(6), b.filled((3 * h * w + 1) // 2)]
        ctx.dev_canny_corners(d_img, SIGMA, LO, HI, h, w, 3, *CORNER_ARGS, cmax, ref[0], ref[1], ref[2], ref[3], 0, ref[4])
        ref_bytes = [b.get(p).tobytes() for p in ref]
        counts = b.get(ref[1]).view(np.int32)
        records = b.get(ref[0]).view(np.int64).reshape(3, cmax, 4)
        assert counts.tolist() == [len(r) for r, _, _, _ in want] and counts.sum() > 10
        for f in range(3):
            assert np.array_equal(records[f, :counts[f]], want[f][0])
        edges = b.get(ref[4]).view(np.int16)[:3 * h * w].reshape(3, h, w)
        assert np.array_equal(edges, maps)
        out = [b.filled(8 * 3 * cmax), b.filled(3), b.filled(3), b.filled(6), b.filled((3 * h * w + 1) // 2)]
        d_desc, d_meta = b.filled(8 * 3 * cmax), b.filled(3 * cmax)
        for steered in (0, 1):
            for p in out + [d_desc, d_meta]:
                ctx.h2d(p, np.full(b.words[p] + N_GUARD, SENT, np.uint32))
            ctx.dev_canny_corner_descriptors(d_img, SIGMA, LO, HI, h, w, 3, *CORNER_ARGS, cmax, out[0], out[1], d_desc,
                                             d_meta, steered, out[2], out[3], 0, out[4])
            assert ctx.get_option("last_canny_smoothed_u8") == (1 if u8 and fuse and w % 8 == 0 else 0)
            assert [b.get(p).tobytes() for p in out] == ref_bytes, "the corner outputs differ from dev_canny_corners'"
            meta = check_descriptors(b, d_desc, d_meta, planes, records, counts, cmax, steered, f"steered {steered}")
            if steered:
                assert len(set((meta & 255).tolist())) > 3
            else:
                assert not (meta & 255).any()
        b.free()


# ---- descriptors: a caller's plane ----------------------------------------------------------------------------------------
def border_records(h, w):
    xs = sorted({0, 1, 14, 15, 16, w // 2, w - 17, w - 16, w - 15, w - 2, w - 1} & set(range(w)))
    ys = sorted({0, 1, 14, 15, 16, h // 2, h - 17, h - 16, h - 15, h - 2, h - 1} & set(range(h)))
    inside = [(x, y) for y in ys for x in xs]
    outside = [(-1, 0), (0, -1), (w, 0), (0, h), (w + 100, h + 100), (-(1 << 40), 3), (3, 1 << 40), (-1, -1)]
    return np.array(inside + outside, np.int64)


def records_of(xy_per_frame, cmax):
    """int64 [n, cmax, 4] records (x, y, junk response, junk rank) and their counts; unused slots hold positions a kernel
    that ignored the counts would describe."""
    n = len(xy_per_frame)
    rec = np.full((n, cmax, 4), 3, np.int64)
    counts = np.zeros(n, np.int32)
    for f, xy in enumerate(xy_per_frame):
        rec[f, :len(xy), :2] = xy
        rec[f, :len(xy), 2] = -5 - np.arange(len(xy))
        counts[f] = len(xy)
    return rec, counts


@pytest.mark.parametrize("h,w", [(2, 2), (16, 31), (40, 52), (33, 70)], ids=["2x2", "16x31", "40x52", "33x70"])
def test_a_callers_plane_with_records_on_every_border_and_outside(hip, h, w):
    rng = np.random.default_rng(h * 100 + w)
    planes = np.stack([rng.integers(0, 256, (h, w), dtype=np.uint8), cr.blur14641(rng.integers(0, 256, (h, w), dtype=np.uint8)),
                       np.full((h, w), 200, np.uint8)])
    all_xy = border_records(h, w)
    # odd counts: the last waves of the last workgroup have no corner; an empty frame; capacity exact
    half = all_xy[::2]
    xy = [all_xy, all_xy[:0], half[:len(half) - 1 + len(half) % 2]]
    assert len(xy[2]) % 2 == 1
    cmax = len(all_xy)
    rec, counts = records_of(xy, cmax)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_plane, d_rec, d_cnt = b.upload(planes), b.upload(rec), b.upload(counts)
        d_desc, d_meta = b.filled(8 * 3 * cmax), b.filled(3 * cmax)
        for steered in (0, 1):
            b.refill()
            ctx.dev_corner_descriptors(d_plane, 3, h, w, d_rec, d_cnt, cmax, d_desc, d_meta, steered)
            meta = check_descriptors(b, d_desc, d_meta, planes, rec, counts, cmax, steered, f"{h}x{w} steered {steered}")
            assert (meta == -1).sum() >= 8 + 3 and (meta >= 0).sum() > 3
        # corners_max 1: one record a frame
        rec1, counts1 = records_of([all_xy[:1], all_xy[3:4], all_xy[-1:]], 1)
        d1, m1 = b.filled(8 * 3), b.filled(3)
        ctx.dev_corner_descriptors(d_plane, 3, h, w, b.upload(rec1), b.upload(counts1), 1, d1, m1, 1)
        check_descriptors(b, d1, m1, planes, rec1, counts1, 1, 1, "corners_max 1")
        b.free()


def test_the_describe_launch_takes_a_second_trip(hip):
    """One wave a slot, four a workgroup, 2048 workgroups at most: 3 x 4096 slots on a small plane are past the cap."""
    n, h, w, cmax = 3, 16, 31, 4096
    assert capi.descriptors_plan("describe", 2, cmax).trips == 1
    plan = capi.descriptors_plan("describe", n, cmax)
    assert (plan.units, plan.per_group, plan.grid, plan.trips) == (n * cmax, 4, 2048, 2)
    rng = np.random.default_rng(4)
    planes = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    xy = [np.stack([rng.integers(-1, w + 1, k), rng.integers(-1, h + 1, k)], 1) for k in (4096, 4095, 4093)]
    rec, counts = records_of(xy, cmax)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_desc, d_meta = b.filled(8 * n * cmax), b.filled(n * cmax)
        ctx.dev_corner_descriptors(b.upload(planes), n, h, w, b.upload(rec), b.upload(counts), cmax, d_desc, d_meta, 1)
        meta = check_descriptors(b, d_desc, d_meta, planes, rec, counts, cmax, 1, "past the cap")
        assert (meta == -1).sum() > 100 and (meta >= 0).sum() > 10000
        b.free()


def test_the_contexts_plane_and_the_refused_descriptor_calls(hip):
    h, w, cmax = 70, 128, 12
    frames, _, planes = reference(h, w)
    rng = np.random.default_rng(9)
    rec, counts = records_of([np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], 1) for k in (12, 5, 7)], cmax)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_rec, d_cnt = b.upload(frames), b.upload(rec), b.upload(counts)
        d_desc, d_meta = b.filled(8 * 3 * cmax), b.filled(3 * cmax)
        with pytest.raises(capi.CannyHipError) as ei:   # a context that ran no canny call has no plane
            ctx.dev_corner_descriptors(0, 3, h, w, d_rec, d_cnt, cmax, d_desc, d_meta)
        assert ei.value.status == 1
        d_edges = b.upload(np.zeros((3, h, w), np.int16))
        for u8 in (0, 1):
            ctx.set_option("smoothed_u8", u8)
            ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, 3, d_edges)
            b.refill()
            ctx.dev_corner_descriptors(0, 3, h, w, d_rec, d_cnt, cmax, d_desc, d_meta, 1)
            check_descriptors(b, d_desc, d_meta, planes, rec, counts, cmax, 1, f"the context's plane, smoothed_u8 {u8}")
        b.refill()
        for n2, h2, w2 in ((2, h, w), (3, h - 1, w), (3, w, h)):   # ... nor one of another shape
            with pytest.raises(capi.CannyHipError) as ei:
                ctx.dev_corner_descriptors(0, n2, h2, w2, d_rec, d_cnt, cmax, d_desc, d_meta)
            assert ei.value.status == 1
        d_plane = b.upload(planes.astype(np.uint8))
        outs = [b.filled(8 * 3 * cmax), b.filled(3)]

        def refused(status, n=3, hh=h, ww=w, rec_=d_rec, cnt=d_cnt, cm=cmax, desc=d_desc, meta=d_meta, opt=0):
            for call in (lambda: ctx.dev_corner_descriptors(d_plane, n, hh, ww, rec_, cnt, cm, desc, meta, opt),
                         lambda: ctx.dev_canny_corner_descriptors(d_img, SIGMA, LO, HI, hh, ww, n, *CORNER_ARGS, cm,
                                                                  outs[0] if rec_ == d_rec else rec_,
                                                                  outs[1] if cnt == d_cnt else cnt, desc, meta, opt)):
                with pytest.raises(capi.CannyHipError) as ei:
                    call()
                assert ei.value.status == status, (status, n, hh, ww, cm, opt)

        for kw in (dict(rec_=0), dict(cnt=0), dict(desc=0), dict(meta=0), dict(cm=0), dict(cm=-1), dict(opt=2), dict(opt=-1),
                   dict(hh=1), dict(ww=1), dict(n=0), dict(desc=d_desc + 4), dict(rec_=d_rec + 4)):
            refused(1, **kw)
        for kw in (dict(cm=4097), dict(hh=65535, ww=32769), dict(n=65536)):
            refused(2, **kw)
        # the corners' own refusals come before anything is queued, too
        with pytest.raises(capi.CannyHipError) as ei:
            ctx.dev_canny_corner_descriptors(d_img, SIGMA, LO, HI, h, w, 3, 0, 4, 0, 2000, 0, 6, cmax, outs[0], outs[1],
                                             d_desc, d_meta)
        assert ei.value.status == 1
        b.untouched()
        b.free()


# ---- the matcher -------------------------------------------------------------------------------------------------------------
SETTINGS = [(64, 205, 1), (256, 0, 0), (0, 0, 1), (100, 256, 0), (40, 1, 1)]


def pack_sets(sets, stride):
    """uint64 [frames, stride, 4] (unused slots: a descriptor that would match everything) and int32 counts."""
    words = np.zeros((len(sets), stride, 4), np.uint64)
    counts = np.zeros(len(sets), np.int32)
    for f, s in enumerate(sets):
        words[f, :len(s)] = s
        counts[f] = len(s)
    return words, counts


_WANT = {}


def want_match(key, q, t, setting):
    k = (key, setting)
    if k not in _WANT:
        _WANT[k] = dr.match(q, t, *setting)
    return _WANT[k]


def run_and_check(ctx, b, name, q_sets, stride_q, t_sets, stride_t, pairs, setting, same=False, bufs=None):
    """One match call on uploaded sets against the rule, pair by pair.  Returns the outputs' bytes."""
    qw, qc = pack_sets(q_sets, stride_q)
    if bufs is None:
        d_q, d_qc = b.upload(qw), b.upload(qc)
        if same:
            d_t, d_tc = d_q, d_qc
        else:
            tw, tc = pack_sets(t_sets, stride_t)
            d_t, d_tc = b.upload(tw), b.upload(tc)
        bufs = (d_q, d_qc, d_t, d_tc, b.filled(len(pairs) * stride_q * 4), b.filled(len(pairs)))
    d_q, d_qc, d_t, d_tc, d_m, d_pc = bufs
    for p in (d_m, d_pc):
        ctx.h2d(p, np.full(b.words[p] + N_GUARD, SENT, np.uint32))
    ctx.dev_match_descriptors(d_q, d_qc, len(q_sets), stride_q, d_t, d_tc, len(t_sets), stride_t, pairs, d_m, d_pc, *setting)
    got = b.get(d_m, "the matches").view(np.int32).reshape(len(pairs), stride_q, 4)
    acc = b.get(d_pc, "the pair counts").view(np.int32)
    for p, (fq, ft) in enumerate(pairs):
        want, n = want_match((name, fq, ft), q_sets[fq], t_sets[ft], setting)
        k = len(want)
        bad = np.flatnonzero((got[p, :k] != want).any(1))
        assert bad.size == 0, f"{name} {setting}: pair {p} ({fq}, {ft}): {bad.size} matches differ, first query {bad[0]}: " \
                              f"{got[p, bad[0]].tolist()} != {want[bad[0]].tolist()}"
        assert (got[p, k:].view(np.uint32) == SENT).all(), f"{name}: pair {p}: slots past the query count were written"
        assert acc[p] == n, f"{name} {setting}: pair {p}: {acc[p]} accepted, the rule {n}"
    return got.tobytes() + acc.tobytes(), bufs


def test_pairs_over_four_frames_with_an_empty_and_a_single_set(hip):
    rng = np.random.default_rng(41)
    every = dr.random_set(rng, 366)
    sets = [every[:0], every[:1], every[1:66], every[66:366]]
    pairs = [(1, 2), (2, 3), (3, 0), (0, 3), (3, 2), (2, 1)]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        bufs = None
        for s in SETTINGS:
            _, bufs = run_and_check(ctx, b, "four", sets, 300, sets, 300, pairs, s, bufs=bufs)
        b.free()


def test_a_set_against_itself(hip):
    rng = np.random.default_rng(42)
    sets = [dr.random_set(rng, 300), dr.random_set(rng, 65), dr.random_set(rng, 1)]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        out, bufs = run_and_check(ctx, b, "self", sets, 300, sets, 300, [(0, 0), (1, 1), (2, 2), (0, 1)], (64, 205, 1), same=True)
        got = np.frombuffer(out[:4 * 300 * 16], np.int32).reshape(4, 300, 4)
        for p, k in ((0, 300), (1, 65), (2, 1)):
            assert (got[p, :k, 1] == 0).all() and got[p, :k, 0].tolist() == list(range(k)), "every query finds itself"
            assert (got[p, :k, 3] & 4).all()
        assert (got[2, 0, 2] == 257) and (got[0, :300, 2] > 0).all()
        b.free()


def test_query_blocks_and_train_tiles_one_before_on_and_past_their_ends(hip):
    rng = np.random.default_rng(43)
    every = dr.random_set(rng, 257 + 1025, spread=40)
    q_sets = [every[:255], every[:256], every[:257]]
    t_sets = [every[257:257 + 1023].copy(), every[257:257 + 1024].copy(), every[257:257 + 1025].copy()]
    # the best neighbour of the last queries sits in the last train slots: one before, on and past the tile's end
    for t in t_sets:
        t[-1] = every[250]
        t[-1, 0] ^= np.uint64(1)
        t[-2] = every[254]
    pairs = [(a, c) for a in range(3) for c in range(3)]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        out, bufs = run_and_check(ctx, b, "ends", q_sets, 257, t_sets, 1025, pairs, (64, 205, 1))
        got = np.frombuffer(out[:9 * 257 * 16], np.int32).reshape(9, 257, 4)
        assert got[8, 254, :2].tolist() == [1023, 0] and got[8, 250, :2].tolist() == [1024, 1]
        run_and_check(ctx, b, "ends", q_sets, 257, t_sets, 1025, pairs, (256, 0, 0), bufs=bufs)
        b.free()


def test_duplicated_descriptors_go_to_the_smaller_index(hip):
    q, t = dr.duplicated_sets(np.random.default_rng(21))
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        bufs = None
        for s in SETTINGS + [(256, 205, 1)]:
            out, bufs = run_and_check(ctx, b, "dup", [q, t], 47, [t, q], 47, [(0, 0), (1, 1), (0, 1)], s, bufs=bufs)
        got = np.frombuffer(out[:3 * 47 * 16], np.int32).reshape(3, 47, 4)
        assert (got[0, :20, 1] == 0).all() and (got[0, :20, 2] == 0).all() and got[0, :20, 0].tolist() == list(range(5, 15)) * 2
        assert (got[0, :10, 3] & 4).all() and not (got[0, 10:20, 3] & 4).any()
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """The dirty-workspace discipline of DESIGN.md section 20: no call may read what an earlier call left.  The context
    first runs the point lists, the chamfer matching and a match call of another shape."""
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    rng = np.random.default_rng(44)
    big = [dr.random_set(rng, 700), dr.random_set(rng, 650)]
    sets = [dr.random_set(rng, k) for k in (0, 1, 65, 300)]
    pairs = [(1, 2), (2, 3), (3, 0), (3, 3)]
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        cset = ctx.chamfer_set_create([np.array([[0, 0], [3, 1], [-2, 4]], np.int16)])
        ctx.canny_chamfer(other, SIGMA, LO, HI, cset, 160, 24, min_dist=4, matches_max=64)
        b = _Bufs(ctx)
        run_and_check(ctx, b, "dirty big", big, 700, big, 700, [(0, 1), (1, 0), (1, 1), (0, 0), (0, 1)], (256, 0, 1))
        runs, bufs = [], None
        for _ in range(3):
            out, bufs = run_and_check(ctx, b, "dirty", sets, 300, sets, 300, pairs, (64, 205, 1), bufs=bufs)
            runs.append(out)
        assert runs[0] == runs[1] == runs[2]
        b.free()


def test_the_match_launches_take_a_second_trip(hip):
    """One workgroup per (pair, block of 256), 2048 workgroups at most: 2049 pairs of one block each, and 1025 pairs of two
    blocks, are past the cap -- for the match and, with the roles swapped, the reverse launch."""
    assert capi.descriptors_plan("match", 2048, 256).trips == 1
    plan = capi.descriptors_plan("match", 2049, 256)
    assert (plan.units, plan.grid, plan.per_group, plan.trips) == (2049, 2048, 1, 2)
    assert capi.descriptors_plan("match", 1025, 300).trips == 2 and capi.descriptors_plan("match", 1025, 12).trips == 1
    rng = np.random.default_rng(45)
    small = [dr.random_set(rng, k, 10) for k in (12, 0, 7, 1, 9, 12, 3, 5)]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        pairs = [(p % 8, (p * 3 + p // 8) % 8) for p in range(2049)]
        run_and_check(ctx, b, "cap", small, 12, small, 12, pairs, (80, 230, 1))
        # two blocks a pair on the query side, one on the train side, and the other way round
        wide = [dr.random_set(rng, k, 10) for k in (300, 257, 2)]
        pairs = [(p % 3, p % 8) for p in range(1025)]
        run_and_check(ctx, b, "cap wide", wide, 300, small, 12, pairs, (80, 230, 1))
        run_and_check(ctx, b, "cap narrow", small, 12, wide, 300, [(t, q) for q, t in pairs], (80, 230, 1))
        b.free()


def test_the_refused_match_calls(hip):
    rng = np.random.default_rng(46)
    sets = [dr.random_set(rng, 5), dr.random_set(rng, 8)]
    words, counts = pack_sets(sets, 8)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_w, d_c = b.upload(words), b.upload(counts)
        d_m, d_pc = b.filled(3 * 8 * 4), b.filled(3)
        good = dict(q=d_w, qc=d_c, nq=2, sq=8, t=d_w, tc=d_c, nt=2, st=8, pairs=[(0, 1), (1, 0), (1, 1)], m=d_m, pc=d_pc,
                    md=64, ratio=205, opt=1)

        def status(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_match_descriptors(a["q"], a["qc"], a["nq"], a["sq"], a["t"], a["tc"], a["nt"], a["st"], a["pairs"],
                                          a["m"], a["pc"], a["md"], a["ratio"], a["opt"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(q=0), dict(qc=0), dict(t=0), dict(tc=0), dict(m=0), dict(pc=0), dict(nq=0), dict(nt=0), dict(sq=0),
                   dict(st=0), dict(pairs=[]), dict(md=-1), dict(md=257), dict(ratio=-1), dict(ratio=257), dict(opt=2),
                   dict(opt=-1), dict(q=d_w + 4), dict(t=d_w + 4), dict(pairs=[(0, 1), (2, 0)]), dict(pairs=[(0, 2)]),
                   dict(pairs=[(-1, 0)]), dict(pairs=[(0, -1)]), dict(nq=1), dict(nt=1)):
            assert status(**kw) == 1, kw
        for kw in (dict(sq=4097), dict(st=4097), dict(nq=65536), dict(nt=65536)):
            assert status(**kw) == 2, kw
        b.untouched()
        assert status() == 0
        b.free()


# ---- host buffers, the CLI ---------------------------------------------------------------------------------------------------
def test_the_host_buffer_form(hip):
    h, w = 70, 77
    frames, _, planes = reference(h, w)
    want = [r for r, _, _, _ in reference_corners(h, w, 40)]
    with hip.Context(0) as ctx:
        for steered in (False, True):
            got = ctx.canny_corner_descriptors(frames, SIGMA, LO, HI, *CORNER_ARGS, corners_max=40, steered=steered)
            for f in range(3):
                rec, desc, meta = got[f]
                assert np.array_equal(rec.view(np.int64).reshape(-1, 4), want[f]), f"frame {f}"
                d, m = dr.describe(planes[f], want[f][:, :2], steered)
                assert np.array_equal(desc, d) and np.array_equal(meta, m), f"frame {f}"
        one = ctx.canny_corner_descriptors(frames[0], SIGMA, LO, HI, corners_max=1)
        assert len(one) == 1 and len(one[0][0]) == 1 and one[0][1].shape == (1, 4)


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.mark.parametrize("word", ["upright", "steered"])
def test_main_j_writes_the_descriptors_of_the_rule(tmp_path, word):
    frames, _, planes = reference(70, 128)
    _write_pgm(tmp_path / "frame.pgm", frames[0])
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, str(SIGMA), str(LO), str(HI), "-i", str(tmp_path / "frame.pgm"), "-o", str(tmp_path), "-q",
                        "2000,6,40,5", "-j", word], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = reference_corners(70, 128, 40)[0][0]
    assert len(want) >= 3
    desc, meta = dr.describe(planes[0], want[:, :2], word == "steered")
    lines = (tmp_path / "canny_descriptors.txt").read_text().splitlines()
    assert lines == [f"{x} {y} {m & 255} {m >> 8} " + "".join(f"{int(v):016x}" for v in d)
                     for (x, y, _, _), d, m in zip(want.tolist(), desc, meta.tolist())]
    assert (tmp_path / "canny_corners.txt").read_text().splitlines() == [f"0 {x} {y} {v} {rank}" for x, y, v, rank in want.tolist()]
