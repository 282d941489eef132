"""Frame-to-frame motion from the corner matches on the GPU (canny_hip_dev_estimate_motion, canny_hip_canny_motion; DESIGN.md
section 31) against tests/motion_rule.py, word for word.  The inputs are synthetic records and match rows uploaded as they
are (images only in the last test); every output buffer is sentinel-filled with guard words behind it."""
import numpy as np
import pytest

import corners_rule as cr
import descriptors_rule as dr
import motion_rule as mr
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
N_GUARD = 64
SIGMA, LO, HI = 1.4, 50, 150
W = mr.WORDS


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

    def refill(self, p):
        self.ctx.h2d(p, np.full(self.words[p] + N_GUARD, SENT, np.uint32))

    def get(self, p, what=""):
        out = np.empty(self.words[p] + N_GUARD, np.uint32)
        self.ctx.d2h(out, p)
        assert (out[self.words[p]:] == SENT).all(), f"guard words overwritten behind {what}"
        return out[:self.words[p]]

    def untouched(self):
        for p in self.words:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def pack_records(sets, stride):
    """int64 [frames, stride, 4] (unused slots: coordinates that would be correspondences) and int32 counts."""
    rec = np.full((len(sets), stride, 4), 77, np.int64)
    counts = np.zeros(len(sets), np.int32)
    for f, s in enumerate(sets):
        rec[f, :len(s)] = s
        counts[f] = len(s)
    return rec, counts


def pack_matches(rows, stride):
    """int32 [pairs, stride, 4]; the slots past a row's length look like accepted matches to slot 0."""
    mt = np.zeros((len(rows), stride, 4), np.int32)
    mt[:, :, 3] = 15
    for p, r in enumerate(rows):
        mt[p, :len(r)] = r
    return mt


_WANT = {}


def want_of(key, *args):
    if key not in _WANT:
        _WANT[key] = mr.estimate(*args)
    return _WANT[key]


def run_and_check(ctx, b, name, q_sets, stride_q, t_sets, stride_t, pairs, rows, setting, same=False, inlier=True,
                  bufs=None, keys=None):
    """One motion call on uploaded records and match rows against the rule, pair by pair.  setting: (model, thr_q4,
    hypotheses, seed).  Returns the outputs' bytes."""
    if bufs is None:
        qr, qc = pack_records(q_sets, stride_q)
        d_q, d_qc = b.upload(qr), b.upload(qc)
        if same:
            d_t, d_tc = d_q, d_qc
        else:
            tr, tc = pack_records(t_sets, stride_t)
            d_t, d_tc = b.upload(tr), b.upload(tc)
        bufs = (d_q, d_qc, d_t, d_tc, b.upload(pack_matches(rows, stride_q)), b.filled(len(pairs) * W * 2),
                b.filled(len(pairs) * stride_q))
    d_q, d_qc, d_t, d_tc, d_m, d_motion, d_in = bufs
    b.refill(d_motion)
    b.refill(d_in)
    model, thr, hyp, seed = setting
    ctx.dev_estimate_motion(d_q, d_qc, len(q_sets), stride_q, d_t, d_tc, len(t_sets), stride_t, pairs, d_m, d_motion,
                            d_in if inlier else 0, model, thr, hyp, seed)
    got = b.get(d_motion, "the records").view(np.int64).reshape(len(pairs), W)
    flags = b.get(d_in, "the inlier flags").view(np.int32).reshape(len(pairs), stride_q)
    if not inlier:
        assert (flags.view(np.uint32) == SENT).all(), f"{name}: flags written without a buffer"
    for p, (fq, ft) in enumerate(pairs):
        key = (name, keys[p] if keys else p, setting)
        want, wf = want_of(key, q_sets[fq], len(q_sets[fq]), t_sets[ft], len(t_sets[ft]), rows[p], *setting)
        assert got[p].tolist() == want.tolist(), f"{name} {setting}: pair {p} ({fq}, {ft}): {got[p].tolist()} != {want.tolist()}"
        if inlier:
            k = len(wf)
            bad = np.flatnonzero(flags[p, :k] != wf)
            assert bad.size == 0, f"{name} {setting}: pair {p}: {bad.size} flags differ, first slot {bad[0]}"
            assert (flags[p, k:].view(np.uint32) == SENT).all(), f"{name}: pair {p}: slots past the query count were written"
    return got.tobytes() + flags.tobytes(), bufs


def random_rows(rng, n_q, n_t, accepted=0.8):
    """A match row with train indices also one outside either end of the set and a mix of flag words."""
    row = np.zeros((n_q, 4), np.int32)
    row[:, 0] = rng.integers(-1, n_t + 2, n_q)
    row[:, 3] = np.where(rng.random(n_q) < accepted, 15, rng.choice([0, 7, 3], n_q))
    return row


def four_frames(rng):
    """An empty frame, a single corner, 65 and 300 corners; frame 2 is frame 3's first 65 points turned by a quarter
    about (300, 300), 20 of them replaced."""
    pts = rng.permutation(600 * 600)[:300]
    f3 = np.zeros((300, 4), np.int64)
    f3[:, 0], f3[:, 1] = pts % 600, pts // 600
    f2 = np.zeros((65, 4), np.int64)
    f2[:, 0], f2[:, 1] = 600 - f3[:65, 1], f3[:65, 0]
    f2[rng.permutation(65)[:20], :2] = rng.integers(0, 600, (20, 2))
    return [f3[:0], f3[7:8], f2, f3]


ALL_MODELS = [(0, 48, 40, 3), (1, 48, 40, 3), (2, 48, 40, 3)]


def test_pairs_over_four_frames_with_an_empty_and_a_single_set(hip):
    rng = np.random.default_rng(51)
    sets = four_frames(rng)
    pairs = [(2, 3), (3, 2), (1, 2), (2, 1), (3, 0), (0, 3), (1, 1), (3, 3)]
    rows = [random_rows(rng, len(sets[q]), len(sets[t])) for q, t in pairs]
    rows[0][:, 0], rows[0][:, 3] = np.arange(65), 15          # the turned points against their originals
    rows[6][:, 0], rows[6][:, 3] = 0, 15                      # m = 1
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        bufs = None
        for s in ALL_MODELS:
            out, bufs = run_and_check(ctx, b, "four", sets, 300, sets, 300, pairs, rows, s, bufs=bufs)
            got = np.frombuffer(out[:len(pairs) * W * 8], np.int64).reshape(-1, W)
            assert got[0, 0] == 3 and (got[0, 2] >= 45 or s[0] == 0), "the quarter turn is found"
            assert got[4, :4].tolist() == [0, 0, 0, -1] and got[5, :4].tolist() == [0, 0, 0, -1]
            assert got[6, 1] == 1 and got[6, 0] == (3 if s[0] == 0 else 0)
        b.free()


_EDGES = {}


def edge_sets():
    """Correspondence lists of 63 / 64 / 65 / 255 / 256 / 257 entries with as many slots in between that are none: m and the
    slots cross the wave and block edges of the gather and of the staging loop."""
    if not _EDGES:
        rng = np.random.default_rng(52)
        q_sets, t_sets, rows = [], [], []
        for m in (63, 64, 65, 255, 256, 257):
            qc, tc, mt = mr.designed(rng, m, (0, -1, 1, 0, 640, 3), m // 3)
            c = np.concatenate([qc[:, :2], tc[mt[:, 0], :2]], 1)
            qg, tg, mg = mr.with_gaps(rng, c, m)
            q_sets.append(qg), t_sets.append(tg), rows.append(mg)
        _EDGES["v"] = (q_sets, t_sets, rows)
    return _EDGES["v"]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_m_one_before_on_and_past_the_wave_and_block_edges(hip, model):
    q_sets, t_sets, rows = edge_sets()
    pairs = [(f, f) for f in range(6)]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        out, _ = run_and_check(ctx, b, "edges", q_sets, 514, t_sets, 514, pairs, rows, (model, 32, 24, 9))
        got = np.frombuffer(out[:6 * W * 8], np.int64).reshape(-1, W)
        assert got[:, 1].tolist() == [63, 64, 65, 255, 256, 257]
        b.free()


_WIDE = {}


def widest_set():
    """m = 4096 with coordinates spread to 0 and 65535: half follow the half turn about the centre (M = -I), the others
    are random; the first entries pin the extreme differences."""
    if not _WIDE:
        rng = np.random.default_rng(53)
        c = np.zeros((4096, 4), np.int64)
        c[:, :2] = rng.integers(0, 65536, (4096, 2))
        c[:, 2:] = 65535 - c[:, :2]
        c[::2, 2:] = rng.integers(0, 65536, (2048, 2))
        c[:8] = [(0, 0, 65535, 65535), (65535, 65535, 0, 0), (0, 65535, 65535, 0), (65535, 0, 0, 65535),
                 (0, 0, 0, 65535), (65535, 65535, 65535, 0), (0, 65535, 0, 0), (65535, 0, 65535, 65535)]
        _WIDE["v"] = (mr.from_correspondences(c), mr.from_correspondences(c[:8]))
    return _WIDE["v"]


@pytest.mark.parametrize("model,thr", [(0, 4095), (1, 4095), (2, 4095), (1, 16)])
def test_4096_correspondences_with_extreme_coordinates(hip, model, thr):
    (qc, tc, mt), (qc8, tc8, mt8) = widest_set()      # the second pair: the eight extreme entries alone
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        out, _ = run_and_check(ctx, b, "wide", [qc, qc8], 4096, [tc, tc8], 4096, [(0, 0), (1, 1)], [mt, mt8],
                               (model, thr, 64, 5))
        got = np.frombuffer(out[:2 * W * 8], np.int64).reshape(2, W)
        assert got[0, 1] == 4096 and got[0, 0] & 1 and got[1, 1] == 8 and got[1, 0] & 1
        b.free()


@pytest.mark.parametrize("hypotheses", [1, 63, 64, 65, 257, 4096])
def test_hypotheses_one_before_on_and_past_the_score_blocks(hip, hypotheses):
    rng = np.random.default_rng(54)
    qc, tc, mt = mr.designed(rng, 36, (2, 0, 0, 2, 11, 5), 14)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        bufs = None
        for model in (0, 1, 2):
            _, bufs = run_and_check(ctx, b, "blocks", [qc], 36, [tc], 36, [(0, 0)], [mt], (model, 48, hypotheses, 12),
                                    bufs=bufs)
        b.free()


def tie_seed():
    """A seed whose hypothesis 0 draws a stray of tie_set (count 1) and whose later ones draw from both groups."""
    for seed in range(1000):
        first = [mr.sample(h, seed, 10, 1)[0] for h in range(8)]
        groups = [0 if i < 4 else 1 if i < 8 else 2 for i in first]
        if groups[0] == 2 and 0 in groups and 1 in groups:
            return seed, next(h for h, g in enumerate(groups) if g != 2)
    raise AssertionError("no such seed")


def threshold_seed(model):
    """A seed whose hypothesis 0 is drawn from the exact correspondences of threshold_set (neighbours under SIMILARITY)."""
    for seed in range(10000):
        idx = mr.sample(0, seed, 8, model + 1)
        if max(idx) < 6 and (model == 0 or abs(idx[0] - idx[1]) == 1):
            return seed
    raise AssertionError("no such seed")


def test_ties_go_to_the_smaller_h_and_the_threshold_is_inclusive(hip):
    seed, h_first = tie_seed()
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        qc, tc, mt = mr.from_correspondences(mr.tie_set())
        out, _ = run_and_check(ctx, b, "tie", [qc], 10, [tc], 10, [(0, 0)], [mt], (0, 16, 8, seed))
        got = np.frombuffer(out[:W * 8], np.int64)
        assert got[2] == 4 and got[3] == h_first and h_first > 0
        for model in (0, 1):
            qc, tc, mt = mr.from_correspondences(mr.threshold_set(model))
            out, _ = run_and_check(ctx, b, f"thr{model}", [qc], 8, [tc], 8, [(0, 0)], [mt], (model, 48, 1, threshold_seed(model)))
            got = np.frombuffer(out[:W * 8], np.int64)
            flags = np.frombuffer(out[W * 8:W * 8 + 32], np.int32)
            assert flags.tolist() == [1] * 7 + [0] and got[2] == 7 and got[15] == (1 if model == 0 else 25)
        b.free()


def test_the_same_buffers_as_query_and_train_side(hip):
    rng = np.random.default_rng(55)
    sets = four_frames(rng)[1:]
    pairs = [(2, 2), (1, 1), (0, 0), (1, 2), (2, 1)]
    rows = [random_rows(rng, len(sets[q]), len(sets[t])) for q, t in pairs]
    rows[0][:, 0], rows[0][:, 3] = np.arange(300), 15
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for s in ALL_MODELS:
            out, _ = run_and_check(ctx, b, "self", sets, 300, sets, 300, pairs, rows, s, same=True)
            got = np.frombuffer(out[:W * 8], np.int64)
            assert got[:3].tolist() == [3, 300, 300] and got[4:12].tolist() == [65536, 0, 0, 0, 65536, 0, 0, 0]
        b.free()


def test_without_the_inlier_buffer(hip):
    rng = np.random.default_rng(56)
    sets = four_frames(rng)
    pairs = [(2, 3), (3, 2), (0, 1)]
    rows = [random_rows(rng, len(sets[q]), len(sets[t])) for q, t in pairs]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        a, bufs = run_and_check(ctx, b, "null", sets, 300, sets, 300, pairs, rows, (1, 48, 70, 2))
        c, _ = run_and_check(ctx, b, "null", sets, 300, sets, 300, pairs, rows, (1, 48, 70, 2), inlier=False, bufs=bufs)
        assert a[:3 * W * 8] == c[:3 * W * 8]
        b.free()


def test_three_identical_runs_on_a_dirty_context(hip):
    """The dirty-workspace discipline of DESIGN.md section 20: no call may read what an earlier call left.  The context
    first runs the point lists and a motion call of another shape whose workspace is then filled with a sentinel."""
    other = np.stack([synth_frame(90, 200, s) for s in (7, 8, 9)])
    rng = np.random.default_rng(57)
    sets = four_frames(rng)
    pairs = [(2, 3), (3, 2), (1, 2), (3, 0), (3, 3)]
    rows = [random_rows(rng, len(sets[q]), len(sets[t])) for q, t in pairs]
    q_sets, t_sets, edge_rows = edge_sets()
    with hip.Context(0) as ctx:
        ctx.canny_points(other, SIGMA, LO, HI)
        b = _Bufs(ctx)
        run_and_check(ctx, b, "edges", q_sets, 514, t_sets, 514, [(f, f) for f in range(6)], edge_rows, (2, 32, 24, 9))
        runs, bufs = [], None
        for _ in range(3):
            (ptr, nbytes), = [(p, size) for name, p, size, _ in ctx.selftest_workspaces() if name == "motion_ws"]
            assert nbytes >= 6 * 514 * 12
            ctx.h2d(ptr, np.full(nbytes // 4, SENT, np.uint32))
            out, bufs = run_and_check(ctx, b, "dirty", sets, 300, sets, 300, pairs, rows, (2, 40, 300, 1), bufs=bufs)
            runs.append(out)
        assert runs[0] == runs[1] == runs[2]
        b.free()


def test_the_score_and_refit_launches_take_a_second_trip(hip):
    """One workgroup per pair (gather, refit) and per (pair, block of 256 hypotheses) (score), 2048 workgroups at most:
    2049 pairs take workgroup 0 of each launch through a second trip, and with 257 hypotheses the score launch through a
    third."""
    assert capi.motion_plan("refit", 2048).trips == 1 and capi.motion_plan("score", 2048, 256).trips == 1
    for which, hyp, units, trips in (("gather", 3, 2049, 2), ("refit", 3, 2049, 2), ("score", 3, 2049, 2), ("score", 257, 4098, 3)):
        plan = capi.motion_plan(which, 2049, hyp)
        assert (plan.units, plan.grid, plan.per_group, plan.trips) == (units, 2048, 1, trips)
    rng = np.random.default_rng(58)
    small = []
    for k in (12, 0, 7, 1, 9, 12, 3, 5):
        s = np.zeros((k, 4), np.int64)
        s[:, :2] = rng.integers(0, 40, (k, 2))
        small.append(s)
    by_frames = {(q, t): random_rows(rng, len(small[q]), len(small[t]), 0.9) for q in range(8) for t in range(8)}
    pairs = [(p % 8, (p * 3 + p // 8) % 8) for p in range(2049)]
    rows = [by_frames[pt] for pt in pairs]
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        bufs = None
        for s in ((2, 64, 3, 4), (1, 64, 257, 4)):
            _, bufs = run_and_check(ctx, b, "cap", small, 12, small, 12, pairs, rows, s, bufs=bufs, keys=pairs)
        b.free()


def test_the_refused_calls(hip):
    rng = np.random.default_rng(59)
    sets = four_frames(rng)[2:]
    rec, counts = pack_records(sets, 300)
    rows = pack_matches([random_rows(rng, 65, 300), random_rows(rng, 300, 65), random_rows(rng, 300, 300)], 300)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_r, d_c, d_m = b.upload(rec), b.upload(counts), b.upload(rows)
        d_motion, d_in = b.filled(3 * W * 2), b.filled(3 * 300)
        good = dict(q=d_r, qc=d_c, nq=2, sq=300, t=d_r, tc=d_c, nt=2, st=300, pairs=[(0, 1), (1, 0), (1, 1)], m=d_m,
                    motion=d_motion, inl=d_in, model=1, thr=48, hyp=16, seed=1)

        def status(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_estimate_motion(a["q"], a["qc"], a["nq"], a["sq"], a["t"], a["tc"], a["nt"], a["st"], a["pairs"],
                                        a["m"], a["motion"], a["inl"], a["model"], a["thr"], a["hyp"], a["seed"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        for kw in (dict(q=0), dict(qc=0), dict(t=0), dict(tc=0), dict(m=0), dict(motion=0), dict(nq=0), dict(nt=0),
                   dict(sq=0), dict(st=0), dict(pairs=[]), dict(model=-1), dict(model=3), dict(thr=-1), dict(thr=4096),
                   dict(hyp=0), dict(hyp=-5), dict(q=d_r + 4), dict(t=d_r + 4), dict(motion=d_motion + 4),
                   dict(pairs=[(0, 1), (2, 0)]), dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, -1)]),
                   dict(nq=1), dict(nt=1)):
            assert status(**kw) == 1, kw
        for kw in (dict(sq=4097), dict(st=4097), dict(nq=65536), dict(nt=65536), dict(hyp=4097)):
            assert status(**kw) == 2, kw
        b.untouched()
        assert status() == 0 and status(inl=0) == 0 and status(seed=0xFFFFFFFF) == 0
        b.free()


def test_canny_motion_end_to_end_on_two_views(hip):
    """Views A and B of the descriptor tests' scene (240 x 320, B shifted by (-7, -4) with noise) as a two-frame batch:
    every output against the host rules chained on the oracle's smoothed planes."""
    big = synth_frame(300, 400, 7)
    rng = np.random.default_rng(1)
    noisy = np.clip(big[14:254, 17:337].astype(np.int64) + rng.integers(-4, 5, (240, 320)), 0, 255).astype(np.uint8)
    frames = np.stack([big[10:250, 10:330], noisy])
    planes = [oracle.gaussian(f, SIGMA) for f in frames]
    corner_args = dict(quality_q16=655, min_dist=8, corners_max=256)
    want_c = [cr.corners(P, **corner_args)[0] for P in planes]
    for steered, model, pairs in ((True, 1, [(0, 1), (1, 0)]), (False, 0, [(0, 1)]), (True, 2, [(1, 1), (0, 1)])):
        desc = [dr.describe(P, c[:, :2], steered)[0] for P, c in zip(planes, want_c)]
        with hip.Context(0) as ctx:
            rec, corners, matches, flags = ctx.canny_motion(frames, SIGMA, LO, HI, pairs=pairs, steered=steered, model=model,
                                                            thr_q4=32, hypotheses=128, seed=3, details=True,
                                                            **corner_args)
            plain = ctx.canny_motion(frames, SIGMA, LO, HI, pairs=pairs, steered=steered, model=model, thr_q4=32,
                                     hypotheses=128, seed=3, **corner_args)
        assert plain.tobytes() == rec.tobytes()
        for f in range(2):
            assert np.array_equal(corners[f].view(np.int64).reshape(-1, 4), want_c[f]), f"frame {f}"
        for p, (fq, ft) in enumerate(pairs):
            want_m, _ = dr.match(desc[fq], desc[ft], 64, 205, 1)
            assert np.array_equal(matches[p], want_m), f"pair {p}: matches"
            want, wf = mr.estimate(want_c[fq], len(want_c[fq]), want_c[ft], len(want_c[ft]), want_m, model, 32, 128, 3)
            assert rec[p].tolist() == tuple(want.tolist()), f"pair {p}: {rec[p].tolist()} != {want.tolist()}"
            assert np.array_equal(flags[p], wf), f"pair {p}: flags"
        p01 = pairs.index((0, 1))
        assert rec[p01]["flags"] == 3 and rec[p01]["inliers"] >= 30
        assert abs(rec[p01]["tx"] / 65536 + 7) < 2.5 and abs(rec[p01]["ty"] / 65536 + 4) < 2.5
