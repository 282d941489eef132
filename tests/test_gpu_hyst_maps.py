"""The stage hysteresis kernels on designed maps and batches (tests/hyst_maps.py), exact and over complete outputs.

What the maps are and why each link of load_tile / process_tile_with carries its frame alone is shown on the CPU in
tests/test_hyst_maps.py.  Here the same batches go through
  dev_hysteresis        one call per atlas with n_frames = the atlas size, forwards and in reversed frame order, with the
                        rows finalize kernel and with the 8-row patch one (tune_finalize_mode, process-wide: restored);
  hysteresis()          the host entry, frame by frame;
  find_edge_pixels()    from the seed, from the seed with the link pixel already visited, and from the far end,
and every result is compared with the oracle's, frame by frame.  The device buffer of a dev_hysteresis call is followed
by a guard of sentinel words that must survive the call; the call itself overwrites every pixel of its input.

Reported sweeps.  last_hysteresis_iterations is hf[0] + 1 (lane_wait), hf[0] being the largest iter + 1 of a sweep that
scheduled a tile: "the last sweep that scheduled a tile, plus two" (test_gpu_hyst_push_path.py), and 1 if none did.  The
device is never slower than the synchronous model, so the report is at most the model's sweep count plus one -- and
exactly 1 where the model schedules nothing: then no tile's changed border faces a neighbour, every tile reads the halo
it would have read in the model, and a report above 1 means that a tile was scheduled which has no business running
(a push across a frame boundary or round the end of a tile row changes no map: the tile it wakes pulls nothing).
The zigzag's lower bound comes from the map alone (hyst_maps.reported_iterations_floor).
"""
import numpy as np
import pytest

import hyst_maps as hm
import oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
GUARD = 256   # int16 words behind the frames


@pytest.fixture(scope="module")
def ctx(hip):
    with hip.Context(0) as c:
        yield c


class _Atlas:
    def __init__(self, cand, lo=hm.LO, hi=hm.HI, metas=None, empty=()):
        self.cand, self.lo, self.hi, self.metas, self.empty = cand, lo, hi, metas, empty
        self.want = np.stack([oracle.hysteresis(f, lo, hi) for f in cand])
        self.sweeps = hm.model_sweeps(cand, lo, hi)[1]
        for a in (self.cand, self.want):
            a.flags.writeable = False


_memo = {}


def _atlases():
    """name -> _Atlas with the oracle's maps and the model's sweep count; computed once and left unchanged."""
    if not _memo:
        for shape in hm.LINK_SHAPES:
            batch, metas = hm.link_atlas(shape)
            _memo[f"link{shape[0]}x{shape[1]}"] = _Atlas(batch, metas=metas)
        for shape in hm.QUIRK_SHAPES:
            batch, metas = hm.quirk_atlas(shape)
            _memo[f"quirk{shape[0]}x{shape[1]}"] = _Atlas(batch, metas=metas)
        for shape in hm.ISOLATION_SHAPES:
            for name, (batch, empty) in hm.isolation_atlas(shape).items():
                _memo[f"isolation_{name}{shape[0]}x{shape[1]}"] = _Atlas(batch, empty=empty)
        _memo["in_tile"] = _Atlas(hm.in_tile_atlas()[0])
        _memo["zigzag"] = _Atlas(hm.zigzag())
        _memo["rows"] = _Atlas(hm.row_atlas())
        _memo["row_gaps"] = _Atlas(hm.row_gap_atlas())
        _memo["rows_wide"] = _Atlas(hm.row_wide_atlas())
    return _memo


ATLAS_NAMES = ([f"link{h}x{w}" for h, w in hm.LINK_SHAPES] + [f"quirk{h}x{w}" for h, w in hm.QUIRK_SHAPES]
               + [f"isolation_{n}{h}x{w}" for h, w in hm.ISOLATION_SHAPES
                  for n in ("last_to_first", "first_to_last", "changing_row", "row_end")]
               + ["in_tile", "zigzag", "rows", "row_gaps", "rows_wide"])


def _dev(ctx, cand, lo, hi):
    """dev_hysteresis on a batch -> (status, planes, last_hysteresis_iterations).  The guard behind the frames must
    come back untouched."""
    from canny_edge_amd.capi import CannyHipError
    n, h, w = cand.shape
    buf = np.concatenate([np.ascontiguousarray(cand, np.int16).ravel(), np.full(GUARD, SENTINEL, np.int16)])
    d = ctx.malloc(buf.nbytes)
    try:
        ctx.h2d(d, buf)
        status = 0
        try:
            ctx.dev_hysteresis(d, h, w, n, lo, hi)
        except CannyHipError as e:
            status = e.status
        ctx.synchronize()
        iters = ctx.last_hysteresis_iterations
        out = np.empty_like(buf)
        ctx.d2h(out, d)
    finally:
        ctx.free(d)
    assert (out[n * h * w:] == SENTINEL).all(), "dev_hysteresis wrote behind its frames"
    return status, out[:n * h * w].reshape(n, h, w), iters


def _same(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=tuple(range(1, got.ndim))))
    if bad.size:
        f = int(bad[0])
        ys, xs = np.nonzero(got[f] != want[f])
        raise AssertionError(f"{what}: {bad.size} of {len(got)} frames differ from the oracle, first frame {f} in "
                             f"{ys.size} pixels, first ({ys[0]}, {xs[0]}): got {got[f][ys[0], xs[0]]}, "
                             f"want {want[f][ys[0], xs[0]]}")


@pytest.mark.parametrize("finalize_mode", (0, 1))
@pytest.mark.parametrize("name", ATLAS_NAMES)
def test_dev_hysteresis_on_whole_atlases(ctx, name, finalize_mode):
    a = _atlases()[name]
    ctx.set_option("tune_finalize_mode", finalize_mode)
    try:
        for order in (slice(None), slice(None, None, -1)):
            what = f"{name}, finalize mode {finalize_mode}, {'reversed' if order.step else 'forward'}"
            status, got, iters = _dev(ctx, a.cand[order], a.lo, a.hi)
            assert status == 0, what
            _same(got, a.want[order], what)
            for i in a.empty:
                assert not got[::order.step or 1][i].any(), f"{what}: frame {i} must come back empty"
            print(f"{what}: {len(got)} frames, last_hysteresis_iterations {iters}, model sweeps {a.sweeps}")
            assert 1 <= iters <= a.sweeps + 1, f"{what}: {iters} sweeps reported, model {a.sweeps}"
            if a.sweeps == 1:
                assert iters == 1, f"{what}: a tile was scheduled where no changed border faces a neighbour"
    finally:
        ctx.set_option("tune_finalize_mode", 0)


def test_zigzag_runs_more_than_one_chunk_of_sweeps(ctx):
    a = _atlases()["zigzag"]
    floor = hm.reported_iterations_floor(a.cand)
    assert floor >= 12
    status, got, iters = _dev(ctx, a.cand, a.lo, a.hi)
    assert status == 0
    _same(got, a.want, "zigzag")
    print(f"zigzag: last_hysteresis_iterations {iters}, floor from the map {floor}, model sweeps {a.sweeps}")
    assert floor <= iters <= a.sweeps + 1
    assert np.array_equal(ctx.hysteresis(a.cand[0], a.lo, a.hi), a.want[0])
    assert floor <= ctx.last_hysteresis_iterations <= a.sweeps + 1


@pytest.mark.parametrize("name", [n for n in ATLAS_NAMES if n.startswith(("link", "quirk", "in_tile"))] + ["rows"])
def test_host_hysteresis_frame_by_frame(ctx, name):
    a = _atlases()[name]
    pick = np.arange(len(a.cand))
    if name == "rows":   # a 200-frame sample, the first and the last frame among them
        pick = np.unique(np.linspace(0, len(a.cand) - 1, 200).astype(int))
    got = np.stack([ctx.hysteresis(a.cand[i], a.lo, a.hi) for i in pick])
    _same(got, a.want[pick], f"hysteresis() on {name}")


@pytest.mark.parametrize("variant", ("from_seed", "link_visited", "from_far_end"))
@pytest.mark.parametrize("name", [n for n in ATLAS_NAMES if n.startswith(("link", "quirk"))])
def test_find_edge_pixels(ctx, name, variant):
    a = _atlases()[name]
    h, w = a.cand.shape[1:]
    got_c, got_v, want_c, want_v = [], [], [], []
    for frame, m in zip(a.cand, a.metas):
        visited = np.zeros((h, w), np.uint8)
        start = m["far"][-1] if variant == "from_far_end" else m["seed"]
        if variant == "link_visited":
            visited[m["link"]] = 1
        start = start[0] * w + start[1]
        c, v = ctx.find_edge_pixels(frame, visited, start, a.lo, a.hi)
        wc, wv = oracle.find_edge_pixels(frame, visited, start, a.lo, a.hi)
        if variant == "link_visited":   # the crossing is blocked: nothing behind it is reached
            assert all(wc[p] == frame[p] and wv[p] == 0 for p in m["far"]), m["name"]
        got_c.append(c), got_v.append(v), want_c.append(wc), want_v.append(wv)
    _same(np.stack(got_c), np.stack(want_c), f"find_edge_pixels {variant} on {name}: cand")
    _same(np.stack(got_v), np.stack(want_v), f"find_edge_pixels {variant} on {name}: visited")


@pytest.mark.parametrize("finalize_mode", (0, 1))
@pytest.mark.parametrize("lo,hi", hm.VALUE_PAIRS)
def test_value_atlas(ctx, lo, hi, finalize_mode):
    """Candidates and thresholds outside the byte range: the packed saturating-subtract classify and its fallback
    (8 x 64, 24 x 64), the generic classify (8 x 61, 23 x 61), the domain flag and edge_value = 0 for hi > 255."""
    ctx.set_option("tune_finalize_mode", finalize_mode)
    try:
        for width in hm.VALUE_WIDTHS:
            batches = {"designed": hm.value_frames(lo, hi, width),
                       "random": hm.value_random(lo, hi, (24 if width == 64 else 23, width))}
            if lo <= 0:
                batches["in domain"], batches["last pixel below lo"] = hm.value_in_domain(lo, hi, width)
            for kind, cand in batches.items():
                what = f"thresholds ({lo}, {hi}), width {width}, {kind}"
                want_status = hm.value_status(cand, lo, hi)
                status, got, _ = _dev(ctx, cand, lo, hi)
                assert status == want_status, f"{what}: status {status}, expected {want_status}"
                if want_status == 0:
                    _same(got, np.stack([oracle.hysteresis(f, lo, hi) for f in cand]), what)
    finally:
        ctx.set_option("tune_finalize_mode", 0)
