"""Reconstruction on the GPU (canny_hip_dev_reconstruct_bits, canny_hip_dev_canny_reconstruct, canny_hip_reconstruct_batch;
DESIGN.md section 38) against tests/reconstruct_rule.py, byte for byte: every output byte and every word of info, with sentinel
bytes behind each buffer, info untouched when it is not asked for, and the same bytes under the stepwise route, the tile flood
and whatever automatic takes."""
import os
import subprocess

import numpy as np
import pytest

import binarize_rule
import components_rule
import oracle
import reconstruct_rule as R
import thin_rule
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_GUARD = 256
SIGMA, LO, HI = 1.4, 50, 150
ROUTES = (capi.RECON_ROUTE_STEPWISE, capi.RECON_ROUTE_TILES, capi.RECON_ROUTE_AUTO)
SHAPES = ((1, 1), (3, 5), (33, 257), (64, 512), (65, 513))


class _Bufs:
    """Device buffers of one context: sentinel-filled outputs with guard bytes behind each, and plain uploads."""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptrs = ctx, {}, []

    def filled(self, nbytes, odd=False):
        p = self.ctx.malloc(nbytes + N_GUARD + 8)
        self.ptrs.append(p)
        self.ctx.h2d(p, np.full(nbytes + N_GUARD + 8, SENT, np.uint8))
        p += 1 if odd else 0
        self.size[p] = nbytes
        return p

    def upload(self, a, odd=False):
        """odd: the data starts one byte into the allocation."""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if odd:
            a = np.concatenate([np.full(1, 0xFF, np.uint8), a])
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p + (1 if odd else 0)

    def get(self, p, what=""):
        out = np.empty(self.size[p] + N_GUARD, np.uint8)
        self.ctx.d2h(out, p)
        assert (out[self.size[p]:] == SENT).all(), f"guard bytes overwritten behind {what}"
        return out[:self.size[p]]

    def untouched(self):
        for p in self.size:
            assert (self.get(p) == SENT).all(), "a refused call wrote something"

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.size, self.ptrs = {}, []


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def check_output(b, what, d_out, d_info, shape, want, want_info, with_info):
    out = b.get(d_out, what + ": out").reshape(shape)
    info = b.get(d_info, what + ": info")
    same(out, want, what)
    if with_info:
        assert info.view(np.int64).reshape(-1, 3).tolist() == want_info.tolist(), what + ": info"
    else:
        assert (info == SENT).all(), what + ": info written without a buffer"
    return out.tobytes() + info.tobytes()


def run(ctx, b, what, d_marker, d_mask, shape, w, op, c, route, want, with_info=True, odd_out=False):
    """One call under one route, checked against `want` = (bits, info).  -> (the bytes that came back, the sweep launches)."""
    n, h, rb = shape
    d_out, d_info = b.filled(n * h * rb, odd_out), b.filled(n * 24)
    ctx.set_option("reconstruct_route", route)
    ctx.dev_reconstruct_bits(d_marker, d_mask, n, h, w, op, c, d_out, d_info if with_info else 0)
    ctx.set_option("reconstruct_route", 0)
    launches = ctx.get_option("last_reconstruct_launches")
    assert launches >= 4, "the first chunk of launches"
    return check_output(b, f"{what} op {op} c {c} route {route}", d_out, d_info, shape, want[0], want[1], with_info), launches


def every_route(ctx, b, what, marker, mask, op, c, dirty=None, odd=False, with_info=True):
    """One case under every route: the rule's bytes and info, identical among the routes.  marker, mask: bool [n, h, w];
    dirty: None for clean pad bits, else a generator for random ones (True: all set).  -> ({route: launches}, rule's info)."""
    mask = np.asarray(mask, bool)
    w = mask.shape[-1]
    pk = R.pack if dirty is None else (R.pack_dirty if dirty is True else (lambda a: R.pack_dirty(a, dirty)))
    mb = pk(mask)
    kb = None if op != R.SEEDED else pk(np.asarray(marker, bool))
    want = R.reconstruct(kb, mb, w, op, c)
    d_mask, d_marker = b.upload(mb, odd), 0 if kb is None else b.upload(kb, odd)
    runs = {r: run(ctx, b, what, d_marker, d_mask, mb.shape, w, op, c, r, want, with_info, odd) for r in ROUTES}
    assert len({r[0] for r in runs.values()}) == 1, what + ": the routes differ"
    return {r: v[1] for r, v in runs.items()}, want[1]


def random_batch(n, h, w, seed):
    """Frames that differ: densities 0.3 / 0.6 / 0.8 in turn, sparse markers."""
    rng = np.random.default_rng(seed)
    mask = np.stack([rng.random((h, w)) < (0.3, 0.6, 0.8)[(seed + f) % 3] for f in range(n)])
    return rng.random((n, h, w)) < 0.01, mask


@pytest.mark.parametrize("c", R.CONNECTIVITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_op_and_connectivity_on_random_batches_of_three(hip, shape, c):
    """Widths 512 (whole aligned words: the state lives in the output) and 1, 5, 257, 513 (it lives in the workspace copy);
    an output one byte off its allocation takes the copy as well."""
    h, w = shape
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for i, op in enumerate(R.OPS):
            seed = 10 * h + i + c
            marker, mask = random_batch(3, h, w, seed)
            every_route(ctx, b, f"3 x {h} x {w}", marker, mask, op, c, np.random.default_rng(seed) if i != 1 else None,
                        odd=(i + c // 4) % 2 == 1, with_info=(seed % 4) != 3)
            b.free()


def test_whole_word_rows_with_the_state_in_the_output(hip):
    """w = 128, 512 and 1024 (two tiles side by side): rows of whole words at aligned addresses; blobs, so that the flood has
    components to tell apart."""
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for w, h in ((128, 70), (512, 130), (1024, 65)):
            mask = np.stack([R.blobs(h, w, s, 5, 0.5) for s in range(3)])
            marker = np.random.default_rng(w).random(mask.shape) < 0.002
            for op in R.OPS:
                for c in R.CONNECTIVITIES:
                    _, info = every_route(ctx, b, f"blobs {h} x {w}", marker, mask, op, c)
                    assert 0 < info[:, 0].min() and (op == R.FILL_HOLES or (info[:, 0] < info[:, 1]).all())
                b.free()


@pytest.mark.parametrize("name", R.DESIGNED)
def test_designed_maps_as_whole_batches_forwards_and_reversed(hip, name):
    d = R.designed(name)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for mask, marker in ((d["mask"], d["marker"]), (d["mask"][::-1], None if d["marker"] is None else d["marker"][::-1])):
            # the designed frames between an empty and a full frame: a batch whose frames finish at different launches
            pad = lambda a, fill: None if a is None else np.concatenate([np.zeros_like(a[:1]), a, np.full_like(a[:1], fill)])
            for c in R.CONNECTIVITIES:
                every_route(ctx, b, name, pad(marker, False), pad(mask, True), d["op"], c, True if d["dirty"] else None)
            b.free()


def test_dirty_pad_bits_in_marker_and_mask(hip):
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for w in (1, 7, 13, 61, 65, 513):
            marker, mask = random_batch(2, 9, w, w)
            for op in R.OPS:
                every_route(ctx, b, f"dirty w {w}", marker, mask, op, 8, True)
                every_route(ctx, b, f"dirty w {w}", marker, mask, op, 4, np.random.default_rng(w), odd=True)
            b.free()


def test_the_zigzag_takes_more_than_the_first_chunk_of_launches(hip):
    """65 x 40, one component of 1319 pixels whose path crosses the border between tile rows 0..63 and row 64 twenty times.  A
    launch of the tile flood runs each tile once, so the path advances at most two crossings a launch: at least 10 launches,
    more than the first chunk of 4.  The stepwise route moves one pixel a launch within a lane's word (one word a row here);
    only where the path changes rows can a wave that runs later see the step of the same launch, once per crossing of the two
    waves' border at rows 63 / 64: at c = 4 the path has 1318 steps, so more than 1318 - 20 launches change something."""
    z = R.zigzag(65, 40)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        launches, info = every_route(ctx, b, "zigzag", R.first_pixel(z)[None], z[None], R.SEEDED, 4)
        assert info[0].tolist() == [1319, 1319, 1]
        assert launches[capi.RECON_ROUTE_TILES] >= 10
        assert launches[capi.RECON_ROUTE_STEPWISE] >= 1300
        launches, info = every_route(ctx, b, "zigzag", R.first_pixel(z)[None], z[None], R.SEEDED, 8)
        assert info[0].tolist() == [1319, 1319, 1] and launches[capi.RECON_ROUTE_TILES] >= 10
        # from the far end, in a batch with frames that finish at once, and the hole-free fill of its complement's background
        far = np.zeros_like(z)
        far[0, 38] = True
        batch = np.stack([np.zeros_like(z), z, np.ones_like(z)])
        marks = np.stack([far, far, far])
        launches, info = every_route(ctx, b, "zigzag batch", marks, batch, R.SEEDED, 4)
        assert info[:, 0].tolist() == [0, 1319, 65 * 40] and launches[capi.RECON_ROUTE_TILES] >= 10
        b.free()


def test_more_tiles_than_the_grid_cap(hip):
    """One tile per 3 x 5 frame and 4096 workgroups at most: 4097 frames send workgroup 0 through a second trip, as the plan
    query says."""
    assert hip.reconstruct_plan(4096, 3, 5, capi.RECON_ROUTE_TILES).trips == 1
    plan = hip.reconstruct_plan(4097, 3, 5, capi.RECON_ROUTE_TILES)
    assert (plan.units, plan.grid, plan.per_group) == (4097, 4096, 1) and plan.trips >= 2
    rng = np.random.default_rng(9)
    mask, marker = rng.random((4097, 3, 5)) < 0.6, rng.random((4097, 3, 5)) < 0.1
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        for op in R.OPS:
            _, info = every_route(ctx, b, "4097 frames", marker, mask, op, 4 if op == R.SEEDED else 8, np.random.default_rng(1))
            assert len(set(info[:, 0].tolist())) > 1
            b.free()


def test_dev_canny_reconstruct_behind_dev_canny(hip):
    n, h, w = 3, 70, 200
    frames = np.stack([synth_frame(h, w, 11 + s) for s in range(n)])
    rb = (w + 7) // 8
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_img, d_edges, d_bits = b.upload(frames), b.filled(n * h * w * 2), b.filled(n * h * rb)
        ctx.dev_canny_bits(d_img, SIGMA, LO, HI, h, w, n, d_bits)
        bits = b.get(d_bits, "the map").reshape(n, h, rb)
        edges = R.unpack(bits, w)
        assert edges.any()
        marker = np.zeros_like(edges)
        marker.reshape(-1)[np.flatnonzero(edges)[::97]] = True   # every 97th edge pixel
        kb = R.pack(marker)
        d_marker = b.upload(kb)
        ctx.dev_canny(d_img, SIGMA, LO, HI, h, w, n, d_edges)
        for op, c, route in ((R.FILL_HOLES, 8, 0), (R.FILL_HOLES, 4, 1), (R.SEEDED, 8, 2), (R.SEEDED, 4, 1), (R.CLEAR_BORDER, 8, 0)):
            want, want_info = R.reconstruct(kb if op == R.SEEDED else None, bits, w, op, c)
            d_out, d_info = b.filled(n * h * rb), b.filled(n * 24)
            ctx.set_option("reconstruct_route", route)
            ctx.dev_canny_reconstruct(d_marker if op == R.SEEDED else 0, n, h, w, op, c, d_out, d_info)
            check_output(b, f"canny_reconstruct op {op} c {c}", d_out, d_info, (n, h, rb), want, want_info, True)
            if op == R.SEEDED:
                assert 0 < want_info[:, 0].sum() < want_info[:, 1].sum(), "some contours hold a marker, some do not"
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_reconstruct(0, n, h + 1, w, R.FILL_HOLES, 8, d_bits)
        b.free()
    with hip.Context(0) as ctx:   # no canny call yet
        b = _Bufs(ctx)
        with pytest.raises(capi.CannyHipError):
            ctx.dev_canny_reconstruct(0, n, h, w, R.FILL_HOLES, 8, b.filled(n * h * rb))
        b.untouched()
        b.free()


def test_the_chain_on_the_device(hip):
    """u8 frame -> dev_binarize FIXED at lo and at hi -> dev_reconstruct_bits SEEDED (hysteresis thresholding of the plane) ->
    FILL_HOLES -> dev_components_bits with nothing downloaded in between, against the rules chained."""
    h, w = 96, 160
    rb = (w + 7) // 8
    frame = synth_frame(h, w, 3)[None]
    low = binarize_rule.binarize(frame, binarize_rule.FIXED, 90)[0]
    high = binarize_rule.binarize(frame, binarize_rule.FIXED, 170)[0]
    want_hyst, hyst_info = R.reconstruct(high, low, w, R.SEEDED, 8)
    want_fill, fill_info = R.reconstruct(None, want_hyst, w, R.FILL_HOLES, 8)
    assert 0 < hyst_info[0, 0] < hyst_info[0, 1]
    want_labels, want_stats, want_off = components_rule.csr(R.unpack(want_fill, w), 1)
    cap = max(len(want_stats), 1)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_frame = b.upload(frame)
        d_lo, d_hi, d_hyst, d_fill = (b.filled(h * rb) for _ in range(4))
        d_i1, d_i2 = b.filled(24), b.filled(24)
        d_labels, d_stats, d_off = b.filled(h * w * 4), b.filled(cap * 6 * 4), b.filled(2 * 8)
        ctx.dev_binarize(d_frame, 1, h, w, capi.BIN_FIXED, 90, d_lo)
        ctx.dev_binarize(d_frame, 1, h, w, capi.BIN_FIXED, 170, d_hi)
        ctx.dev_reconstruct_bits(d_hi, d_lo, 1, h, w, R.SEEDED, 8, d_hyst, d_i1)
        ctx.dev_reconstruct_bits(0, d_hyst, 1, h, w, R.FILL_HOLES, 8, d_fill, d_i2)
        ctx.dev_components_bits(d_fill, h, w, 1, 1, d_labels, 0, d_stats, cap, d_off)
        same(b.get(d_hyst, "hysteresis").reshape(1, h, rb), want_hyst, "hysteresis")
        same(b.get(d_fill, "filled").reshape(1, h, rb), want_fill, "filled")
        assert b.get(d_i1, "info").view(np.int64).tolist() == hyst_info[0].tolist()
        assert b.get(d_i2, "info").view(np.int64).tolist() == fill_info[0].tolist()
        assert b.get(d_off, "offsets").view(np.uint64).tolist() == [0, len(want_stats)]
        same(b.get(d_stats, "stats").view(np.int32).reshape(cap, 6)[:len(want_stats)], want_stats, "stats")
        b.free()


def test_reconstruct_batch_on_host_buffers(hip):
    s = thin_rule.demo_scene()
    mask = np.stack([s, np.roll(s, -10, axis=1), R.blobs(96, 160, 3)])
    marker = np.stack([R.first_pixel(m) for m in mask])
    mb, kb = R.pack_dirty(mask, np.random.default_rng(2)), R.pack_dirty(marker, np.random.default_rng(3))
    with hip.Context(0) as ctx:
        for op, c in ((R.SEEDED, 8), (R.FILL_HOLES, 8), (R.CLEAR_BORDER, 8), (R.FILL_HOLES, 4), (R.SEEDED, 4)):
            k = kb if op == R.SEEDED else None
            want, want_info = R.reconstruct(k, mb, 160, op, c)
            out, info = ctx.reconstruct_batch(k, mb, 160, op, c)
            same(out, want, f"reconstruct_batch op {op} c {c}")
            assert info.tolist() == want_info.tolist()
            if (op, c) == (R.SEEDED, 8):
                assert info[0].tolist() == [427, 1735, 1]
            if (op, c) == (R.FILL_HOLES, 8):
                assert info[0].tolist()[:2] == [3248, 1735]
            if (op, c) == (R.CLEAR_BORDER, 8):
                assert info[0, 0] == 1735 and info[1, 0] == 427, "the shifted scene loses the ring, and only it"


def test_three_identical_runs_on_a_dirty_context(hip):
    """No call may read what an earlier call left: the context first runs a larger, denser call and a thinning call that
    leaves thin_ws full, and every data workspace it holds is filled with a sentinel before each of three identical runs."""
    big_marker, big = random_batch(4, 129, 577, 1)
    n, h, w = 3, 50, 130
    marker, mask = random_batch(n, h, w, 21)
    mb, kb = R.pack_dirty(mask), R.pack_dirty(marker)
    with hip.Context(0) as ctx:
        ctx.reconstruct_batch(R.pack(big_marker), R.pack(big | True), 577, R.SEEDED, 8)
        ctx.thin_batch(R.pack(big), 577, thin_rule.GUOHALL, 0)
        b = _Bufs(ctx)
        d_mask, d_marker = b.upload(mb), b.upload(kb)
        for op, c, route in ((R.SEEDED, 8, 0), (R.FILL_HOLES, 8, 1), (R.CLEAR_BORDER, 4, 2), (R.SEEDED, 4, 1)):
            want = R.reconstruct(kb if op == R.SEEDED else None, mb, w, op, c)
            runs = []
            for _ in range(3):
                for _name, ptr, nbytes, kind in ctx.selftest_workspaces():
                    if kind == hip.WS_DATA and ptr and nbytes:
                        ctx.h2d(ptr, np.full(nbytes, SENT, np.uint8))
                runs.append(run(ctx, b, "dirty", d_marker if op == R.SEEDED else 0, d_mask, mb.shape, w, op, c, route, want)[0])
            assert runs[0] == runs[1] == runs[2]
        assert any(name == "thin_ws" and kind == hip.WS_DATA and nbytes for name, _p, nbytes, kind in ctx.selftest_workspaces())
        b.free()


def test_the_refused_calls(hip):
    n, h, w = 2, 20, 30
    rb = 4
    marker, mask = random_batch(n, h, w, 40)
    with hip.Context(0) as ctx:
        b = _Bufs(ctx)
        d_mask, d_marker = b.upload(R.pack(mask)), b.upload(R.pack(marker))
        d_out, d_info = b.filled(n * h * rb), b.filled(n * 24 + 8)
        good = dict(marker=d_marker, mask=d_mask, n=n, h=h, w=w, op=R.SEEDED, c=8, out=d_out, info=d_info)

        def call(**kw):
            a = dict(good, **kw)
            try:
                ctx.dev_reconstruct_bits(a["marker"], a["mask"], a["n"], a["h"], a["w"], a["op"], a["c"], a["out"], a["info"])
            except capi.CannyHipError as e:
                return e.status
            return 0

        # among them the four of the issue: a bad enum, a bad connectivity, a marker where none is allowed, an overlapping output
        for kw in (dict(op=3), dict(c=6), dict(op=R.FILL_HOLES), dict(out=d_mask + 8), dict(op=-1), dict(c=0), dict(marker=0),
                   dict(mask=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(op=R.CLEAR_BORDER), dict(out=d_marker),
                   dict(out=d_mask + n * h * rb - 1), dict(info=d_info + 4), dict(info=d_mask), dict(info=d_out + 8)):
            assert call(**kw) == 1, kw
        for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
            assert call(**kw) == 2, kw
        for name, value in (("reconstruct_route", 3), ("reconstruct_route", -1), ("last_reconstruct_launches", 0)):
            with pytest.raises(capi.CannyHipError):
                ctx.set_option(name, value)
        assert ctx.get_option("last_reconstruct_launches") == 0, "a fresh context, and refused calls queue nothing"
        ctx.synchronize()
        b.untouched()
        assert call() == 0 and call(info=0) == 0 and call(marker=0, op=R.FILL_HOLES, c=4) == 0
        assert ctx.get_option("last_reconstruct_launches") >= 4
        b.get(d_out), b.get(d_info)
        b.free()


def test_the_profile_parts_answer(hip):
    bits = R.pack(thin_rule.demo_scene()[None])
    with hip.Context(0) as ctx:
        ctx.profile_enable(1)
        for op in (R.FILL_HOLES, R.CLEAR_BORDER):
            ctx.reconstruct_batch(None, bits, 160, op, 8)
        for part in range(len(capi.RECON_PARTS)):
            ms, launches = ctx.profile_part("reconstruct", part)
            assert launches > 0 and ms > 0.0, capi.RECON_PARTS[part]
        with pytest.raises(capi.CannyHipError):
            ctx.profile_part("reconstruct", 2)


def test_cli_writes_the_reconstructed_map(hip, fixture_image, tmp_path):
    """Main ... [-a ...] -R: the binarized frame (with -a) or the finished edge map reconstructed into canny_reconstruct.pgm, and
    the three info words on stdout; -a fixed,lo -R seeded,c,hi is hysteresis thresholding of the frame."""
    h, w = fixture_image.shape
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + fixture_image.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canny_edge_amd", "Main")
    fixed = lambda thr, invert=0: binarize_rule.binarize(fixture_image[None], binarize_rule.FIXED, thr, invert=invert)[0]
    edges = R.pack((np.asarray(oracle.canny(fixture_image, 1.0, 50, 150)) != 0)[None])
    cases = ((("-a", "fixed,90", "-R", "seeded,8,170"), fixed(170), fixed(90), R.SEEDED, 8),
             (("-R", "seeded,4,60", "-a", "fixed,120,3,3,1"), fixed(60, 1), fixed(120, 1), R.SEEDED, 4),
             (("-a", "fixed,127", "-R", "fill"), None, fixed(127), R.FILL_HOLES, 8),
             (("-a", "otsu", "-R", "clear,4"), None, binarize_rule.binarize(fixture_image[None], binarize_rule.OTSU)[0], R.CLEAR_BORDER, 4),
             (("-R", "fill,4"), None, edges, R.FILL_HOLES, 4), (("-R", "clear"), None, edges, R.CLEAR_BORDER, 8))
    for i, (args, marker, mask, op, c) in enumerate(cases):
        out = tmp_path / f"out_{i}"
        out.mkdir()
        r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(out), *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want, info = R.reconstruct(marker, mask, w, op, c)
        data = (out / "canny_reconstruct.pgm").read_bytes()
        assert data.startswith(b"P5\n%d %d\n255\n" % (w, h))
        got = np.frombuffer(data[-h * w:], np.uint8).reshape(h, w)
        assert np.array_equal(got, np.where(R.unpack(want, w)[0], 255, 0)), args
        assert "reconstruct set %d mask %d start %d\n" % tuple(info[0].tolist()) in r.stdout, (args, r.stdout)
    usage = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "-R op[,connectivity[,thr]]" in usage.stderr and "canny_reconstruct.pgm" in usage.stderr
