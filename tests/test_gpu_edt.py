"""The exact Euclidean distance transform on the GPU (canny_hip_dev_canny_edt / canny_hip_dev_edt_bits /
canny_hip_canny_edt): per pixel the squared distance to the nearest edge pixel, its correctly rounded root and the index of
that pixel (the smallest among equally near ones).

Reference: oracle.canny per frame -> the numpy rule of tests/edt_rule.py (and scipy at full size).  dist2 and nearest are
integers and dist is compared by its bytes: equality is exact.  The three planes are checked separately so that a failure
names which.  Every output buffer is pre-filled with a pattern and followed by guard words."""
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import components_rule
import edt_rule as rule
import oracle
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = np.int32(0x5A5A5A5A)
N_GUARD = 64
SHAPES = [(270, 480), (37, 53), (64, 8), (9, 2), (2, 9), (120, 1001), (256, 256), (130, 4096)]   # test_gpu_components.py
PLANES = ("dist2", "dist", "nearest")

_oracle_cache = {}


def _frames(n, h, w, seed0, first=None):
    fr = [synth_frame(h, w, seed0 + i) for i in range(n)]
    if first is not None:
        fr[0] = np.ascontiguousarray(first)
    return np.stack(fr)


def _oracle_maps(frames, sigma, lo, hi, key):
    k = (key, frames.shape, sigma, lo, hi)
    if k not in _oracle_cache:
        _oracle_cache[k] = np.stack([oracle.canny(f, sigma, lo, hi) for f in frames])
    return _oracle_cache[k]


class _Dev:
    """Device buffers of one transform call.  source: frames uint8 [n, h, w] (the canny route) or, with bits=True, packed
    bit maps [n, h, ceil(w / 8)] placed `shift` bytes into their allocation.  Planes are int32 words on this side; dist is
    compared by its bit pattern."""

    def __init__(self, ctx, source, h=None, w=None, bits=False, shift=0, dist2=True, dist=True, nearest=True, edges=False):
        self.ctx, self.bits = ctx, bits
        self.n = source.shape[0]
        self.h, self.w = (h, w) if bits else source.shape[1:]
        self.npx = self.n * self.h * self.w
        self.ptrs = []
        self.d_src = self._malloc(source.nbytes + shift + 16) + shift
        ctx.h2d(self.d_src, source)
        self.d_planes = [self._filled(np.full(self.npx + N_GUARD, GUARD32, np.int32)) if asked else 0
                         for asked in (dist2, dist, nearest)]
        self.d_edges = self._filled(np.full(self.npx, 0x5A5A, np.int16)) if edges else 0

    def _malloc(self, nbytes):
        p = self.ctx.malloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def _filled(self, a):
        p = self._malloc(a.nbytes)
        self.ctx.h2d(p, a)
        return p

    def run(self, sigma=None, lo=None, hi=None):
        if self.bits:
            self.ctx.dev_edt_bits(self.d_src, self.h, self.w, self.n, *self.d_planes)
        else:
            self.ctx.dev_canny_edt(self.d_src, sigma, lo, hi, self.h, self.w, self.n, *self.d_planes, self.d_edges)

    def plane(self, k):
        """(plane int32 [n, h, w], guard words) of output k."""
        a = np.empty(self.npx + N_GUARD, np.int32)
        self.ctx.d2h(a, self.d_planes[k])
        return a[:self.npx].reshape(self.n, self.h, self.w), a[self.npx:]

    def edges(self):
        a = np.empty(self.npx, np.int16)
        self.ctx.d2h(a, self.d_edges)
        return a.reshape(self.n, self.h, self.w)

    def check(self, want, what):
        """want = (dist2 int32, dist float32, nearest int32), each [n, h, w]: every output that exists, each named."""
        for k, name in enumerate(PLANES):
            if not self.d_planes[k]:
                continue
            got, guard = self.plane(k)
            assert np.array_equal(got, want[k].view(np.int32)), f"{what}: {name} differs"
            assert np.all(guard == GUARD32), f"{what}: written past {name}"

    def untouched(self):
        return all(np.all(self.plane(k)[0] == GUARD32) for k in range(3) if self.d_planes[k])

    def raw(self):
        return tuple(self.plane(k)[0].tobytes() for k in range(3) if self.d_planes[k])

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _empty_planes(n, h, w):
    return (np.full((n, h, w), rule.NONE, np.int32), np.full((n, h, w), np.inf, np.float32),
            np.full((n, h, w), -1, np.int32))


def _check_canny_call(ctx, frames, maps, sigma, lo, hi, what, edges=True, want=None, **outs):
    want = rule.stack(maps != 0) if want is None else want
    with _Dev(ctx, frames, edges=edges, **outs) as d:
        d.run(sigma, lo, hi)
        d.check(want, what)
        if edges:
            assert np.array_equal(d.edges(), maps), f"{what}: the s16 map differs from the oracle"
    return want


def _check_bits_call(ctx, masks, what, shift=0, pad_ones=False, want=None, **outs):
    n, h, w = masks.shape
    bits = np.packbits(masks, axis=-1)
    if pad_ones and w % 8:
        bits[..., -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    want = rule.stack(masks) if want is None else want
    with _Dev(ctx, bits, h=h, w=w, bits=True, shift=shift, **outs) as d:
        d.run()
        d.check(want, what)
    return want


# ---- through dev_canny_edt ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edt_matches_the_rule_on_the_oracles_maps(hip, fixture_image, shape):
    h, w = shape
    all_frames = _frames(3, h, w, 500 + h + w, first=fixture_image if shape == (256, 256) else None)
    with hip.Context(0) as ctx:
        for sigma, (lo, hi) in ((1.4, (50, 150)), (1.0, (1, 2)), (0.6, (20, 60)), (2.0, (10, 30))):
            all_maps = _oracle_maps(all_frames, sigma, lo, hi, "main")
            all_want = rule.stack(all_maps != 0)
            for n in (1, 3):
                frames, maps, want = all_frames[:n], all_maps[:n], tuple(p[:n] for p in all_want)
                what = f"{shape} sigma={sigma} thr=({lo},{hi}) n={n}"
                # d_edges, when given, is what dev_canny alone writes: the oracle's map
                _check_canny_call(ctx, frames, maps, sigma, lo, hi, "d_edges given, " + what, edges=True, want=want)
                _check_canny_call(ctx, frames, maps, sigma, lo, hi, "d_edges NULL, " + what, edges=False, want=want)


@pytest.mark.parametrize("shape", [(1, 64), (64, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_row_and_one_column_frames(hip, shape):
    """The detector itself needs two rows and two columns (the oracle and canny_hip_dev_canny both refuse less), and the
    transform's canny forms return dev_canny's status and write nothing.  The transform of such a map is checked through
    the bits route."""
    h, w = shape
    frames = _frames(2, h, w, 8)
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, edges=True) as d:
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1.4, 50, 150)
            assert ei.value.status == 2   # CANNY_HIP_ERR_UNSUPPORTED, dev_canny's own
            ctx.synchronize()
            assert d.untouched() and np.all(d.edges() == 0x5A5A)
        rng = np.random.default_rng(h * 7 + w)
        masks = np.stack([rng.random((h, w)) < p for p in (0.0, 0.05, 0.5, 1.0)])
        masks[1, h // 2, w // 2] = True
        _check_bits_call(ctx, masks, f"{shape} bits")
        _check_bits_call(ctx, masks[1:2], f"{shape} bits, one frame", shift=3)


def test_max_val_above_255_follows_the_map(hip):
    frames = _frames(3, 96, 256, 5)
    maps = _oracle_maps(frames, 1.0, 50, 300, "hi300")
    assert not maps.any(), "the oracle's map is all zero for max_val = 300"
    want = _empty_planes(3, 96, 256)
    with hip.Context(0) as ctx:
        _check_canny_call(ctx, frames, maps, 1.0, 50, 300, "max_val=300", want=want)
        d2, d, nn = ctx.canny_edt(frames, 1.0, 50, 300)
        assert np.all(d2 == rule.NONE), "dist2"
        assert np.all(np.isposinf(d)), "dist"
        assert np.all(nn == -1), "nearest"


def test_every_combination_of_null_outputs(hip):
    frames = _frames(3, 120, 1001, 21)
    maps = _oracle_maps(frames, 1.4, 50, 150, "nulls")
    want = rule.stack(maps != 0)
    with hip.Context(0) as ctx:
        for k in range(1, 8):
            outs = dict(dist2=bool(k & 1), dist=bool(k & 2), nearest=bool(k & 4))
            _check_canny_call(ctx, frames, maps, 1.4, 50, 150, f"{outs}", edges=False, want=want, **outs)
            _check_bits_call(ctx, maps != 0, f"bits, {outs}", pad_ones=True, want=want, **outs)
        with _Dev(ctx, frames, dist2=False, dist=False, nearest=False, edges=True) as d:   # nothing asked for
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1.4, 50, 150)
            assert ei.value.status == 1
            ctx.synchronize()
            assert np.all(d.edges() == 0x5A5A)
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.dev_edt_bits(1 << 20, 8, 8, 1, 0, 0, 0)
        assert ei.value.status == 1


def test_a_rejected_call_writes_nothing(hip):
    frames = _frames(2, 64, 64, 9)
    with hip.Context(0) as ctx:
        with _Dev(ctx, frames, edges=True) as d:
            with pytest.raises(hip.CannyHipError) as ei:
                d.run(1.0, 300, 100)
            assert ei.value.status == 5   # CANNY_HIP_ERR_DOMAIN, dev_canny's own
            # beyond the 32-bit limits: refused before anything is queued (the sizes are never used)
            for h, w in ((46341, 2), (2, 46341), (40000, 30000), (65536, 32768)):
                for call in (lambda: ctx.dev_canny_edt(d.d_src, 1.0, 50, 150, h, w, 1, *d.d_planes, d.d_edges),
                             lambda: ctx.dev_edt_bits(d.d_src, h, w, 1, *d.d_planes)):
                    with pytest.raises(hip.CannyHipError) as ei:
                        call()
                    assert ei.value.status == 2, (h, w)   # CANNY_HIP_ERR_UNSUPPORTED
            ctx.synchronize()
            assert d.untouched() and np.all(d.edges() == 0x5A5A)
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.canny_edt(frames, 1.0, 300, 100)
        assert ei.value.status == 5


# ---- through dev_edt_bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1024, 1024), (130, 4096), (129, 131), (37, 1001), (9, 2), (2, 9)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_directed_masks_through_the_bits_route(hip, shape):
    h, w = shape
    named = rule.directed_masks_large(h, w)
    for name, gen in (("cc_serpentine", components_rule.serpentine), ("cc_checkerboard", components_rule.checkerboard),
                      ("cc_combs", components_rule.combs), ("cc_staircase", components_rule.staircase)):
        named[name] = gen(h, w)
    masks = np.stack(list(named.values()))
    with hip.Context(0) as ctx:
        want = _check_bits_call(ctx, masks, f"directed {shape}: {list(named)}")
        _check_bits_call(ctx, masks, f"directed {shape}, dirty padding, odd address: {list(named)}", shift=1,
                         pad_ones=True, want=want)
    names = list(named)
    assert np.all(want[0][names.index("empty")] == rule.NONE) and not want[0][names.index("full")].any()


@pytest.mark.parametrize("density", [0.001, 0.05, 0.3, 0.9])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (37, 63), (40, 64), (33, 65), (66, 129), (200, 333), (3, 4600),
                                   (300, 4100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_masks_through_the_bits_route(hip, shape, density):
    h, w = shape
    masks = np.random.default_rng(17 * h + w).random((3, h, w)) < density
    with hip.Context(0) as ctx:
        _check_bits_call(ctx, masks, f"{shape} density={density}", shift=1, pad_ones=True)


def test_maps_at_any_byte_address(hip):
    h, w = 77, 203
    masks = np.random.default_rng(12).random((4, h, w)) < 0.03
    want = rule.stack(masks)
    with hip.Context(0) as ctx:
        for shift in (0, 1, 3, 7):
            _check_bits_call(ctx, masks, f"shift={shift}", shift=shift, pad_ones=bool(shift & 1), want=want)


def test_frames_of_a_batch_do_not_leak_into_each_other(hip):
    h, w = 150, 330
    rng = np.random.default_rng(99)
    masks = np.stack([np.zeros((h, w), bool), np.ones((h, w), bool), rng.random((h, w)) < 0.01,
                      np.zeros((h, w), bool), rng.random((h, w)) < 0.4, np.ones((h, w), bool),
                      np.zeros((h, w), bool), rng.random((h, w)) < 0.0005, np.zeros((h, w), bool)])
    with hip.Context(0) as ctx:
        want = _check_bits_call(ctx, masks, "empty / full / random alternating", pad_ones=True)
        _check_bits_call(ctx, masks[::-1].copy(), "... reversed", want=tuple(p[::-1] for p in want))
        _check_bits_call(ctx, masks, "... dist2 NULL (the stack in the workspace)", want=want, dist2=False)


# ---- host form, sizes, reuse -------------------------------------------------------------------------------------------
def test_host_form_brings_down_only_what_was_asked_for(hip):
    frames = _frames(3, 270, 480, 31)
    maps = _oracle_maps(frames, 1.4, 50, 150, "host")
    want = rule.stack(maps != 0)
    with hip.Context(0) as ctx:
        d2, d, nn = ctx.canny_edt(frames, 1.4, 50, 150)
        assert d2.dtype == np.int32 and np.array_equal(d2, want[0]), "dist2"
        assert d.dtype == np.float32 and d.tobytes() == want[1].tobytes(), "dist"
        assert nn.dtype == np.int32 and np.array_equal(nn, want[2]), "nearest"
        for k in range(1, 7):
            flags = [bool(k & 1), bool(k & 2), bool(k & 4)]
            got = ctx.canny_edt(frames[0], 1.4, 50, 150, *flags)
            for name, asked, g, wnt in zip(PLANES, flags, got, want):
                assert (g is not None) == asked, name
                if asked:
                    assert g.tobytes() == wnt[:1].tobytes(), f"{name} with outputs {flags}"


def test_two_4k_frames_against_scipy(hip):
    frames = _frames(2, 2160, 3840, 1)
    maps = _oracle_maps(frames, 1.4, 50, 150, "4k")
    assert int((maps[0] != 0).sum()) == 62325
    with hip.Context(0) as ctx, _Dev(ctx, frames) as d:
        d.run(1.4, 50, 150)
        got = [d.plane(k) for k in range(3)]
    for f in range(2):
        mask = maps[f] != 0
        e = ndimage.distance_transform_edt(~mask)
        assert np.array_equal(got[0][0][f], np.rint(e * e).astype(np.int32)), f"frame {f}: dist2 differs from scipy"
        assert got[1][0][f].tobytes() == e.astype(np.float32).tobytes(), f"frame {f}: dist differs from scipy"
        want_d2, want_nn = rule.separable(mask)
        assert np.array_equal(got[0][0][f], want_d2), f"frame {f}: dist2 differs from the rule"
        assert np.array_equal(got[2][0][f], want_nn), f"frame {f}: nearest differs from the rule"
    for k, name in enumerate(PLANES):
        assert np.all(got[k][1] == GUARD32), f"written past {name}"


def test_one_edge_pixel_and_none_in_4096_x_4096(hip):
    h = w = 4096
    masks = np.zeros((2, h, w), bool)
    masks[0, 1234, 3210] = True
    r, c = np.indices((h, w))
    d2 = ((r - 1234) ** 2 + (c - 3210) ** 2).astype(np.int32)
    one = (d2, rule.dist_of(d2), np.full((h, w), 1234 * w + 3210, np.int32))
    want = tuple(np.stack([a, b[0]]) for a, b in zip(one, _empty_planes(1, h, w)))
    with hip.Context(0) as ctx:
        _check_bits_call(ctx, masks, "one pixel / no pixel, 4096 x 4096", want=want)


def test_same_bytes_on_every_run(hip):
    frames = _frames(6, 270, 480, 77)
    with hip.Context(0) as ctx:
        runs = []
        for k in range(3):
            if k == 2:   # an unrelated call on the context in between
                ctx.canny_points(_frames(2, 96, 256, 1), 1.4, 50, 150)
            with _Dev(ctx, frames) as d:
                d.run(1.0, 1, 2)
                runs.append(d.raw())
        assert runs[0] == runs[1] == runs[2]


def test_edt_call_after_an_unflushed_stream_call(hip):
    h, w = 96, 256
    streamed, mine = _frames(5, h, w, 1200), _frames(3, h, w, 1300)
    streamed_maps = _oracle_maps(streamed, 1.4, 50, 150, "streamed")
    maps = _oracle_maps(mine, 1.4, 50, 150, "mine")
    want = rule.stack(maps != 0)
    with hip.Context(0) as ctx:
        ctx.set_option("hysteresis_tail", 0)
        d_in, d_map = ctx.malloc(streamed.nbytes), ctx.malloc(streamed.nbytes * 2)
        try:
            ctx.h2d(d_in, streamed)
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_canny_call(ctx, mine, maps, 1.4, 50, 150, "after a streamed call", want=want)
            got = np.empty(streamed.shape, np.int16)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map"
            # ... and the bits form flushes a pending lane as well
            ctx.dev_canny_stream(d_in, 1.4, 50, 150, h, w, 5, d_map)
            _check_bits_call(ctx, maps != 0, "bits form after a streamed call", want=want)
            ctx.d2h(got, d_map)
            assert np.array_equal(got, streamed_maps), "the streamed batch's map (2)"
        finally:
            ctx.free(d_in)
            ctx.free(d_map)


@pytest.mark.parametrize("edt_first", [False, True], ids=["components_then_edt", "edt_then_components"])
def test_components_and_edt_share_a_context(hip, edt_first):
    frames = _frames(3, 130, 4096, 61)
    maps = _oracle_maps(frames, 1.4, 50, 150, "shared")
    want = rule.stack(maps != 0)
    want_l, _, want_s, want_off = (lambda l, s, o: (l, None, s, o))(*components_rule.csr(maps, 2))

    def run_components(ctx):
        l, k, s, off = ctx.canny_components(frames, 1.4, 50, 150, min_area=2, want_labels=False, want_kept=True)
        assert np.array_equal(off, want_off), "components: offsets"
        assert np.array_equal(s, want_s), "components: stats"
        assert np.array_equal(k, np.where(want_l != 0, 255, 0)), "components: kept_u8"

    def run_edt(ctx, what):
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, what, want=want)
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, what + ", dist2 NULL", want=want, dist2=False, edges=False)

    with hip.Context(0) as ctx:
        for _ in range(2):
            if edt_first:
                run_edt(ctx, "EDT before components")
                run_components(ctx)
            else:
                run_components(ctx)
                run_edt(ctx, "EDT after components")


def test_cli_writes_the_distance_image(hip, fixture_image, tmp_path):
    h, w = fixture_image.shape
    src = tmp_path / "in.pgm"
    src.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + fixture_image.tobytes())
    out = tmp_path / "out"
    out.mkdir()
    exe = os.path.join(ROOT, "canny_edge_amd", "Main")
    r = subprocess.run([exe, "1.0", "50", "150", "-i", str(src), "-o", str(out), "-d"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    d2 = rule.transform(oracle.canny(fixture_image, 1.0, 50, 150) != 0)[0].astype(np.int64)
    root = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    root = root - (root * root > d2) + ((root + 1) * (root + 1) <= d2)   # the integer square root, whatever sqrt rounded
    data = (out / "canny_dist.pgm").read_bytes()
    assert data.startswith(b"P5\n%d %d\n255\n" % (w, h))
    got = np.frombuffer(data[-h * w:], np.uint8).reshape(h, w)
    assert np.array_equal(got, np.minimum(root, 255))
    assert not (out / "canny_kept.pgm").exists()   # -d alone asks for nothing else
    usage = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "-d:" in usage.stderr and "canny_dist.pgm" in usage.stderr


def test_parts_are_timed_and_the_stages_are_unaffected(hip):
    frames = _frames(2, 96, 256, 3)
    maps = _oracle_maps(frames, 1.4, 50, 150, "timed")
    with hip.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 0b11 << 17)
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, "profiled", edges=False)
        for part in range(2):
            ms, launches = ctx.edt_profile_get(part)
            assert launches == 1 and ms > 0.0, hip.EDT_PARTS[part]
        for stage in range(9):
            assert ctx.profile_get(stage)[1] == 0
        assert ctx.hough_profile_get(0)[1] == 0 and ctx.components_profile_get(0)[1] == 0
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0)   # all stages
        _check_canny_call(ctx, frames, maps, 1.4, 50, 150, "profiled, all stages", edges=False, nearest=False)
        assert ctx.profile_get(hip.STAGE_GAUSSIAN)[1] == 1
        assert ctx.edt_profile_get(0)[1] == 1 and ctx.edt_profile_get(1)[1] == 1
        with pytest.raises(hip.CannyHipError):
            ctx.edt_profile_get(2)
