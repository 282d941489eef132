"""Per-frame hysteresis thresholds on the GPU (canny_hip_*_thresholds, canny_hip_*_auto).

The pairs the automatic rules report must equal the numpy restatement of the rule applied to np.bincount of the oracle's
smoothed plane (median) or of min(magnitude, 256) (quantile), and every frame's map must equal
oracle.canny(frame, sigma, min_f, max_f) -- on every kernel path, through the device and the batch entry points."""
import math

import numpy as np
import pytest

import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

# sigma -> window 1 + 2 ceil(3 sigma): 3 .. 17 (marching Gaussian), 4.0 -> 25 (generic Gaussian)
SIGMAS = (0.3, 0.6, 1.0, 1.2, 1.4, 1.8, 2.2, 2.5, 4.0)
RULES = (("median", 0.67, 1.33), ("quantile", 0.7, 0.9))
DEFAULTS = {"fuse_classify": 1, "smoothed_u8": 1, "sobel_nms_path": 0, "hysteresis_tail": 1, "overlap_hysteresis": 0,
            "tune_batch_chunk_frames": 0, "tune_batch_compact": 0}


def np_quantile(hist, q):
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64))
    need = max(1, math.ceil(float(np.float32(q)) * float(int(cum[-1]))))
    return int(np.searchsorted(cum, need, side="left"))


def np_rule(hist, rule, low, high):
    if rule == "median":
        m = np_quantile(hist, 0.5)
        lo, hi = math.floor(float(np.float32(low)) * m), math.floor(float(np.float32(high)) * m)
    else:
        lo, hi = np_quantile(hist, low), np_quantile(hist, high)
    lo = min(max(lo, 1), 255)
    return lo, min(max(hi, lo), 255)


def want_pair(frame, sigma, rule, low, high):
    st = oracle.canny(frame, sigma, 1, 1, stages=True)
    plane = st["smoothed"] if rule == "median" else np.minimum(st["magnitude"], 256)
    return np_rule(np.bincount(plane.ravel().astype(np.int64), minlength=257), rule, low, high)


def mixed_batch(h, w, seed=0):
    """Frames that need different thresholds: synth frames, contrast-scaled copies, constant 0 / 255, uniform noise."""
    rng = np.random.default_rng(seed)
    a, b, c = (synth_frame(h, w, seed * 7 + k) for k in range(3))
    frames = [a, b, c,
              (a.astype(np.float32) * 0.25 + 100).astype(np.uint8),  # low contrast
              (b.astype(np.float32) * 0.5).astype(np.uint8),  # dark
              np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8),
              rng.integers(0, 256, (h, w), dtype=np.uint8)]
    return np.stack(frames)


def check_auto(frames, sigma, rule, low, high, edges, thr):
    for f in range(frames.shape[0]):
        want = want_pair(frames[f], sigma, rule, low, high)
        assert tuple(int(v) for v in thr[f]) == want, (f, rule, sigma)
        assert np.array_equal(edges[f], oracle.canny(frames[f], sigma, *want)), (f, rule, sigma, want)


@pytest.fixture(scope="module")
def ctx(hip):
    with capi.Context(0) as c:
        yield c


@pytest.fixture
def octx(ctx):
    """The module context, its options restored after each test."""
    yield ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


class Dev:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 1))
        self.ptrs.append(p)
        self.ctx.h2d(p, a)
        return p

    def alloc(self, nbytes):
        p = self.ctx.malloc(nbytes)
        self.ptrs.append(p)
        return p

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.synchronize()
        self.ctx.d2h(out, p)
        return out

    def free(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.free(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free()


def dev_auto(ctx, dev, frames, sigma, rule, low, high):
    n, h, w = frames.shape
    d_in, d_out, d_thr = dev.up(frames), dev.alloc(frames.size * 2), dev.alloc(n * 8)
    ctx.dev_canny_auto(d_in, sigma, rule, low, high, h, w, n, d_out, d_thr)
    return dev.down(d_out, frames.shape, np.int16), dev.down(d_thr, (n, 2), np.int32)


# ---- reported thresholds and maps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,low,high", RULES)
def test_auto_batch_matches_numpy_rule_and_oracle(octx, rule, low, high):
    frames = mixed_batch(72, 128)
    edges, thr = octx.canny_auto(frames, 1.4, rule, low, high)
    assert thr.shape == (frames.shape[0], 2) and thr.dtype == np.int32
    assert len({tuple(t) for t in thr}) >= 4  # the batch really needs different pairs
    check_auto(frames, 1.4, rule, low, high, edges, thr)


@pytest.mark.parametrize("rule,low,high", RULES)
def test_auto_single_frame_and_module_function(octx, rule, low, high):
    img = synth_frame(90, 120, 5)
    edges, thr = octx.canny_auto(img, 1.0, rule, low, high)
    assert edges.shape == img.shape and thr.shape == (2,)
    check_auto(img[None], 1.0, rule, low, high, edges[None], thr[None])
    e2, t2 = capi.canny_auto(img, 1.0, rule, low, high)
    assert np.array_equal(e2, edges) and np.array_equal(t2, thr)


@pytest.mark.parametrize("rule,low,high", RULES + (("median", 0.0, 5.0), ("quantile", 1e-6, 1.0),
                                                   ("median", 1.0, 1.0), ("quantile", 0.5, 0.5)))
def test_dev_auto_matches_numpy_rule_and_oracle(octx, dev, rule, low, high):
    frames = mixed_batch(64, 96, seed=1)
    edges, thr = dev_auto(octx, dev, frames, 1.4, rule, low, high)
    check_auto(frames, 1.4, rule, low, high, edges, thr)
    # without a pair array: the same maps
    n, h, w = frames.shape
    d_in, d_out = dev.up(frames), dev.alloc(frames.size * 2)
    octx.dev_canny_auto(d_in, 1.4, rule, low, high, h, w, n, d_out)
    assert np.array_equal(dev.down(d_out, frames.shape, np.int16), edges)


def test_dev_auto_rejects_bad_arguments(octx, dev):
    frames = mixed_batch(16, 16)
    n, h, w = frames.shape
    d_in, d_out = dev.up(frames), dev.alloc(frames.size * 2)
    for rule, low, high in ((0, 0.5, 1.0), (3, 0.5, 1.0), (1, -1.0, 1.0), (1, 2.0, 1.0), (2, 0.0, 0.5),
                            (2, 0.5, 1.5), (1, float("nan"), 1.0), (2, 0.5, float("nan"))):
        st = octx._L.canny_hip_dev_canny_auto(octx._h, d_in, 1.0, rule, low, high, h, w, n, d_out, None)
        assert st == 1, (rule, low, high)
        st = octx._L.canny_hip_canny_batch_auto(octx._h, capi._hp(frames), n, 1.0, rule, low, high, h, w,
                                                capi._hp(np.empty(frames.shape, np.int16)), None)
        assert st == 1, (rule, low, high)


# ---- explicit per-frame pairs --------------------------------------------------------------------------------------
PAIRS = [(50, 150), (1, 1), (10, 40), (200, 255), (1, 255), (90, 90), (30, 200), (120, 180)]


def test_explicit_pairs_batch_matches_per_frame_oracle(octx):
    frames = mixed_batch(72, 128, seed=2)
    edges = octx.canny_thresholds(frames, 1.4, PAIRS)
    for f, (lo, hi) in enumerate(PAIRS):
        assert np.array_equal(edges[f], oracle.canny(frames[f], 1.4, lo, hi)), f


def test_explicit_pairs_device_out_of_domain_are_clamped(octx, dev):
    frames = mixed_batch(64, 96, seed=3)
    n, h, w = frames.shape
    raw = np.array([(0, 50), (-5, 300), (200, 100), (300, 400), (256, 10), (0, 0), (-7, -3), (40, 2**31 - 1)],
                   np.int32)
    d_in, d_thr, d_out = dev.up(frames), dev.up(raw), dev.alloc(frames.size * 2)
    octx.dev_canny_thresholds(d_in, 1.4, d_thr, h, w, n, d_out)
    edges = dev.down(d_out, frames.shape, np.int16)
    for f, (lo, hi) in enumerate(raw.tolist()):
        lo = min(max(lo, 1), 255)
        hi = min(max(hi, lo), 255)
        assert np.array_equal(edges[f], oracle.canny(frames[f], 1.4, lo, hi)), (f, lo, hi)


@pytest.mark.parametrize("bad", [(0, 50), (60, 50), (10, 256), (-1, 5)])
def test_explicit_pairs_host_rejects_out_of_domain(octx, bad):
    frames = mixed_batch(32, 64)
    pairs = list(PAIRS)
    pairs[5] = bad
    out = np.full(frames.shape, 77, np.int16)
    with pytest.raises(capi.CannyHipError) as ei:
        octx.canny_thresholds(frames, 1.0, pairs, out=out)
    assert ei.value.status == 1
    assert (out == 77).all()


# ---- every kernel path ---------------------------------------------------------------------------------------------
def _oracle_thr_maps(frames, sigma, pairs):
    return np.stack([oracle.canny(f, sigma, int(lo), int(hi)) for f, (lo, hi) in zip(frames, pairs)])


@pytest.mark.parametrize("width", [64, 62])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("rule,low,high", RULES)
def test_paths_sigma_and_width(octx, dev, sigma, width, rule, low, high):
    frames = mixed_batch(40, width, seed=4)
    edges, thr = dev_auto(octx, dev, frames, sigma, rule, low, high)
    check_auto(frames, sigma, rule, low, high, edges, thr)
    n, h, w = frames.shape
    d_in, d_thr, d_out = dev.up(frames), dev.up(np.array(PAIRS, np.int32)), dev.alloc(frames.size * 2)
    octx.dev_canny_thresholds(d_in, sigma, d_thr, h, w, n, d_out)
    assert np.array_equal(dev.down(d_out, frames.shape, np.int16), _oracle_thr_maps(frames, sigma, PAIRS))


OPTION_SETS = [{"fuse_classify": 0}, {"smoothed_u8": 0}, {"sobel_nms_path": 1}, {"hysteresis_tail": 0},
               {"fuse_classify": 0, "smoothed_u8": 0}, {"hysteresis_tail": 0, "smoothed_u8": 0}]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("width", [64, 62])
@pytest.mark.parametrize("rule,low,high", RULES)
def test_paths_options(octx, dev, opts, width, rule, low, high):
    frames = mixed_batch(48, width, seed=5)
    for k, v in opts.items():
        octx.set_option(k, v)
    for sigma in (1.0, 1.4):
        edges, thr = dev_auto(octx, dev, frames, sigma, rule, low, high)
        check_auto(frames, sigma, rule, low, high, edges, thr)
        n, h, w = frames.shape
        d_in, d_thr, d_out = dev.up(frames), dev.up(np.array(PAIRS, np.int32)), dev.alloc(frames.size * 2)
        octx.dev_canny_thresholds(d_in, sigma, d_thr, h, w, n, d_out)
        assert np.array_equal(dev.down(d_out, frames.shape, np.int16), _oracle_thr_maps(frames, sigma, PAIRS))


@pytest.mark.parametrize("smoothed_u8", [1, 0])
@pytest.mark.parametrize("rule,low,high", RULES)
def test_paths_overlap_hysteresis(octx, dev, smoothed_u8, rule, low, high):
    frames = np.concatenate([mixed_batch(40, 64, seed=6), mixed_batch(40, 64, seed=7), mixed_batch(40, 64, seed=8)])
    assert frames.shape[0] >= 16
    octx.set_option("overlap_hysteresis", 1)
    octx.set_option("smoothed_u8", smoothed_u8)
    edges, thr = dev_auto(octx, dev, frames, 1.4, rule, low, high)
    check_auto(frames, 1.4, rule, low, high, edges, thr)
    pairs = np.array([PAIRS[(5 * f) % len(PAIRS)] for f in range(frames.shape[0])], np.int32)
    n, h, w = frames.shape
    d_in, d_thr, d_out = dev.up(frames), dev.up(pairs), dev.alloc(frames.size * 2)
    octx.dev_canny_thresholds(d_in, 1.4, d_thr, h, w, n, d_out)
    assert np.array_equal(dev.down(d_out, frames.shape, np.int16), _oracle_thr_maps(frames, 1.4, pairs))


@pytest.mark.parametrize("smoothed_u8", [1, 0])
@pytest.mark.parametrize("shape", [(37, 53), (33, 31)])
@pytest.mark.parametrize("rule,low,high", RULES)
def test_paths_odd_pixel_counts(octx, dev, shape, smoothed_u8, rule, low, high):
    """Frames whose pixel count is no multiple of 16 start inside the intensity histogram's 16-pixel groups and end the
    batch with a partial one: the masked paths, on the plane the real Gaussian wrote (bytes and shorts).
    tests/test_gpu_histograms.py pins the same paths bin by bin on designed planes."""
    frames = mixed_batch(*shape, seed=12)
    assert frames[0].size % 16 not in (0, 8)
    octx.set_option("smoothed_u8", smoothed_u8)
    edges, thr = dev_auto(octx, dev, frames, 1.4, rule, low, high)
    check_auto(frames, 1.4, rule, low, high, edges, thr)
    edges, thr = octx.canny_auto(frames, 1.4, rule, low, high)
    check_auto(frames, 1.4, rule, low, high, edges, thr)


# ---- batch pipeline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("pinned", [False, True])
def test_batch_pipeline_chunks_match_dev(octx, dev, compact, pinned):
    frames = np.concatenate([mixed_batch(48, 80, seed=9), mixed_batch(48, 80, seed=10)[:2]])
    assert frames.shape[0] == 10
    n, h, w = frames.shape
    pairs = np.array([PAIRS[(3 * f) % len(PAIRS)] for f in range(n)], np.int32)
    # device results first, on the default options
    want = {}
    for rule, low, high in RULES:
        want[rule] = dev_auto(octx, dev, frames, 1.4, rule, low, high)
    d_in, d_thr, d_out = dev.up(frames), dev.up(pairs), dev.alloc(frames.size * 2)
    octx.dev_canny_thresholds(d_in, 1.4, d_thr, h, w, n, d_out)
    want_explicit = dev.down(d_out, frames.shape, np.int16)
    octx.set_option("tune_batch_chunk_frames", 3)
    octx.set_option("tune_batch_compact", compact)
    src = frames
    if pinned:
        src = octx.pinned_array(frames.shape, np.uint8)
        src[...] = frames
    for rule, low, high in RULES:
        edges, thr = octx.canny_auto(src, 1.4, rule, low, high)
        assert np.array_equal(thr, want[rule][1]), rule
        assert np.array_equal(edges, want[rule][0]), rule
    assert np.array_equal(octx.canny_thresholds(src, 1.4, pairs), want_explicit)


# ---- no state leaks ------------------------------------------------------------------------------------------------
def test_fixed_canny_after_auto_matches_fresh_context(octx, dev):
    frames = mixed_batch(64, 128, seed=11)
    for rule, low, high in RULES:
        octx.canny_auto(frames, 1.4, rule, low, high)
        dev_auto(octx, dev, frames, 1.4, rule, low, high)
    octx.canny_thresholds(frames, 1.4, PAIRS)
    got = [octx.canny(f, 1.4, 50, 150) for f in frames]
    n, h, w = frames.shape
    d_in, d_out = dev.up(frames), dev.alloc(frames.size * 2)
    octx.dev_canny(d_in, 1.4, 50, 150, h, w, n, d_out)
    got_dev = dev.down(d_out, frames.shape, np.int16)
    with capi.Context(0) as fresh:
        for f, g in zip(frames, got):
            assert np.array_equal(g, fresh.canny(f, 1.4, 50, 150))
        assert np.array_equal(got_dev, fresh.canny_batch(frames, 1.4, 50, 150))


# ---- full size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,low,high", RULES)
def test_full_size_4k(octx, rule, low, high):
    frames = np.stack([synth_frame(2160, 3840, 60),
                       (synth_frame(2160, 3840, 61).astype(np.float32) * 0.3 + 80).astype(np.uint8),
                       np.zeros((2160, 3840), np.uint8),
                       np.random.default_rng(62).integers(0, 256, (2160, 3840), dtype=np.uint8)])
    edges, thr = octx.canny_auto(frames, 1.4, rule, low, high)
    check_auto(frames, 1.4, rule, low, high, edges, thr)
