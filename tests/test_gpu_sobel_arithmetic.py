"""The Sobel+NMS kernels' per-pixel arithmetic on the device, exhaustively and through the real kernels.

1. canny_hip_selftest_sobel_pixel runs each kernel form's own device helpers (magnitude, bin carrier, neighbour
   select, threshold floor) over all 4.16 M (gx, gy) in [-1020, 1020]^2 against the oracle's tables.
2. The adversarial planes of tests/sobel_planes.py (every gradient an interior pixel can have, the bin-boundary
   pairs at all four borders, tie ramps) go through dev_sobel_nms and dev_sobel_nms_u8in on every marching variant
   and through dev_canny at sigma 0.05 (fused classify on and off, u8 and s16 smoothed plane), bit for bit against
   the oracle.
"""
import numpy as np
import pytest

import oracle
import sobel_planes as sp

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables():
    return oracle.magnitude_table(1020), oracle.angle_table(1020)


@pytest.fixture(scope="module")
def planes():
    """The planes (one batch of N_PLANES frames) and the oracle's Sobel+NMS of each, computed once per module."""
    built = sp.build()
    frames = built["planes"]
    nms = np.stack([oracle.nms(*oracle.sobel(f.astype(np.int16))) for f in frames])
    return built, frames, nms


# ---------------------------------------------------------------------------------------------
# 1. Per-pixel self-test
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2, 3], ids=["lds_tile_d8", "packed_i16_march", "f32_march", "f32_march_floor"])
def test_selftest_sobel_pixel_exhaustive(ctx, hip, tables, form):
    mags, bins = ctx.selftest_sobel_pixel(form, 1020)
    want_m, want_b = tables
    bad_m, bad_b = np.argwhere(mags != want_m), np.argwhere(bins != want_b)
    assert bad_m.size == 0, (form, len(bad_m), (bad_m[:5] - 1020).tolist())  # rows: (gy, gx)
    assert bad_b.size == 0, (form, len(bad_b), (bad_b[:5] - 1020).tolist())


def test_selftest_sobel_pixel_small_lim_and_bad_form(ctx, hip):
    want_m, want_b = oracle.magnitude_table(7), oracle.angle_table(7)
    for form in (hip.PIXEL_LDS_TILE, hip.PIXEL_PACKED_I16, hip.PIXEL_F32, hip.PIXEL_F32_FLOOR):
        mags, bins = ctx.selftest_sobel_pixel(form, 7)
        assert np.array_equal(mags, want_m) and np.array_equal(bins, want_b), form
    for form, lim in ((4, 10), (-1, 10), (2, 1021)):
        with pytest.raises(hip.CannyHipError) as ei:
            ctx.selftest_sobel_pixel(form, lim)
        assert ei.value.status == ERR_INVALID


# ---------------------------------------------------------------------------------------------
# 2. The adversarial planes through the kernels
# ---------------------------------------------------------------------------------------------
@pytest.fixture(params=[(0, 0, 0), (2, 0, 0), (1, 0, 0), (1, 1, 0), (2, 0, 1), (1, 0, 1)],
                ids=["auto", "f32_everywhere", "packed_i16_everywhere", "packed_i16_4px_per_lane",
                     "f32_direct_plane_stores", "packed_i16_direct_plane_stores"])
def sobel_px(hip, request):
    """The marching kernel's process-wide variant switches (as in test_gpu_parity.py), restored afterwards."""
    variant, px, direct = request.param
    with hip.Context(0) as c:
        c.set_option("tune_sobel_variant", variant)
        c.set_option("tune_sobel_px", px)
        c.set_option("tune_plane_stores", direct)
    yield request.param
    with hip.Context(0) as c:
        c.set_option("tune_sobel_variant", 0)
        c.set_option("tune_sobel_px", 0)
        c.set_option("tune_plane_stores", 0)


def _report(got, want):
    bad = np.argwhere(got != want)
    return len(bad), [(*b.tolist(), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]]


@pytest.mark.parametrize("inp", ["s16", "u8"])
@pytest.mark.parametrize("path", [1, 2])
def test_sobel_nms_adversarial_planes(hip, planes, sobel_px, path, inp):
    built, frames, want = planes
    n, h, w = frames.shape
    src = frames.astype(np.int16) if inp == "s16" else frames
    # the u8-input kernel exists for 8 pixels per lane with the plane bytes staged in LDS only (launch_march)
    refused = inp == "u8" and (sobel_px[1] != 0 or sobel_px[2] != 0)
    with hip.Context(0) as c:
        c.set_option("sobel_nms_path", path)
        d_in, d_out = c.malloc(src.nbytes), c.malloc(n * h * w * 2)
        try:
            c.h2d(d_in, src)
            if inp == "s16":
                c.dev_sobel_nms(d_in, h, w, n, d_out)
            elif refused:
                with pytest.raises(hip.CannyHipError) as ei:
                    c.dev_sobel_nms_u8in(d_in, h, w, n, d_out)
                assert ei.value.status == ERR_UNSUPPORTED
                return
            else:
                c.dev_sobel_nms_u8in(d_in, h, w, n, d_out)
            got = np.empty((n, h, w), np.int16)
            c.d2h(got, d_out)
        finally:
            c.free(d_in)
            c.free(d_out)
    # the output holds the magnitudes themselves: the critical-margin centres the oracle keeps are compared here
    c = built["centres"][built["critical"]]
    assert np.count_nonzero(want[c[:, 0], c[:, 1], c[:, 2]]) >= 270
    assert np.array_equal(got, want), (sobel_px, path, inp, _report(got, want))


@pytest.fixture(scope="module")
def critical_magnitude(planes):
    """The largest magnitude of a critical-margin centre that the oracle's NMS keeps."""
    built, _, nms = planes
    c = built["centres"][built["critical"]]
    kept = nms[c[:, 0], c[:, 1], c[:, 2]]
    assert kept.max() > 1024
    return int(kept.max())


_oracle_canny = {}


# (255, 255) / (254, 255): every magnitude up to 255 occurs many times, a magnitude one off at the threshold flips an
# edge pixel.  (k, k) / (k, k + 1) with k the largest kept critical magnitude: the bit-plane kernel's threshold floor
# and strong test at the top of the range; the reference's map is empty there (promoted pixels are written as 255 and
# cleared again because 255 < max_val), so critical magnitudes are observed through the Sobel+NMS output above.
@pytest.mark.parametrize("spec", [(1, 1), (50, 150), (255, 255), (254, 255), ("k", 0), ("k", 1)],
                         ids=["1_1", "50_150", "255_255", "254_255", "k_k", "k_k+1"])
@pytest.mark.parametrize("u8", [1, 0], ids=["u8_smoothed_plane", "s16_smoothed_plane"])
@pytest.mark.parametrize("fuse", [1, 0], ids=["fused_classify", "classify_pass"])
def test_canny_adversarial_planes(hip, planes, critical_magnitude, spec, u8, fuse):
    built, frames, nms = planes
    n, h, w = frames.shape
    lo, hi = (critical_magnitude, critical_magnitude + spec[1]) if spec[0] == "k" else spec
    if (lo, hi) not in _oracle_canny:
        _oracle_canny[(lo, hi)] = np.stack([oracle.canny(f, 0.05, lo, hi) for f in frames])
    want = _oracle_canny[(lo, hi)]
    if hi == 255:
        assert np.count_nonzero((nms == hi) & (want != 0)) > 1000  # kept pixels sitting exactly on the threshold
    assert (np.count_nonzero(want) > 10 ** 6) == (hi <= 255)
    with hip.Context(0) as c:
        c.set_option("fuse_classify", fuse)
        c.set_option("smoothed_u8", u8)
        c.profile_enable(True)
        d_in, d_out = c.malloc(frames.nbytes), c.malloc(frames.nbytes * 2)
        try:
            c.h2d(d_in, frames)
            c.profile_reset()
            c.dev_canny(d_in, 0.05, lo, hi, h, w, n, d_out)
            classify_launches = c.profile_get(hip.STAGE_HYST_CLASSIFY)[1]
            got = np.empty(frames.shape, np.int16)
            c.d2h(got, d_out)
        finally:
            c.free(d_in)
            c.free(d_out)
        assert c.get_option("last_canny_smoothed_u8") == (u8 if fuse else 0)
    # the fused run wrote the hysteresis bit-planes from the Sobel+NMS kernel: no classify pass
    assert (classify_launches == 0) == bool(fuse), classify_launches
    assert np.array_equal(got, want), (fuse, u8, lo, hi, _report(got, want))
