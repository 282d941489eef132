"""CPU checks of the adversarial Gaussian planes (tests/gaussian_planes.py) that tests/test_gpu_gaussian_planes.py
runs through the kernels: the float32 model equals the oracle bit for bit, the planes reach what they were designed
to reach, and they are sensitive to one-ulp mistakes where random images are not.  The floors below are conditions on
the inputs and the reference, not on the kernels.

Measured (oracle and model agree on every figure):

critical pixels (quotient an integer or one ulp below one) per 300 x 964 frame
  sigma   half-window  noise, seed 3   mosaic frames 0..3
  0.3     1            6               131397 132829 130313 131523
  0.5     2            4                48965  48189  49157  48861
  1.0     3            9                76077  73510  75575  74258
  1.2     4            4                57336  55868  56837  55568
  1.4     5            7                41574  38992  40236  39736
  2.0     6            6                26542  24746  25193  25337
  2.3     7            10               27097  25474  25510  25692
  2.6     8            1                17576  16336  15778  16374
  1.9362  6            4                 3482   3454   3835   3601

pixels that differ from the oracle on the flat (24, 24) batch + mosaic frames 0 and 1: total (of which at distance
>= half-window from every frame border)
  mutant               sigma 1.0       sigma 1.4        sigma 2.0
  weights_descending    8372 (0)       31244 (0)        13917 (0)
  fma                  16668 (12657)   37517 (22494)    44795 (22763)
  pairs                 4960 (2671)    99275 (73826)   100628 (56685)
  reciprocal            1625 (0)        9551 (0)        15065 (4440)
"""
import numpy as np
import pytest

import gaussian_planes as gp
import oracle

ALL_SIGMAS = gp.HALF_WINDOW_SIGMAS + (gp.TABLE_MISS_SIGMA,)
MUTANT_SIGMAS = (1.0, 1.4, 2.0)
NOISE_SHAPES = ((37, 53), (97, 131))


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


@pytest.fixture(scope="module")
def planes():
    return gp.designed()


@pytest.fixture(scope="module")
def want(planes):
    """(name, sigma) -> the oracle's planes of every designed batch; computed once."""
    return {(name, s): np.stack([oracle.gaussian(f, s) for f in batch]) for name, batch in planes.items()
            for s in ALL_SIGMAS}


@pytest.fixture(scope="module")
def quotients(planes):
    """(name, sigma) -> the model's float planes before truncation."""
    return {(name, s): gp.model(batch, oracle.gaussian_kernel(s)) for name, batch in planes.items() for s in ALL_SIGMAS}


@pytest.fixture(scope="module")
def mutant_diffs(planes, want):
    """(mutant, sigma) -> (differing pixels, of which at distance >= C from every border) on the flat (24, 24) batch
    plus mosaic frames 0 and 1."""
    out = {}
    for s in MUTANT_SIGMAS:
        taps = oracle.gaussian_kernel(s)
        C = len(taps) // 2
        for m in gp.MUTANTS:
            total = inner = 0
            for name, batch in (("flat24x24", planes["flat24x24"]), ("mosaic", planes["mosaic"][:2])):
                diff = gp.model(batch, taps, m).astype(np.int16) != want[name, s][:len(batch)]
                total += int(diff.sum())
                inner += int((diff & (gp.border_distance(batch.shape[1:]) >= C)).sum())
            out[m, s] = (total, inner)
    return out


# ---- the model --------------------------------------------------------------------------------------------------------
def test_sigmas_cover_every_half_window():
    assert [len(oracle.gaussian_kernel(s)) // 2 for s in ALL_SIGMAS] == [1, 2, 3, 4, 5, 6, 7, 8, 6]


@pytest.mark.parametrize("sigma", ALL_SIGMAS)
def test_model_equals_oracle(planes, want, quotients, sigma):
    for name in planes:
        q = quotients[name, sigma]
        assert q.dtype == np.float32
        assert np.array_equal(q.astype(np.int16), want[name, sigma]), (sigma, name)
    taps = oracle.gaussian_kernel(sigma)
    for seed, (h, w) in enumerate(NOISE_SHAPES):
        img = _noise(h, w, seed + 1)
        assert np.array_equal(gp.model(img, taps).astype(np.int16), oracle.gaussian(img, sigma)), (sigma, h, w)


def test_model_rejects_unknown_mutants_and_types():
    taps = oracle.gaussian_kernel(1.0)
    with pytest.raises(ValueError):
        gp.model(np.zeros((4, 4), np.uint8), taps, "other")
    with pytest.raises(ValueError):
        gp.model(np.zeros((4, 4), np.int16), taps)


def test_critical_marks_integers_and_their_predecessors():
    f32 = np.float32
    q = np.array([0.0, 7.0, np.nextafter(f32(7), f32(0)), np.nextafter(f32(7), f32(8)), 6.5,
                  np.nextafter(f32(255), f32(0)), np.nextafter(np.nextafter(f32(7), f32(0)), f32(0))], f32)
    assert gp.critical(q).tolist() == [True, True, True, False, False, True, False]


# ---- the design -------------------------------------------------------------------------------------------------------
def test_flat_batches(planes):
    for h, w in gp.FLAT_SHAPES:
        b = planes[f"flat{h}x{w}"]
        assert b.shape == (256, h, w) and b.dtype == np.uint8 and b.flags["C_CONTIGUOUS"]
        assert np.array_equal(b.min((1, 2)), np.arange(256)) and np.array_equal(b.max((1, 2)), np.arange(256))
    # (24, 24): a pixel can lose taps on the left and on the right independently up to half-window 8, and there are
    # columns that lose none; (7, 40) / (40, 7): no row / column has its whole window inside for any half-window >= 4,
    # and at half-window 8 every one renormalises
    assert 24 >= 2 * 8 + 1 and 7 < 2 * 4 + 1 and 7 <= 8


def test_mosaic_recipe(planes):
    m = planes["mosaic"]
    assert m.shape == (gp.MOSAIC_FRAMES,) + gp.MOSAIC_SHAPE == (4, 300, 964) and m.dtype == np.uint8
    perm = np.random.default_rng(1234).permutation(256)
    ncx = (964 + 23) // 23 + 1
    for f in range(4):
        for y, x in ((0, 0), (17, 22), (150, 500), (299, 963)):
            cy, cx = (y + (5 * f) % 23) // 23, (x + (7 * f) % 23) // 23
            assert m[f, y, x] == perm[(cy * ncx + cx + 61 * f) % 256], (f, y, x)


def test_mosaic_cells_keep_a_flat_core(planes):
    """Every whole cell is constant, so at half-window 8 its middle 7 x 7 pixels see one level only."""
    assert gp.CELL - 2 * 8 == 7
    for f, m in enumerate(planes["mosaic"]):
        oy, ox = (-(5 * f)) % gp.CELL, (-(7 * f)) % gp.CELL  # first grid line inside the frame
        cells = m[oy:oy + (300 - oy) // 23 * 23, ox:ox + (964 - ox) // 23 * 23]
        cells = cells.reshape(cells.shape[0] // 23, 23, cells.shape[1] // 23, 23)
        assert (cells.min((1, 3)) == cells.max((1, 3))).all(), f
        # neighbouring cells differ: the edges are real
        flat = cells[:, 0, :, 0].astype(int)
        assert (np.diff(flat, axis=0) != 0).all() and (np.diff(flat, axis=1) != 0).all(), f


def test_mosaic_interior_window_has_every_level(planes):
    """Rows 20..279, columns 260..699 lie in interior strips and interior segments for every half-window (the widest
    strip is 252 columns, the segments are 67 rows)."""
    window = planes["mosaic"][:, 20:280, 260:700]
    assert np.array_equal(np.unique(window), np.arange(256))


def test_mosaic_edges_fall_on_every_lane_position(planes):
    """A lane holds four pixels of a row: cell edges sit at each of the four positions, in every frame, and the cell
    width shares no factor with a strip width, so the edges drift against the strip seams."""
    seam_offsets = {sw: set() for sw in (240, 244, 248, 252)}  # column of a strip seam within its cell
    for f, m in enumerate(planes["mosaic"]):
        edges = np.flatnonzero((m[:, 1:] != m[:, :-1]).any(0)) + 1  # first column of each cell
        assert np.array_equal(edges, np.arange((-(7 * f)) % 23 or 23, 964, 23)), f
        assert set((edges % 4).tolist()) == {0, 1, 2, 3}, f
        for sw, seen in seam_offsets.items():
            assert np.gcd(sw, gp.CELL) == 1
            seen |= {int((k * sw - edges[0]) % 23) for k in range(1, -(-964 // sw))}
    for sw, seen in seam_offsets.items():
        # some seam runs through the flat middle of a cell, some other within five columns of a cell edge
        assert any(8 <= o <= 14 for o in seen) and any(o <= 5 or o >= 18 for o in seen), (sw, sorted(seen))


# ---- sensitivity floors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", ALL_SIGMAS)
def test_mosaics_are_full_of_critical_pixels(quotients, sigma):
    floor = 2000 if sigma == gp.TABLE_MISS_SIGMA else 10000
    counts = [int(gp.critical(q).sum()) for q in quotients["mosaic", sigma]]
    print(sigma, "critical pixels per mosaic frame", counts)
    assert min(counts) >= floor, (sigma, counts)


@pytest.mark.parametrize("sigma", ALL_SIGMAS)
def test_noise_has_next_to_none(sigma):
    q = gp.model(_noise(300, 964, 3), oracle.gaussian_kernel(sigma))
    n = int(gp.critical(q).sum())
    print(sigma, "critical pixels in a noise frame", n)
    assert n <= 100, (sigma, n)


@pytest.mark.parametrize("sigma", MUTANT_SIGMAS)
@pytest.mark.parametrize("mutant", gp.MUTANTS)
def test_every_mutant_is_caught(mutant_diffs, mutant, sigma):
    """Any one of the four mistakes in the model breaks its equality with the oracle on the designed planes."""
    total, inner = mutant_diffs[mutant, sigma]
    print(mutant, sigma, "differing pixels", total, "of which away from the borders", inner)
    assert total >= 500, (mutant, sigma, total)


@pytest.mark.parametrize("sigma", MUTANT_SIGMAS)
def test_sum_order_mutants_are_caught_away_from_the_borders(mutant_diffs, sigma):
    for mutant in ("fma", "pairs"):
        assert mutant_diffs[mutant, sigma][1] >= 500, (mutant, sigma, mutant_diffs[mutant, sigma])


@pytest.mark.parametrize("sigma", MUTANT_SIGMAS)
def test_flat_frames_have_edges_in_the_reference(planes, want, sigma):
    """The reference itself truncates some pixels of a flat frame to g - 1 (the float quotient is g or one ulp less),
    so its edge maps of the flat frames at thresholds (1, 2) are not empty: the end-to-end GPU comparison can lose a
    pixel in either direction."""
    flat = want["flat24x24", sigma]
    levels = np.arange(256)[:, None, None]
    assert ((flat == levels) | (flat == levels - 1)).all() and (flat == levels - 1).any()
    edges = sum(int(np.count_nonzero(oracle.canny(f, sigma, 1, 2))) for f in planes["flat24x24"])
    print(sigma, "edge pixels of the 256 flat frames at thresholds (1, 2)", edges)
    assert edges > 0, sigma


@pytest.mark.parametrize("sigma", MUTANT_SIGMAS)
def test_weight_order_mutant_shows_at_the_borders_only(mutant_diffs, sigma):
    total, inner = mutant_diffs["weights_descending", sigma]
    assert inner == 0 and total >= 500, (sigma, total, inner)
