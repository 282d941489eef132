"""CPU checks of the adversarial Sobel planes (tests/sobel_planes.py) that tests/test_gpu_sobel_arithmetic.py runs
through the kernels: the planes carry exactly the intended gradients, the reachable set is right, and canny() at
sigma 0.05 sees the planes themselves."""
import itertools

import numpy as np
import pytest

import oracle
import sobel_planes as sp

# every pixel offset the Sobel stencil weighs, with its (gx, gy) weights
_CELLS = [((-1, -1), (-1, -1)), ((-1, 0), (0, -2)), ((-1, 1), (1, -1)), ((0, -1), (-2, 0)), ((0, 1), (2, 0)),
          ((1, -1), (-1, 1)), ((1, 0), (0, 2)), ((1, 1), (1, 1))]


@pytest.fixture(scope="module")
def built():
    return sp.build()


def _minkowski(vmax):
    """Reachable (gx, gy) at an interior pixel as the Minkowski sum of the eight cells' segments {0..vmax} * weight
    (independent of the closed form): a boolean grid indexed [gy + 4 vmax, gx + 4 vmax]."""
    lim = 4 * vmax
    grid = np.zeros((2 * lim + 1, 2 * lim + 1), bool)
    grid[lim, lim] = True
    for _, (wx, wy) in _CELLS:
        acc = grid
        for v in range(1, vmax + 1):
            acc = acc | np.roll(np.roll(grid, v * wy, 0), v * wx, 1)
        grid = acc
    return grid


@pytest.mark.parametrize("vmax", [1, 2, 5])
def test_reachable_set_matches_brute_force(vmax):
    """Every 3x3 block over [0, vmax] enumerated: its gradients are exactly interior_reachable's set."""
    lim = 4 * vmax
    vals = np.array(list(itertools.product(range(vmax + 1), repeat=8)), np.int64)
    gx = sum(vals[:, k] * wx for k, (_, (wx, _)) in enumerate(_CELLS))
    gy = sum(vals[:, k] * wy for k, (_, (_, wy)) in enumerate(_CELLS))
    want = np.zeros((2 * lim + 1, 2 * lim + 1), bool)
    want[gy + lim, gx + lim] = True
    g = np.arange(-lim, lim + 1)
    GX, GY = np.meshgrid(g, g)
    assert np.array_equal(sp.interior_reachable(GX, GY, vmax), want)
    assert np.array_equal(_minkowski(vmax), want)


def test_reachable_set_full_range():
    g = np.arange(-sp.LIM, sp.LIM + 1)
    GX, GY = np.meshgrid(g, g)
    reach = sp.interior_reachable(GX, GY)
    assert np.array_equal(reach, _minkowski(sp.VMAX))
    assert int(reach.sum()) == 1822741


@pytest.mark.parametrize("kind", ["left", "right", "top", "bottom"])
def test_border_blocks_give_their_pairs(kind):
    """Each band's half-blocks, alone in a small plane, have the intended gradient at the border pixel; a pair the
    solver rejects has no half-block at all (checked by enumeration on a reduced value range)."""
    vmax = 3
    lim = 4 * vmax
    g = np.arange(-lim, lim + 1)
    GX, GY = (a.ravel() for a in np.meshgrid(g, g))
    blk, ok = sp.border_blocks(kind, GX, GY, vmax)
    vals = np.array(list(itertools.product(range(vmax + 1), repeat=6)), np.int64)
    shape = (3, 2) if kind in ("left", "right") else (2, 3)
    cy, cx = {"left": (1, 0), "right": (1, 1), "top": (0, 1), "bottom": (1, 1)}[kind]
    reach = set()
    for v in vals[:: max(1, len(vals) // 4096)]:
        gx, gy = oracle.xy_gradient(v.reshape(shape).astype(np.int16))
        reach.add((int(gx[cy, cx]), int(gy[cy, cx])))
    for i in np.flatnonzero(ok):
        gx, gy = oracle.xy_gradient(blk[i].astype(np.int16))
        assert (int(gx[cy, cx]), int(gy[cy, cx])) == (GX[i], GY[i]), (kind, GX[i], GY[i])
    assert reach <= set(zip(GX[ok].tolist(), GY[ok].tolist())), kind


def test_planes_carry_the_intended_pairs(built):
    planes, c = built["planes"], built["centres"]
    assert planes.shape[2] % 8 == 0 and planes.shape[2] > 2 * 496
    for p in range(planes.shape[0]):
        gx, gy = oracle.xy_gradient(planes[p].astype(np.int16))
        m = c[:, 0] == p
        assert np.array_equal(gx[c[m, 1], c[m, 2]], c[m, 3])
        assert np.array_equal(gy[c[m, 1], c[m, 2]], c[m, 4])
    interior = c[built["kind"] == 0]
    # every reachable pair is placed at an interior pixel, and the centres cover every pixel-in-lane position
    placed = set(zip(interior[:, 3].tolist(), interior[:, 4].tolist()))
    assert len(placed) == built["n_interior"] == 1822741
    assert set((interior[:, 2] % 8).tolist()) == set(range(8))
    # the border bands: every band reached, each on its own border, none full (so no reachable pair was dropped)
    band = c[built["kind"] == 1]
    H, W = planes.shape[1:]
    assert ((band[:, 1] == 0) | (band[:, 1] == H - 1) | (band[:, 2] == 0) | (band[:, 2] == W - 1)).all()
    assert all(built["band_use"][k] > 500 and built["band_use"][k] < built["band_capacity"][k] for k in built["band_use"])


def test_band_pairs_are_the_reachable_boundary_pairs(built):
    """The bands hold every bin-boundary pair that some border formula reaches (critical-margin pairs need
    |gx|, |gy| beyond what a border pixel can produce: none is reachable there)."""
    bgx, bgy = sp.bin_boundary_pairs()
    cgx, cgy = sp.critical_pairs()
    reach = np.zeros(bgx.size, bool)
    creach = np.zeros(cgx.size, bool)
    for kind in ("left", "right", "top", "bottom"):
        reach |= sp.border_blocks(kind, bgx, bgy)[1]
        creach |= sp.border_blocks(kind, cgx, cgy)[1]
    band = built["centres"][built["kind"] == 1]
    assert set(zip(band[:, 3].tolist(), band[:, 4].tolist())) == set(zip(bgx[reach].tolist(), bgy[reach].tolist()))
    assert not creach.any()


def test_critical_pairs_are_the_tight_sqrt_cases():
    gx, gy = sp.critical_pairs()
    n = gx * gx + gy * gy
    k = np.rint(np.sqrt(n + 0.5)).astype(np.int64)
    assert gx.size == 1400 and set((n - k * k).tolist()) == {-1, 0} and k.min() > 1024
    assert sp.interior_reachable(gx, gy).sum() == 280


def test_gaussian_at_sigma_005_is_the_identity(built):
    """At sigma 0.05 the side taps underflow to 0: canny(plane, 0.05, ...) runs Sobel+NMS on the plane itself."""
    assert np.array_equal(oracle.gaussian_kernel(0.05), np.array([0, 1, 0], np.float32))
    for p in built["planes"]:
        assert np.array_equal(oracle.gaussian(p, 0.05), p.astype(np.int16))


def test_oracle_keeps_critical_centres_and_ties(built):
    """NMS can hide a centre: the oracle output must keep most critical-margin centres, or a layout change would
    quietly stop the GPU tests from observing them; the ramps must produce suppressed ties."""
    planes, c = built["planes"], built["centres"]
    kept = ties = 0
    for p in range(planes.shape[0]):
        mag, ang = oracle.sobel(planes[p].astype(np.int16))
        nm = oracle.nms(mag, ang)
        m = (c[:, 0] == p) & built["critical"]
        kept += int(np.count_nonzero(nm[c[m, 1], c[m, 2]]))
        r0 = planes.shape[1] - 2 - sp.RAMP_ROWS
        ramp_mag, ramp_nm = mag[r0 + 1:r0 + sp.RAMP_ROWS - 1, 3:-3], nm[r0 + 1:r0 + sp.RAMP_ROWS - 1, 3:-3]
        ties += int(np.count_nonzero((ramp_mag > 0) & (ramp_nm == 0)))
    assert int(built["critical"].sum()) == 280
    assert kept >= 270, kept
    assert ties >= 100000, ties
