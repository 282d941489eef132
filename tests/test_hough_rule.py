"""Host-only checks of the Hough line feature (no GPU): the header declares, the library exports and capi binds every
entry point; canny_hip_hough_geometry / _tables / _line_of equal the numpy restatement of the rule (tests/hough_rule.py).
Geometry and line_of are exact.  The tables are the one non-exact check: numpy's and the C library's sin / cos may differ
in the last place of the double, so entries must agree to within one float ulp -- and be exactly reproducible."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import hough_rule as hr
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
NAMES = ("canny_hip_hough_geometry", "canny_hip_hough_tables", "canny_hip_hough_line_of", "canny_hip_dev_hough_points",
         "canny_hip_dev_hough_bits", "canny_hip_dev_canny_hough", "canny_hip_canny_hough", "canny_hip_hough_profile_get")
PI = float(np.pi)
RHOS = [0.5, 1.0, 2.0, 3.7]
THETAS = [PI / 90, PI / 180, PI / 360, 0.01]
RANGES = [(0.0, PI), (PI / 4, 3 * PI / 4), (0.3, 1.0)]
SHAPES = [(1, 1), (2, 2), (77, 77), (256, 256), (480, 640), (1080, 1920), (2160, 3840), (4320, 7680), (9, 4001)]


def test_every_entry_point_is_declared_exported_and_bound():
    lib = ctypes.CDLL(capi.LIB_PATH)
    L = capi.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", HEADER), f"{name} not declared in canny_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in capi.EXPORTS and getattr(L, name).argtypes is not None, f"{name} not bound by capi"
    for name in ("hough_geometry", "hough_tables", "hough_line_of"):
        assert callable(getattr(capi, name))
    for name in ("canny_hough", "dev_hough_points", "dev_hough_bits", "dev_canny_hough", "hough_profile_get"):
        assert callable(getattr(capi.Context, name))


def test_version_and_pinned_constants():
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", HEADER).group(1)) >= 600
    assert capi.load().canny_hip_version() >= 600
    assert int(re.search(r"CANNY_HIP_STAGE_END = (\d+)", HEADER).group(1)) == 10
    assert int(re.search(r"CANNY_HIP_STAGE_COUNT = (\d+)", HEADER).group(1)) == 9
    assert int(re.search(r"#define CANNY_HIP_HOUGH_MAX_LINES (\d+)", HEADER).group(1)) == capi.HOUGH_MAX_LINES == 4096


def test_geometry_of_a_4k_frame():
    assert capi.hough_geometry(2160, 3840, 1.0, PI / 180) == (180, 12001)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_equals_the_rule(shape):
    h, w = shape
    for rho, theta, (lo, hi) in itertools.product(RHOS, THETAS, RANGES):
        assert capi.hough_geometry(h, w, rho, theta, lo, hi) == hr.geometry(h, w, rho, theta, lo, hi), (rho, theta, lo, hi)


@pytest.mark.parametrize("rho,theta,lo,hi", [(r, t, lo, hi) for r in RHOS for t in THETAS for lo, hi in RANGES])
def test_tables_within_one_float_ulp_and_reproducible(rho, theta, lo, hi):
    numangle, _ = capi.hough_geometry(480, 640, rho, theta, lo, hi)
    tc, ts = capi.hough_tables(rho, theta, lo, numangle)
    tc2, ts2 = capi.hough_tables(rho, theta, lo, numangle)
    assert tc.dtype == np.float32 and tc.shape == (numangle,) and ts.shape == (numangle,)
    assert tc.tobytes() == tc2.tobytes() and ts.tobytes() == ts2.tobytes()
    wc, ws = hr.tables(rho, theta, lo, numangle)
    for got, want in ((tc, wc), (ts, ws)):
        ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp.astype(np.float64))


@pytest.mark.parametrize("rho,theta,lo", [(1.0, PI / 180, 0.0), (0.5, PI / 90, PI / 4), (3.7, 0.01, 0.3)])
def test_line_of_equals_the_float32_expression_for_every_base(rho, theta, lo):
    numangle, numrho = capi.hough_geometry(12, 17, rho, theta, lo, min(lo + 1.0, PI))
    bases = np.arange((numangle + 2) * (numrho + 2))
    want_rho, want_theta = hr.line_of(bases, numrho, rho, theta, lo)
    got = np.array([capi.hough_line_of(int(b), numrho, rho, theta, lo) for b in bases], np.float32)
    assert got[:, 0].tobytes() == want_rho.tobytes()
    assert got[:, 1].tobytes() == want_theta.tobytes()


BAD = [dict(rho=0.0), dict(rho=-1.0), dict(rho=float("nan")), dict(rho=float("inf")), dict(theta=0.0),
       dict(theta=-0.1), dict(theta=float("nan")), dict(theta=float("inf")), dict(min_theta=-0.1),
       dict(min_theta=1.0, max_theta=1.0), dict(min_theta=2.0, max_theta=1.0), dict(max_theta=3.2),
       dict(max_theta=float("nan")), dict(height=0), dict(width=0)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_geometry_rejects_invalid_arguments(bad):
    args = dict(height=480, width=640, rho=1.0, theta=PI / 180, min_theta=0.0, max_theta=PI)
    args.update(bad)
    with pytest.raises(capi.CannyHipError) as ei:
        capi.hough_geometry(**args)
    assert ei.value.status == 1  # CANNY_HIP_ERR_INVALID


def test_tables_and_line_of_reject_invalid_arguments():
    for rho, theta, lo, n in [(0.0, 0.1, 0.0, 4), (1.0, 0.0, 0.0, 4), (float("nan"), 0.1, 0.0, 4), (1.0, float("inf"), 0.0, 4),
                              (1.0, 0.1, -1.0, 4), (1.0, 0.1, 0.0, 0)]:
        with pytest.raises(capi.CannyHipError) as ei:
            capi.hough_tables(rho, theta, lo, n)
        assert ei.value.status == 1
    for numrho, rho, theta in [(0, 1.0, 0.1), (9, 0.0, 0.1), (9, 1.0, float("nan"))]:
        with pytest.raises(capi.CannyHipError) as ei:
            capi.hough_line_of(5, numrho, rho, theta)
        assert ei.value.status == 1
    L = capi.load()
    na = ctypes.c_int(0)
    assert L.canny_hip_hough_geometry(4, 4, 1.0, 0.1, 0.0, 1.0, ctypes.byref(na), None) == 1


def test_rule_helper_on_a_drawn_line():
    """The helper itself: a horizontal line of 40 pixels at row 7 gives its 40 votes to theta = pi/2, rho = 7."""
    h, w = 32, 48
    numangle, numrho = hr.geometry(h, w, 1.0, PI / 180)
    tc, ts = capi.hough_tables(1.0, PI / 180, 0.0, numangle)
    pts = 7 * w + np.arange(4, 44)
    acc = hr.accumulate(pts, w, numrho, tc, ts)
    assert acc.sum() == pts.size * numangle and acc.max() == 40
    ln, votes, bases, count = hr.lines(acc, 39, 7, 1.0, PI / 180)
    assert count >= 1 and votes[0] == 40 and ln[0, 0] == 7.0 and abs(ln[0, 1] - PI / 2) < 1e-6
    assert capi.hough_line_of(int(bases[0]), numrho, 1.0, PI / 180) == (ln[0, 0], ln[0, 1])
