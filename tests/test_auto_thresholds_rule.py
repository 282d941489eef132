"""CPU-only checks of the automatic per-frame threshold rule: the host export
canny_hip_auto_thresholds_from_histogram -- the same __host__ __device__ function the GPU select kernel runs -- against a
numpy restatement of the rule, its argument checks, and the header's constants.  No kernel is launched here."""
import math
import os
import re

import numpy as np
import pytest

from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "canny_hip.h")).read()


def np_quantile(hist, q):
    """Inverted-CDF quantile: min { b : h[0] + ... + h[b] >= max(1, ceil(q * N)) }, q a float32 widened to double."""
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64))
    need = max(1, math.ceil(float(np.float32(q)) * float(int(cum[-1]))))
    return int(np.searchsorted(cum, need, side="left"))


def np_rule(hist, rule, low, high):
    if rule == capi.AUTO_MEDIAN:
        m = np_quantile(hist, 0.5)
        lo = math.floor(float(np.float32(low)) * m)
        hi = math.floor(float(np.float32(high)) * m)
    else:
        lo, hi = np_quantile(hist, low), np_quantile(hist, high)
    lo = min(max(lo, 1), 255)
    hi = min(max(hi, lo), 255)
    return lo, hi


def _random_hist(rng):
    kind = rng.integers(0, 5)
    h = np.zeros(257, np.uint32)
    if kind == 0:  # dense
        h[:] = rng.integers(0, 1000, 257)
    elif kind == 1:  # a few occupied bins
        idx = rng.integers(0, 257, rng.integers(1, 6))
        h[idx] = rng.integers(1, 10**6, idx.size)
    elif kind == 2:  # an image-like intensity histogram
        v = np.clip(rng.normal(rng.uniform(0, 255), rng.uniform(1, 60), rng.integers(1, 5000)), 0, 255).astype(int)
        h[:256] = np.bincount(v, minlength=256)
    elif kind == 3:  # a gradient-like histogram: mass near 0, a long tail, clamped at 256
        v = np.minimum(rng.exponential(rng.uniform(1, 200), rng.integers(1, 5000)).astype(int), 256)
        h[:] = np.bincount(v, minlength=257)
    else:  # large counts (a 4K frame has 8.3 M pixels)
        h[:] = rng.integers(0, 2**24, 257)
    if h.sum() == 0:
        h[rng.integers(0, 257)] = 1
    return h


def _check(h, rule, low, high):
    got = capi.auto_thresholds_from_histogram(h, rule, low, high)
    assert got == np_rule(h, rule, low, high), (rule, low, high, np.nonzero(h)[0][:10])
    lo, hi = got
    assert 1 <= lo <= hi <= 255
    return got


def test_rule_matches_numpy_on_random_histograms():
    rng = np.random.default_rng(400)
    for _ in range(3000):
        h = _random_hist(rng)
        if rng.integers(0, 2):
            low = float(rng.uniform(0, 1.5))
            _check(h, capi.AUTO_MEDIAN, low, low + float(rng.uniform(0, 3)))
        else:
            lo = float(rng.uniform(1e-6, 1))
            _check(h, capi.AUTO_QUANTILE, lo, float(rng.uniform(lo, 1)))


@pytest.mark.parametrize("rule,low,high", [(capi.AUTO_MEDIAN, 0.67, 1.33), (capi.AUTO_MEDIAN, 0.0, 0.0),
                                           (capi.AUTO_MEDIAN, 1.0, 1.0), (capi.AUTO_MEDIAN, 2.0, 300.0),
                                           (capi.AUTO_QUANTILE, 0.7, 0.9), (capi.AUTO_QUANTILE, 1.0, 1.0),
                                           (capi.AUTO_QUANTILE, 1e-9, 1e-9), (capi.AUTO_QUANTILE, 0.5, 0.5),
                                           (capi.AUTO_QUANTILE, 1e-9, 1.0)])
@pytest.mark.parametrize("case", ["n1_mid", "n1_zero", "one_bin", "bin256_only", "zero_median", "high_median",
                                  "two_bins"])
def test_rule_edge_cases(case, rule, low, high):
    h = np.zeros(257, np.uint32)
    if case == "n1_mid":
        h[77] = 1
    elif case == "n1_zero":
        h[0] = 1
    elif case == "one_bin":
        h[200] = 8294400
    elif case == "bin256_only":
        h[256] = 12345
    elif case == "zero_median":  # m = 0: the median rule gives (0, 0) before the clamp
        h[0], h[100] = 10, 3
    elif case == "high_median":  # factors push past 255
        h[250], h[255] = 5, 5
    else:
        h[3], h[250] = 1, 1
    _check(h, rule, low, high)


def test_rule_known_values():
    h = np.zeros(257, np.uint32)
    h[0] = 1000  # a black frame
    assert capi.auto_thresholds_from_histogram(h, "median", 0.67, 1.33) == (1, 1)
    assert capi.auto_thresholds_from_histogram(h, "quantile", 0.7, 0.9) == (1, 1)
    h[:] = 0
    h[100] = 1  # N = 1, m = 100
    assert capi.auto_thresholds_from_histogram(h, "median", 0.67, 1.33) == (67, 133)
    assert capi.auto_thresholds_from_histogram(h, "median", 2.0, 3.0) == (200, 255)
    assert capi.auto_thresholds_from_histogram(h, "median", 3.0, 3.0) == (255, 255)
    h[:] = 0
    h[10], h[20], h[30], h[40] = 1, 1, 1, 1  # quantiles: ceil(q * 4) -th sample
    assert capi.auto_thresholds_from_histogram(h, "quantile", 0.25, 0.5) == (10, 20)
    assert capi.auto_thresholds_from_histogram(h, "quantile", 0.26, 1.0) == (20, 40)
    h[:] = 0
    h[256] = 7  # magnitudes of 256 and more: clamped to 255
    assert capi.auto_thresholds_from_histogram(h, "quantile", 0.1, 0.9) == (255, 255)


@pytest.mark.parametrize("rule,low,high", [
    (0, 0.5, 1.0), (3, 0.5, 1.0), (-1, 0.5, 1.0),
    (capi.AUTO_MEDIAN, -0.1, 1.0), (capi.AUTO_MEDIAN, 1.2, 1.0), (capi.AUTO_MEDIAN, float("nan"), 1.0),
    (capi.AUTO_MEDIAN, 0.5, float("nan")), (capi.AUTO_MEDIAN, 0.5, float("inf")),
    (capi.AUTO_QUANTILE, 0.0, 0.5), (capi.AUTO_QUANTILE, 0.5, 1.01), (capi.AUTO_QUANTILE, 0.9, 0.5),
    (capi.AUTO_QUANTILE, -0.5, 0.5), (capi.AUTO_QUANTILE, float("nan"), 0.5), (capi.AUTO_QUANTILE, 0.5, float("nan")),
])
def test_rule_rejects_bad_arguments(rule, low, high):
    h = np.ones(257, np.uint32)
    with pytest.raises(capi.CannyHipError) as ei:
        capi.auto_thresholds_from_histogram(h, rule, low, high)
    assert ei.value.status == 1  # CANNY_HIP_ERR_INVALID


def test_rule_rejects_empty_histogram():
    with pytest.raises(capi.CannyHipError) as ei:
        capi.auto_thresholds_from_histogram(np.zeros(257, np.uint32), "median", 0.67, 1.33)
    assert ei.value.status == 1


def test_python_rule_names():
    with pytest.raises(ValueError):
        capi.auto_thresholds_from_histogram(np.ones(257, np.uint32), "mean")
    with pytest.raises(ValueError):
        capi.auto_thresholds_from_histogram(np.ones(256, np.uint32), "median")


def test_header_constants_and_version():
    assert int(re.search(r"\bCANNY_HIP_AUTO_MEDIAN\s*=\s*(\d+)", HEADER).group(1)) == capi.AUTO_MEDIAN == 1
    assert int(re.search(r"\bCANNY_HIP_AUTO_QUANTILE\s*=\s*(\d+)", HEADER).group(1)) == capi.AUTO_QUANTILE == 2
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", HEADER).group(1)) >= 400
    assert capi.load().canny_hip_version() >= 400
    for name in ("canny_hip_auto_thresholds_from_histogram", "canny_hip_dev_canny_thresholds",
                 "canny_hip_dev_canny_auto", "canny_hip_canny_batch_thresholds", "canny_hip_canny_batch_auto"):
        assert name in capi.EXPORTS and re.search(r"\b%s\s*\(" % name, HEADER)
