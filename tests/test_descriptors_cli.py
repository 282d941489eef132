"""The -j grammar of Main (descriptors of the corners of -q -> canny_descriptors.txt) without a GPU: a malformed value, or -j
without -q, is a usage error with exit status 2 before any device is touched; with fewer than three positionals the usage
text names the option.  (-b is Main's batch directory, so the descriptors took the next free letter.)"""
import os
import re

import subprocess

import pytest

from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_version():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2000
    assert capi.load().canny_hip_version() >= 2000


@pytest.mark.parametrize("value", ["", "steer", "Steered", "1", "steered,1", " upright", "upright ", "-q"])
def test_malformed_j_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-q", "655,5,100", "-j", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -j expects upright or steered")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_j_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-q", "655,5,100", "-j")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -j expects upright or steered")


@pytest.mark.parametrize("value", ["upright", "steered"])
def test_j_without_q_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-j", value)
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -j needs the corners of -q"), r.stderr
    assert not list(tmp_path.iterdir()), "nothing was written"


@pytest.mark.parametrize("value", ["upright", "steered"])
def test_well_formed_j_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-q", "655,5,100", "-j", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-j upright|steered" in r.stderr and "canny_descriptors.txt" in r.stderr
    r = run("-j", value, "-q", "655,5,100", "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
