"""The -q grammar of Main (corners of the smoothed plane -> canny_corners.txt) without a GPU: a malformed value is a usage
error with exit status 2 before any device is touched; with fewer than three positionals the usage text names the option."""
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
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 1900
    assert capi.load().canny_hip_version() >= 1900


@pytest.mark.parametrize("value", ["", "655", "655,5", "655,5,", ",5,100", "655,,100", "655,5,100,", "655,5,100,3,10,1",
                                   "655,5,0", "655,5,4097", "655,5,100,4", "655,5,100,9", "655,5,100,3,65", "65537,5,100",
                                   "-1,5,100", "655,-5,100", "655,5,100,3,-1", "6.5,5,100", "655,5,100x", " 655,5,100",
                                   "655,5, 100", "a,b,c"])
def test_malformed_q_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-q", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -q expects quality_q16,min_dist,corners_max[,block[,k_q8]]")
    assert not list(tmp_path.iterdir()), "nothing was written"


@pytest.mark.parametrize("value", ["655,5,100", "0,0,1", "65536,0,4096,7", "655,5,100,5,0", "655,5,100,3,64"])
def test_well_formed_q_passes_the_grammar(tmp_path, value):
    """With fewer than three positionals the usage text is printed and the program exits 0 before any device is touched,
    as for every other flag; a threshold error behind a well-formed -q is the reference's (exit 0)."""
    r = run("1.0", "50", "-q", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-q quality_q16,min_dist,corners_max[,block[,k_q8]]" in r.stderr and "canny_corners.txt" in r.stderr
    r = run("-q", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
