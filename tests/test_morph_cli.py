"""The -z grammar of Main (binary morphology of the edge map -> canny_morph.pgm) without a GPU: a malformed value is a usage
error with exit status 2 before any device is touched; with fewer than three positionals the usage text names the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "open", "open,", "open,4", "open,0", "open,33", "open,-3", "open,3x", "open, 3", "Open,3",
                                   "smooth,3", "3,open", "open,3,2", "open,3,,rect", "open,3,3,disk", "open,3,3,rect,0",
                                   "open,3,3,rect,17", "open,3,3,rect,1,1", "open,3,3,1", "open,3,3,rect,one", "open,3,3,rect,"])
def test_malformed_z_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-z", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -z expects op,kw[,kh[,shape[,iterations]]]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_z_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-z")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -z expects op,kw")


@pytest.mark.parametrize("value", ["erode,1", "dilate,3", "open,3,5", "close,31,1,rect", "gradient,5,5,cross", "tophat,7,7,ellipse,2",
                                   "blackhat,31,31,ellipse,16"])
def test_well_formed_z_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-z", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-z op,kw[,kh[,shape[,iterations]]]" in r.stderr and "canny_morph.pgm" in r.stderr
    r = run("-z", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
