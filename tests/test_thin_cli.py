"""The -v grammar of Main (a bit map of the frame thinned on the GPU -> canny_thin.pgm) without a GPU: a malformed value is a
usage error with exit status 2 before any device is touched; with fewer than three positionals the usage text names the
option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "thin", "guohall,", ",3", "guohall,-1", "guohall,16385", "guohall,99999", "guohall,123456",
                                   "guohall,3x", "guohall, 3", "Guohall", "GUOHALL,3", "guo-hall", "3", "3,guohall", "guohall,3,4",
                                   "zhangsuen,,", "zhangsuen,one", "zhangsuen,1.5", "zhang-suen,2", " zhangsuen"])
def test_malformed_v_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-v", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -v expects method[,max_iterations]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_v_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-v")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -v expects method")


def test_a_malformed_v_behind_a_well_formed_a_is_still_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a", "fixed,200", "-v", "skeleton")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -v expects method")


@pytest.mark.parametrize("value", ["guohall", "zhangsuen", "guohall,0", "zhangsuen,1", "guohall,16384", "guohall,007"])
def test_well_formed_v_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-v", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-v method[,max_iterations]" in r.stderr and "canny_thin.pgm" in r.stderr
    r = run("-a", "fixed,200", "-v", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
