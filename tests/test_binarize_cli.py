"""The -a grammar of Main (the input frame binarized -> canny_binary.pgm) without a GPU: a malformed value is a usage error
with exit status 2 before any device is touched; with fewer than three positionals the usage text names the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "otsu,", "Otsu", "sauvola", "fixed,256", "fixed,-2", "fixed,12x", "fixed, 12", "fixed,,3",
                                   "fixed,+5", "fixed,1000", "127,fixed", "mean,256", "mean,-256", "mean,7,4", "mean,7,1", "mean,7,257",
                                   "mean,7,31,2", "mean,7,31,31,2", "mean,7,31,31,-1", "mean,7,31,31,0,0", "mean,7,31,31,", "mean,7,,31",
                                   "mean,--7", "mean,-", "otsu,0,3,3,2", "otsu,x"])
def test_malformed_a_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -a expects method[,thr_or_c[,kw[,kh[,invert]]]]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_a_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -a expects method")


@pytest.mark.parametrize("value", ["fixed", "fixed,-1", "fixed,255,3,3,1", "otsu", "otsu,0,0,0,1", "mean", "mean,-255", "mean,7,3",
                                   "mean,0,255,3", "mean,255,31,31,1"])
def test_well_formed_a_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-a", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-a method[,thr_or_c[,kw[,kh[,invert]]]]" in r.stderr and "canny_binary.pgm" in r.stderr
    r = run("-a", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
