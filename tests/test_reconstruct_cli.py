"""The -R grammar of Main (a bit map of the frame reconstructed on the GPU -> canny_reconstruct.pgm) without a GPU: a malformed
value, or seeded without -a fixed, is a usage error with exit status 2 before any device is touched; with fewer than three
positionals the usage text names the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "holes", "fill,", ",8", "fill,6", "fill,0", "fill,12", "fill,-8", "fill,8x", "fill, 8", "Fill",
                                   "FILL,8", "fill-holes", "8", "8,fill", "fill,8,100", "clear,4,0", "clear,,", "clear,four",
                                   "seeded", "seeded,8", "seeded,8,", "seeded,8,256", "seeded,8,-2", "seeded,8,1000", "seeded,8,1.5",
                                   "seeded,8,100,1", "seeded,,100", " seeded,8,100", "seeded,8,12x"])
def test_malformed_R_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a", "fixed,90", "-R", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -R expects op[,connectivity[,thr]]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_R_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-R")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -R expects op")


@pytest.mark.parametrize("binarize", [(), ("-a", "otsu"), ("-a", "mean,7,31")])
def test_seeded_without_a_fixed_binarization_is_a_usage_error(tmp_path, binarize):
    for args in (("-R", "seeded,8,170") + binarize, binarize + ("-R", "seeded,4,170")):
        r = run("1.0", "50", "150", "-o", str(tmp_path), *args)
        assert r.returncode == 2 and r.stderr.startswith("ERROR: -R seeded needs -a fixed"), r.stderr
        assert not list(tmp_path.iterdir()), "nothing was written"


def test_a_malformed_R_behind_a_well_formed_a_is_still_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a", "fixed,200", "-R", "flood")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -R expects op")


@pytest.mark.parametrize("value", ["fill", "clear", "fill,8", "fill,4", "clear,4", "clear,8", "seeded,8,170", "seeded,4,-1",
                                   "seeded,8,255", "seeded,8,007"])
def test_well_formed_R_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-a", "fixed,90", "-R", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-R op[,connectivity[,thr]]" in r.stderr and "canny_reconstruct.pgm" in r.stderr
    r = run("-R", value, "-a", "fixed,200", "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
