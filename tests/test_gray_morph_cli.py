"""The -G grammar of Main (a grey-level operator on the input frame on the GPU -> canny_gray.pgm) without a GPU: a malformed
value is a usage error with exit status 2 before any device is touched; with fewer than three positionals the usage text
names the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "erode", "erode,", ",3", "erode,2", "erode,0", "erode,33", "erode,-3", "erode,3x", "erode, 3",
                                   "Erode,3", "ERODE,3", "erosion,3", "3", "3,erode", "erode,3,4", "erode,3,,rect", "erode,3,3,disk",
                                   "erode,3,3,rect,0", "erode,3,3,rect,17", "erode,3,3,rect,1,", "erode,3,3,rect,1,256",
                                   "erode,3,3,rect,1,-1", "erode,3,3,rect,1,constant", "erode,3,3,rect,1,Neutral", "erode,3,3,rect,1,1000",
                                   "erode,3,3,rect,1,1.5", "erode,3,3,rect,1,0,0", "erode,3,3,rect,1,neutral,", " erode,3", "erode,003",
                                   "median,7", "median,3,5", "median,5,3", "median,1", "median,3,3,cross", "median,3,3,ellipse",
                                   "median,3,3,rect,1,neutral", "median,3,3,rect,0", "median,4"])
def test_malformed_G_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-G", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -G expects op,kw[,kh[,shape[,iterations[,border]]]]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_G_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-G")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -G expects op")


def test_a_malformed_G_behind_a_well_formed_a_is_still_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-a", "otsu", "-G", "blackhat")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -G expects op")


@pytest.mark.parametrize("value", ["erode,3", "dilate,31", "open,5,3", "close,3,5,cross", "gradient,7,7,ellipse,2", "tophat,15,15,rect,1,neutral",
                                   "blackhat,15,15,rect,16,replicate", "erode,3,3,rect,1,0", "erode,3,3,rect,1,255", "dilate,1,1,rect,1,077",
                                   "median,3", "median,5", "median,5,5", "median,3,3,rect,2", "median,3,3,rect,16,replicate",
                                   "median,5,5,rect,1,128", "erode,03"])
def test_well_formed_G_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-a", "otsu", "-G", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-G op,kw[,kh[,shape[,iterations[,border]]]]" in r.stderr and "canny_gray.pgm" in r.stderr
    assert "canny_gray_binary.pgm" in r.stderr
    r = run("-G", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
