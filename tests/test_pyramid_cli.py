"""The -P grammar of Main (the pyramid of the input frame on the GPU -> canny_pyr1.pgm ..) without a GPU: a malformed value is
a usage error with exit status 2 before any device is touched; with fewer than three positionals the usage text names the
option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "canny_edge_amd", "Main")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["", "0", "16", "99", "100", "-1", "+3", "3.0", "3x", " 3", "3 ", "three", "up", ",up", "3,", "3,down",
                                   "3,UP", "3,Up", "3,up,", "3,up,up", "3,,up", "3, up", "up,3", "0,up", "16,up", "0x3", "1e1", "3;up"])
def test_malformed_P_is_a_usage_error(tmp_path, value):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-P", value)
    assert r.returncode == 2, (value, r.stdout, r.stderr)
    assert r.stderr.startswith("ERROR: -P expects levels[,up]")
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_P_as_the_last_word_is_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-P")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -P expects levels")


def test_a_malformed_P_behind_a_well_formed_G_is_still_a_usage_error(tmp_path):
    r = run("1.0", "50", "150", "-o", str(tmp_path), "-G", "median,3", "-P", "up")
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -P expects levels")


@pytest.mark.parametrize("value", ["1", "3", "9", "15", "03", "1,up", "3,up", "15,up", "07,up"])
def test_well_formed_P_passes_the_grammar(tmp_path, value):
    r = run("1.0", "50", "-P", value, "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("USAGE:")
    assert "-P levels[,up]" in r.stderr and "canny_pyr1.pgm" in r.stderr and "canny_pyr_up.pgm" in r.stderr
    r = run("-P", value, "1.0", "150", "50", "-o", str(tmp_path))
    assert r.returncode == 0 and r.stderr.startswith("ERROR: minVal must be less than maxVal")
    assert not list(tmp_path.iterdir()), "nothing was written"
