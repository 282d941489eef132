"""The hysteresis sweeps place a tile (frame, tile row, tile column) with a multiply-high by a reciprocal the host prepares
(canny_edge_amd/csrc/canny_tile_div.h) instead of dividing.  Host only, no GPU: tests/cpp/test_tile_div.cpp includes the
header alone and compares quotient and remainder with / and % -- for every tile count per frame and per tile row up to 4096
(the tail route's limit) with every tile number of a 128-frame batch, and at the steps of the quotient over the whole int range."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reciprocal_division_equals_integer_division(tmp_path):
    exe = tmp_path / "test_tile_div"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "canny_edge_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_tile_div.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "tile_div ok" in r.stdout, r.stdout + r.stderr
