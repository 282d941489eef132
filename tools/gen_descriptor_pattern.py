#!/usr/bin/env python3
"""Writes canny_edge_amd/csrc/canny_desc_pattern.h: the 32 x 256 x 4 signed bytes (ax, ay, bx, by) of the descriptor
pattern in every rotation, from the generator of tests/descriptors_rule.py.  The header holds only the numbers; the file
that includes it wraps them in an array.  tests/test_descriptors_rule.py checks the committed header against the
generator."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import descriptors_rule as dr  # noqa: E402


def text() -> str:
    pat = dr.pattern()
    lines = ["/* canny_desc_pattern.h -- the descriptor pattern (include/canny_hip.h, DESIGN.md section 30): ax, ay, bx, by of",
             " * test t in rotation k at [(k * 256 + t) * 4 ..], 32 x 256 x 4 signed bytes.  Written by",
             " * tools/gen_descriptor_pattern.py; data only -- include it between the braces of an array. */"]
    for k in range(dr.DESC_ROTATIONS):
        lines.append(f"/* rotation {k} */")
        for t0 in range(0, dr.DESC_BITS, 8):
            lines.append(" ".join("%d,%d,%d,%d," % tuple(pat[k, t]) for t in range(t0, t0 + 8)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    path = os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_desc_pattern.h")
    with open(path, "w") as f:
        f.write(text())
    print("wrote", path)
