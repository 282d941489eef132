#!/usr/bin/env python3
"""The distance transform on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device
resident: what its two parts cost behind dev_canny for three sets of outputs -- dist2 only, dist
only, all three planes.

HIP-event times via edt_profile_get (0 rows, 1 columns), "profile_stage_mask" set to those two slots, in ONE process:
ROUNDS rounds of STEPS calls of dev_canny_edt after a warm-up, the variants alternating within each round.  Yardsticks from
the same process: dev_canny alone (host clock around STEPS calls that end in a synchronise) and, per variant,
canny_hip_probe_copy of half the bytes the variant necessarily moves -- its output planes plus the u16 plane written and
read once; a copy of X bytes reads X and writes X, the way bench.py --full prices its copy probe.  One host time of
scipy.ndimage.distance_transform_edt on frame 0's map for context.  Frame 0's planes are compared with scipy (dist2, dist)
and the numpy rule (nearest, tests/edt_rule.py) on the s16 map of the same call.
    python tools/probe_edt.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
ROUNDS, STEPS = 5, 3
VARIANTS = {"dist2": (True, False, False), "dist": (False, True, False), "all": (True, True, True)}
PARTS = ("rows", "columns")


def _stat(vals):
    return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}


def main():
    import edt_rule as rule
    from scipy import ndimage
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_planes = [ctx.malloc(px * 4) for _ in range(3)]
    d_copy_src, d_copy_dst = ctx.malloc(px * 8), ctx.malloc(px * 8)
    ctx.h2d(d_in, frames)

    def call(variant):
        ptrs = [p if asked else 0 for p, asked in zip(d_planes, VARIANTS[variant])]
        ctx.dev_canny_edt(d_in, SIGMA, LO, HI, H, W, N, *ptrs, d_edges)

    def measure(variant):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0b11 << 17)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            call(variant)
        ctx.synchronize()
        ms = [ctx.edt_profile_get(p)[0] / STEPS for p in range(2)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    def canny_ms():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            ctx.dev_canny(d_in, SIGMA, LO, HI, H, W, N, d_edges)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / STEPS

    def moved_bytes(variant):   # outputs + the u16 plane written by the row pass and read by the column pass
        return px * (4 * sum(VARIANTS[variant]) + 2 + 2)

    for v in VARIANTS:  # warm-up: workspaces, code objects
        call(v)
    canny_ms()
    per_round = {v: [] for v in VARIANTS}
    copies = {v: [] for v in VARIANTS}
    canny = []
    for _ in range(ROUNDS):
        for v in VARIANTS:
            per_round[v].append(measure(v))
            copies[v].append(ctx.probe_copy(d_copy_src, d_copy_dst, (moved_bytes(v) // 2) & ~15, 5))
        canny.append(canny_ms())

    # the timed output is the right one: frame 0 against scipy and the rule on the s16 map of the same call
    call("all")
    edges0 = np.empty((H, W), np.int16)
    ctx.d2h(edges0, d_edges)
    got = [np.empty((H, W), dt) for dt in (np.int32, np.float32, np.int32)]
    for a, p in zip(got, d_planes):
        ctx.d2h(a, p)
    mask = edges0 != 0
    t0 = time.perf_counter()
    e = ndimage.distance_transform_edt(~mask)
    scipy_s = time.perf_counter() - t0
    want_d2, want_nn = rule.separable(mask)
    same = bool(np.array_equal(got[0], np.rint(e * e).astype(np.int32)) and np.array_equal(got[0], want_d2)
                and got[1].tobytes() == e.astype(np.float32).tobytes() and np.array_equal(got[2], want_nn))

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(), "edge_pixels_frame0": int(mask.sum()),
              "max_dist_frame0": round(float(got[1].max()), 2), "frame0_equals_scipy_and_rule": same,
              "dev_canny_alone_ms": _stat(canny), "scipy_one_frame_s": round(scipy_s, 3)}
    for v, rounds in per_round.items():
        for i, part in enumerate(PARTS):
            result[f"{v}_{part}_ms"] = _stat([r[i] for r in rounds])
        result[f"{v}_total_ms"] = round(sum(result[f"{v}_{p}_ms"]["median"] for p in PARTS), 4)
        result[f"{v}_moved_bytes"] = moved_bytes(v)
        result[f"{v}_copy_ms"] = _stat(copies[v])
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in [d_in, d_edges, d_copy_src, d_copy_dst] + d_planes:
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's planes differ from scipy / the numpy rule")


if __name__ == "__main__":
    main()
