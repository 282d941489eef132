#!/usr/bin/env python3
"""Hough lines on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150, rho 1,
theta pi/180, threshold 270, lines_max 256), device resident: what the three parts of the transform cost behind
dev_canny, and the LDS-row vote against the global-atomic vote.

HIP-event times via hough_profile_get (0 vote, 1 peaks, 2 select), "profile_stage_mask" set to those three slots, in ONE
process: ROUNDS rounds of STEPS calls of dev_canny_hough after a warm-up, the variants alternating within each round.
Variants: "hough_path" 2 with the default LDS budget, with a 144 KiB budget (three rows of a 4K frame per workgroup, one
workgroup per CU), and "hough_path" 1.  Frame 0's lines are compared with the numpy rule (tests/hough_rule.py).
    python tools/probe_hough_lines.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
RHO, THETA, THRESHOLD, LINES_MAX = 1.0, float(np.pi / 180), 270, 256
ROUNDS, STEPS = 5, 3
VARIANTS = {"lds_rows": (2, 0), "lds_rows_144k": (2, 144), "global_atomics": (1, 0)}  # hough_path, tune_hough_lds_kb
PARTS = ("vote", "peaks", "select")


def main():
    import hough_rule as hr
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    slots = N * LINES_MAX
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_lines, d_votes, d_bases, d_counts = ctx.malloc(8 * slots), ctx.malloc(4 * slots), ctx.malloc(4 * slots), ctx.malloc(4 * N)
    ctx.h2d(d_in, frames)
    numangle, numrho = capi.hough_geometry(H, W, RHO, THETA)

    def call():
        ctx.dev_canny_hough(d_in, SIGMA, LO, HI, H, W, N, RHO, THETA, THRESHOLD, LINES_MAX, 0.0, float(np.pi), d_lines,
                            d_votes, d_bases, d_counts, 0, d_edges)

    def measure(variant):
        path, kb = VARIANTS[variant]
        ctx.set_option("hough_path", path)
        ctx.set_option("tune_hough_lds_kb", kb)
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0b111 << 10)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            call()
        ctx.synchronize()
        ms = [ctx.hough_profile_get(p)[0] / STEPS for p in range(3)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for v in VARIANTS:  # warm-up: workspaces, code objects, tables
        ctx.set_option("hough_path", VARIANTS[v][0])
        ctx.set_option("tune_hough_lds_kb", VARIANTS[v][1])
        call()
    per_round = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            per_round[v].append(measure(v))

    # the timed output is the right one: frame 0 against the rule applied to the s16 map of the same call
    ctx.set_option("hough_path", 0)
    ctx.set_option("tune_hough_lds_kb", 0)
    call()
    edges0 = np.empty((H, W), np.int16)
    ctx.d2h(edges0, d_edges)
    lines, votes = np.empty((slots, 2), np.float32), np.empty(slots, np.int32)
    bases, counts = np.empty(slots, np.uint32), np.empty(N, np.int32)
    for host, dev in ((lines, d_lines), (votes, d_votes), (bases, d_bases), (counts, d_counts)):
        ctx.d2h(host, dev)
    acc = hr.accumulate(np.flatnonzero(edges0), W, numrho, *capi.hough_tables(RHO, THETA, 0.0, numangle))
    wl, wv, wb, wc = hr.lines(acc, THRESHOLD, LINES_MAX, RHO, THETA)
    k = min(wc, LINES_MAX)
    same = bool(counts[0] == wc and np.array_equal(bases[:k], wb) and np.array_equal(votes[:k], wv) and
                lines[:k].tobytes() == wl.tobytes())
    # the batch's edge pixels, from the point lists' offsets
    d_off = ctx.malloc(8 * (N + 1))
    ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, 0, 0, d_off, d_edges)
    offsets = np.empty(N + 1, np.uint64)
    ctx.d2h(offsets, d_off)
    edge_px = int(offsets[-1])
    n_votes = edge_px * numangle

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rho": RHO,
              "theta": THETA, "threshold": THRESHOLD, "lines_max": LINES_MAX, "numangle": numangle, "numrho": numrho,
              "rounds": ROUNDS, "steps": STEPS, "host": socket.gethostname(), "edge_pixels": edge_px, "votes": n_votes,
              "peaks_frame0": int(counts[0]), "peaks_total": int(counts.sum()), "lines_equal_numpy_rule": same}
    for v, rounds in per_round.items():
        for i, part in enumerate(PARTS):
            vals = [r[i] for r in rounds]
            result[f"{v}_{part}_ms"] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4),
                                        "max": round(max(vals), 4)}
        result[f"{v}_votes_per_second"] = round(n_votes / (result[f"{v}_vote_ms"]["median"] * 1e-3), 0)
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_lines, d_votes, d_bases, d_counts, d_off):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's lines differ from the numpy rule")


if __name__ == "__main__":
    main()
