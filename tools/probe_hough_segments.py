#!/usr/bin/env python3
"""Hough line segments on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150, rho 1,
theta pi/180, threshold 270, lines_max 256; min_length 30, max_gap 10, segments_max 4096), device resident: what the
segments add to a Hough call behind dev_canny.

HIP-event times via hough_segments_profile_get (0 count, 1 emit, 2 exclusive) and hough_profile_get (0 vote, 1 peaks,
2 select), "profile_stage_mask" set to those six slots, in ONE process: ROUNDS rounds of STEPS calls of
dev_canny_hough_segments after a warm-up, the two modes alternating within each round.  Frame 0's segments of both modes
are compared with the library's host walk of the rule (hough_segments_from_bits) on the s16 map of the same call.
    python tools/probe_hough_segments.py [out.jsonl]   (one JSON line per mode; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
RHO, THETA, THRESHOLD, LINES_MAX = 1.0, float(np.pi / 180), 270, 256
MIN_LENGTH, MAX_GAP, SEGMENTS_MAX = 30, 10, 4096
ROUNDS, STEPS = 5, 3
MODES = {"non_exclusive": 0, "exclusive": 1}
HOUGH_PARTS = ("vote", "peaks", "select")
SEGMENT_PARTS = ("count", "emit", "exclusive")


def main():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    slots = N * LINES_MAX
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_bases, d_counts = ctx.malloc(4 * slots), ctx.malloc(4 * N)
    d_seg, d_seg_counts = ctx.malloc(4 * 6 * N * SEGMENTS_MAX), ctx.malloc(4 * N)
    ctx.h2d(d_in, frames)

    def call(exclusive):
        ctx.dev_canny_hough_segments(d_in, SIGMA, LO, HI, H, W, N, RHO, THETA, THRESHOLD, LINES_MAX, 0.0, float(np.pi),
                                     MIN_LENGTH, MAX_GAP, exclusive, d_seg, SEGMENTS_MAX, d_seg_counts, d_bases=d_bases,
                                     d_line_counts=d_counts, d_edges=d_edges)

    def measure(exclusive):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", (0b111 << 10) | (0b111 << 19))
        ctx.profile_enable(True)
        for _ in range(STEPS):
            call(exclusive)
        ctx.synchronize()
        ms = [ctx.hough_profile_get(p)[0] / STEPS for p in range(3)]
        ms += [ctx.hough_segments_profile_get(p)[0] / STEPS for p in range(3)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for exclusive in MODES.values():  # warm-up: workspaces, code objects, tables
        call(exclusive)
    per_round = {m: [] for m in MODES}
    for _ in range(ROUNDS):
        for m, exclusive in MODES.items():
            per_round[m].append(measure(exclusive))

    lines = []
    all_same = True
    for m, exclusive in MODES.items():
        # the timed output is the right one: frame 0 against the host walk of the rule on the s16 map of the same call
        call(exclusive)
        edges0 = np.empty((H, W), np.int16)
        ctx.d2h(edges0, d_edges)
        bases, counts = np.empty(slots, np.uint32), np.empty(N, np.int32)
        seg, seg_counts = np.empty((N, SEGMENTS_MAX, 6), np.int32), np.empty(N, np.int32)
        for host, dev in ((bases, d_bases), (counts, d_counts), (seg, d_seg), (seg_counts, d_seg_counts)):
            ctx.d2h(host, dev)
        k = min(int(counts[0]), LINES_MAX)
        want, total = capi.hough_segments_from_bits(np.packbits(edges0 != 0, axis=-1), H, W, bases[:k], RHO, THETA, 0.0,
                                                    float(np.pi), MIN_LENGTH, MAX_GAP, exclusive, segments_max=SEGMENTS_MAX)
        same = bool(total == seg_counts[0] and np.array_equal(want, seg[0, :len(want)]))
        all_same &= same
        result = {"mode": m, "frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rho": RHO,
                  "theta": THETA, "threshold": THRESHOLD, "lines_max": LINES_MAX, "min_length": MIN_LENGTH,
                  "max_gap": MAX_GAP, "segments_max": SEGMENTS_MAX, "rounds": ROUNDS, "steps": STEPS,
                  "host": socket.gethostname(), "lines_total": int(np.minimum(counts, LINES_MAX).sum()),
                  "segments_frame0": int(seg_counts[0]), "segments_total": int(seg_counts.sum()),
                  "frame0_equals_host_walk": same}
        for i, part in enumerate(HOUGH_PARTS + tuple("segments_" + p for p in SEGMENT_PARTS)):
            vals = [r[i] for r in per_round[m]]
            result[f"{part}_ms"] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4),
                                    "max": round(max(vals), 4)}
        lines.append(json.dumps(result))
    for line in lines:
        print(line)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    for p in (d_in, d_edges, d_bases, d_counts, d_seg, d_seg_counts):
        ctx.free(p)
    if not all_same:
        raise SystemExit("frame 0's segments differ from the host walk of the rule")


if __name__ == "__main__":
    main()
