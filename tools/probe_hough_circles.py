#!/usr/bin/env python3
"""Hough circles on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150, radii 10..100,
threshold 30, support threshold 20, min_dist 10, centres_max 256), device resident: what the four parts of the transform
cost behind dev_canny, with cells of one and of two pixels.

HIP-event times via hough_circles_profile_get (0 vote, 1 centres, 2 radius, 3 accept), "profile_stage_mask" set to those
four slots, in ONE process: ROUNDS rounds of STEPS calls of dev_canny_hough_circles after a warm-up call per variant, the
variants alternating within each round.  The votes cast are the sums of the accumulators of the 16 distinct frames of the
batch (times 8); frame 0's accumulator and circles are compared with the numpy rule (tests/hough_circles_rule.py) fed with
the map of the same call and the oracle's Sobel of the oracle's smoothed plane.
    python tools/probe_hough_circles.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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

N, H, W, DISTINCT = 128, 2160, 3840, 16
SIGMA, LO, HI = 1.4, 50, 150
MIN_R, MAX_R, THRESHOLD, SUPPORT, MIN_DIST, CENTRES_MAX = 10, 100, 30, 20, 10, 256
ROUNDS, STEPS = 5, 3
VARIANTS = {"cell1": 0, "cell2": 1}  # cell_shift
PARTS = ("vote", "centres", "radius", "accept")


def main():
    import hough_circles_rule as cr
    import oracle
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=DISTINCT)
    slots = N * CENTRES_MAX
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_rec, d_counts, d_peaks = ctx.malloc(24 * slots), ctx.malloc(4 * N), ctx.malloc(4 * N)
    ctx.h2d(d_in, frames)

    def call(shift, d_accum=0):
        ctx.dev_canny_hough_circles(d_in, SIGMA, LO, HI, H, W, N, MIN_R, MAX_R, shift, THRESHOLD, SUPPORT, MIN_DIST,
                                    CENTRES_MAX, d_rec, d_counts, d_peaks, d_accum, d_edges)

    def measure(shift):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0b1111 << 26)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            call(shift)
        ctx.synchronize()
        ms = [ctx.hough_circles_profile_get(p)[0] / STEPS for p in range(4)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for shift in VARIANTS.values():  # warm-up: workspaces, code objects
        call(shift)
    per_round = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v, shift in VARIANTS.items():
            per_round[v].append(measure(shift))

    # the batch's edge pixels, from the point lists' offsets
    d_off = ctx.malloc(8 * (N + 1))
    ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, 0, 0, d_off, d_edges)
    offsets = np.empty(N + 1, np.uint64)
    ctx.d2h(offsets, d_off)
    edge_px = int(offsets[-1])
    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "radii": [MIN_R, MAX_R],
              "threshold": THRESHOLD, "support_threshold": SUPPORT, "min_dist": MIN_DIST, "centres_max": CENTRES_MAX,
              "rounds": ROUNDS, "steps": STEPS, "host": socket.gethostname(), "edge_pixels": edge_px,
              "smoothed_u8": ctx.get_option("last_canny_smoothed_u8")}

    # the timed output is the right one: the votes cast, and frame 0 against the rule
    sm0 = oracle.gaussian(frames[0], SIGMA)
    gx0, gy0 = cr.sobel(sm0)
    same_all = True
    for v, shift in VARIANTS.items():
        c = 1 << shift
        cells = ((H + c - 1) // c + 2) * ((W + c - 1) // c + 2)
        d_accum = ctx.malloc(4 * cells * N)
        call(shift, d_accum)
        acc = np.empty((DISTINCT, (H + c - 1) // c + 2, (W + c - 1) // c + 2), np.int32)
        ctx.d2h(acc, d_accum)
        ctx.free(d_accum)
        n_votes = int(acc.sum(dtype=np.int64)) * (N // DISTINCT)
        edges0 = np.empty((H, W), np.int16)
        ctx.d2h(edges0, d_edges)
        rec, counts, peaks = np.empty((N, CENTRES_MAX, 6), np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
        for host, dev in ((rec, d_rec), (counts, d_counts), (peaks, d_peaks)):
            ctx.d2h(host, dev)
        want_acc = cr.accumulate(edges0 != 0, gx0, gy0, MIN_R, MAX_R, shift)
        want, n_peaks = cr.circles(edges0 != 0, want_acc, MIN_R, MAX_R, shift, THRESHOLD, SUPPORT, MIN_DIST, CENTRES_MAX)
        same = bool(np.array_equal(acc[0], want_acc) and counts[0] == len(want) and peaks[0] == n_peaks and
                    np.array_equal(rec[0, :len(want)], want))
        same_all &= same
        result[f"{v}_votes"] = n_votes
        result[f"{v}_max_cell_votes"] = int(acc.max())
        result[f"{v}_peaks_frame0"] = int(peaks[0])
        result[f"{v}_circles_frame0"] = int(counts[0])
        result[f"{v}_circles_total"] = int(counts.sum())
        result[f"{v}_frame0_equal_numpy_rule"] = same
        for i, part in enumerate(PARTS):
            vals = [r[i] for r in per_round[v]]
            result[f"{v}_{part}_ms"] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4),
                                        "max": round(max(vals), 4)}
        result[f"{v}_votes_per_second"] = round(n_votes / (result[f"{v}_vote_ms"]["median"] * 1e-3), 0)
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_rec, d_counts, d_peaks, d_off):
        ctx.free(p)
    if not same_all:
        raise SystemExit("frame 0's accumulator or circles differ from the numpy rule")


if __name__ == "__main__":
    main()
