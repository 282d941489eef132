#!/usr/bin/env python3
"""Sub-pixel line fits on the Hough segments' own workload (DESIGN.md sections 16 and 24): 128 x 3840x2160 synth_batch, sigma
1.4, thresholds 50 / 150, rho 1, theta pi / 180, Hough threshold 270, lines_max 256, min_length 30, max_gap 10, segments_max
4096, device resident.

  count, emit  the two parts of the non-exclusive segments (every line walked twice), per call
  fit          the one part of the line fits behind them (canny_hip_line_fits_profile_get), per call

All are HIP-event times of the SAME calls in one process, ROUNDS rounds of STEPS calls after a warm-up; medians and ranges
over the rounds.  Frame 0's fits are compared with the host rule on the same call's map and smoothed plane.
    python tools/probe_line_fits.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
RHO, THETA, THRESHOLD, LINES_MAX = 1.0, float(np.pi / 180), 270, 256
MIN_LENGTH, MAX_GAP, SEGMENTS_MAX = 30, 10, 4096
ROUNDS, STEPS = 5, 5


def main():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_bases, d_lc = ctx.malloc(4 * N * LINES_MAX), ctx.malloc(4 * N)
    d_seg, d_sc = ctx.malloc(4 * 6 * N * SEGMENTS_MAX), ctx.malloc(4 * N)
    d_fit = ctx.malloc(4 * 12 * N * SEGMENTS_MAX)
    ctx.h2d(d_in, frames)
    options = 0

    def fits():
        ctx.dev_canny_hough_line_fits(d_in, SIGMA, LO, HI, H, W, N, RHO, THETA, THRESHOLD, LINES_MAX, 0.0, float(np.pi),
                                      MIN_LENGTH, MAX_GAP, 0, d_seg, SEGMENTS_MAX, d_sc, options, d_fit, d_bases=d_bases,
                                      d_line_counts=d_lc, d_edges=d_edges)

    for _ in range(2):  # warm-up: workspaces, code objects
        fits()
    rounds = []
    for _ in range(ROUNDS):
        row = {}
        for options in (0, 3):
            ctx.synchronize()
            ctx.profile_reset()
            ctx.set_option("profile_stage_mask", (1 << 19) | (1 << 20) | (1 << 30))
            ctx.profile_enable(True)
            for _ in range(STEPS):
                fits()
            ctx.synchronize()
            cnt, emit = (ctx.hough_segments_profile_get(p)[0] / STEPS for p in (0, 1))
            fit = ctx.line_fits_profile_get(capi.LINE_FIT_PART_FIT)[0] / STEPS
            ctx.profile_enable(False)
            ctx.set_option("profile_stage_mask", 0)
            if options == 0:
                row.update({"count_ms": round(cnt, 4), "emit_ms": round(emit, 4), "fit_ms": round(fit, 4)})
            else:
                row["fit_gate_refined_ms"] = round(fit, 4)
        rounds.append(row)
    options = 0
    fits()
    sc, lc = np.empty(N, np.int32), np.empty(N, np.int32)
    ctx.d2h(sc, d_sc)
    ctx.d2h(lc, d_lc)
    seg = np.empty((N, SEGMENTS_MAX, 6), np.int32)
    fit = np.empty((N, SEGMENTS_MAX, 12), np.int32)
    bases = np.empty((N, LINES_MAX), np.uint32)
    ctx.d2h(seg, d_seg)
    ctx.d2h(fit, d_fit)
    ctx.d2h(bases, d_bases)
    filled = np.minimum(sc, SEGMENTS_MAX)
    all_fits = np.concatenate([fit[f, :filled[f]] for f in range(N)])
    all_segs = np.concatenate([seg[f, :filled[f]] for f in range(N)])
    u = capi.line_fits_unpack(all_fits)
    # frame 0 against the host rule on the same call's smoothed plane and map
    d_sm = ctx.malloc(2 * H * W)
    ctx.dev_gaussian(d_in, SIGMA, H, W, 1, d_sm)
    plane, edges0 = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
    ctx.d2h(plane, d_sm)
    ctx.d2h(edges0, d_edges)
    want = capi.line_fits_from_plane(np.packbits(edges0 != 0, axis=-1), plane, bases[0, :min(int(lc[0]), LINES_MAX)],
                                     seg[0, :filled[0]], RHO, THETA)
    same = bool(np.array_equal(fit[0, :filled[0]], want))

    def med(key):
        v = [r[key] for r in rounds]
        return {"median": round(statistics.median(v), 4), "min": min(v), "max": max(v)}

    pixels = int(u["n"].sum())
    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rho": RHO, "theta_deg": 1,
              "hough_threshold": THRESHOLD, "lines_max": LINES_MAX, "min_length": MIN_LENGTH, "max_gap": MAX_GAP,
              "segments_max": SEGMENTS_MAX, "rounds": ROUNDS, "steps": STEPS, "lines": int(np.minimum(lc, LINES_MAX).sum()),
              "segments": int(filled.sum()), "segments_true": int(sc.sum()), "fitted_pixels": pixels,
              "positions_walked": int((np.maximum(np.abs(all_segs[:, 2] - all_segs[:, 0]),
                                                  np.abs(all_segs[:, 3] - all_segs[:, 1])) + 1).sum()),
              "degenerate": int(u["degenerate"].sum()), "invalid": int(u["invalid"].sum()),
              "rms_px_median": round(float(np.median(u["rms"][~u["degenerate"]])), 4) if pixels else None,
              "frame0_equals_the_host_rule": same, "count_ms": med("count_ms"), "emit_ms": med("emit_ms"),
              "fit_ms": med("fit_ms"), "fit_gate_refined_ms": med("fit_gate_refined_ms"),
              "fit_over_emit": round(med("fit_ms")["median"] / med("emit_ms")["median"], 3),
              "fit_ns_per_pixel": round(1e6 * med("fit_ms")["median"] / max(pixels, 1), 3), "per_round": rounds}
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_bases, d_lc, d_seg, d_sc, d_fit, d_sm):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's fits differ from the host rule")


if __name__ == "__main__":
    main()
