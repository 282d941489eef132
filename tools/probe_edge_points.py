#!/usr/bin/env python3
"""Edge point lists on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device
resident: what the compaction costs, next to the existing pass that also reads the strong plane once (DESIGN.md
section 12).

  compact   the COMPACT stage of dev_canny_points (count + scan + scatter kernels), per call
  finalize  the HYST_FINALIZE stage of dev_hysteresis on an s16 candidate plane of the same shape, per launch (the
            speculative finalize may run more than once per call)

Both are HIP-event stage times with "profile_stage_mask" set to that one stage, in ONE process, ROUNDS rounds of STEPS
calls after a warm-up, the two stages alternating; the batch's edge density comes from the offsets.
    python tools/probe_edge_points.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
ROUNDS, STEPS = 5, 5


def main():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges, d_sm, d_cand, d_off = (ctx.malloc(px), ctx.malloc(px * 2), ctx.malloc(px * 2), ctx.malloc(px * 2),
                                          ctx.malloc(8 * (N + 1)))
    ctx.h2d(d_in, frames)
    # counts first: the points buffer is sized from them
    ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, 0, 0, d_off, d_edges)
    offsets = np.empty(N + 1, np.uint64)
    ctx.d2h(offsets, d_off)
    total = int(offsets[-1])
    d_pts = ctx.malloc(4 * max(total, 1))
    ctx.dev_gaussian(d_in, SIGMA, H, W, N, d_sm)

    def compact():
        ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, d_pts, total, d_off, d_edges)

    def finalize():
        ctx.dev_sobel_nms(d_sm, H, W, N, d_cand)  # dev_hysteresis works in place: a fresh candidate plane per call
        ctx.dev_hysteresis(d_cand, H, W, N, LO, HI)

    def stage_ms(fn, stage):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 1 << stage)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            fn()
        ctx.synchronize()
        ms, launches = ctx.profile_get(stage)
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms, launches

    for _ in range(2):  # warm-up: workspaces, code objects
        compact()
        finalize()
    rounds = []
    for _ in range(ROUNDS):
        c_ms, c_n = stage_ms(compact, capi.STAGE_COMPACT)
        f_ms, f_n = stage_ms(finalize, capi.STAGE_HYST_FINALIZE)
        rounds.append({"compact_ms_per_call": round(c_ms / STEPS, 4), "compact_event_pairs": c_n,
                       "finalize_ms_per_launch": round(f_ms / max(f_n, 1), 4), "finalize_launches": f_n})
    # the timed output is the right one: against the s16 map of the same call
    pts, edges = np.empty(total, np.uint32), np.empty((N, H, W), np.int16)
    ctx.d2h(pts, d_pts)
    ctx.d2h(edges, d_edges)
    same = all(np.array_equal(pts[int(offsets[f]):int(offsets[f + 1])], np.flatnonzero(edges[f])) for f in range(N))
    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(),
              "edge_pixels": total, "edge_density": round(total / px, 6),
              "points_equal_flatnonzero_of_the_map": bool(same),
              "compact_ms_per_call_median": round(statistics.median(r["compact_ms_per_call"] for r in rounds), 4),
              "finalize_ms_per_launch_median": round(statistics.median(r["finalize_ms_per_launch"] for r in rounds), 4),
              "per_round": rounds}
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_sm, d_cand, d_off, d_pts):
        ctx.free(p)
    if not same:
        raise SystemExit("the point lists differ from the s16 map")


if __name__ == "__main__":
    main()
