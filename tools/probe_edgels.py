#!/usr/bin/env python3
"""Sub-pixel edgels on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device
resident: what the records cost beyond dev_canny, next to the point lists of the same map and a plain copy (DESIGN.md
section 23).

  layout, refine  the two parts of dev_canny_edgels (count + scan; the row kernel), per call
  compact         the COMPACT stage of dev_canny_points (count + scan + scatter), per call
  copy            canny_hip_probe_copy of as many bytes as the records hold (16 B per edgel read and written)

All are HIP-event times in ONE process, ROUNDS rounds of STEPS calls after a warm-up, the calls alternating; medians and
ranges over the rounds.  The refined share and frame 0 against the host rule come from the timed output itself.
    python tools/probe_edgels.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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
ROUNDS, STEPS = 5, 5


def main():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges, d_off = ctx.malloc(px), ctx.malloc(px * 2), ctx.malloc(8 * (N + 1))
    ctx.h2d(d_in, frames)
    ctx.dev_canny_edgels(d_in, SIGMA, LO, HI, H, W, N, 0, 0, d_off, d_edges)  # counts first: they size the buffers
    offsets = np.empty(N + 1, np.uint64)
    ctx.d2h(offsets, d_off)
    total = int(offsets[-1])
    rec_bytes = 16 * max(total, 1)
    d_rec, d_pts, d_copy = ctx.malloc(rec_bytes), ctx.malloc(4 * max(total, 1)), ctx.malloc(rec_bytes)

    def edgels():
        ctx.dev_canny_edgels(d_in, SIGMA, LO, HI, H, W, N, d_rec, total, d_off, d_edges)

    def points():
        ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, d_pts, total, d_off, d_edges)

    def timed(fn, mask, read):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", mask)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            fn()
        ctx.synchronize()
        ms = read()
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for _ in range(2):  # warm-up: workspaces, code objects
        edgels()
        points()
    rounds = []
    for _ in range(ROUNDS):
        lay, ref = timed(edgels, 1 << 30, lambda: [ctx.edgels_profile_get(p)[0] / STEPS for p in (0, 1)])
        comp = timed(points, 1 << capi.STAGE_COMPACT, lambda: ctx.profile_get(capi.STAGE_COMPACT)[0] / STEPS)
        copy = ctx.probe_copy(d_rec, d_copy, rec_bytes, STEPS)
        rounds.append({"layout_ms": round(lay, 4), "refine_ms": round(ref, 4), "points_compact_ms": round(comp, 4),
                       "copy_of_the_records_ms": round(copy, 4)})
    edgels()
    rec = np.empty((total, 4), np.int32)
    ctx.d2h(rec, d_rec)
    _, refined, invalid = capi.edgels_flags(rec)
    # frame 0 against the host rule on the same call's smoothed plane and map
    d_sm = ctx.malloc(2 * H * W)
    ctx.dev_gaussian(d_in, SIGMA, H, W, 1, d_sm)
    plane, edges0 = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
    ctx.d2h(plane, d_sm)
    ctx.d2h(edges0, d_edges)
    want = capi.edgels_from_plane(plane, np.flatnonzero(edges0.reshape(-1)))
    same = bool(np.array_equal(rec[:int(offsets[1])], want))

    def med(key):
        v = [r[key] for r in rounds]
        return {"median": round(statistics.median(v), 4), "min": min(v), "max": max(v)}

    extra = statistics.median(r["layout_ms"] + r["refine_ms"] for r in rounds)
    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS, "steps": STEPS,
              "edgels": total, "edge_density": round(total / px, 6), "refined_share": round(float(refined.mean()), 4),
              "invalid": int(invalid.sum()), "frame0_equals_the_host_rule": same,
              "layout_ms": med("layout_ms"), "refine_ms": med("refine_ms"), "points_compact_ms": med("points_compact_ms"),
              "copy_of_the_records_ms": med("copy_of_the_records_ms"),
              "edgel_extra_over_points_extra": round(extra / med("points_compact_ms")["median"], 3),
              "record_bytes_per_edgel": 16, "refine_ns_per_edgel": round(1e6 * med("refine_ms")["median"] / max(total, 1), 4),
              "refine_record_gb_per_s": round(16 * total / (1e6 * med("refine_ms")["median"]), 1), "per_round": rounds}
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_off, d_rec, d_pts, d_copy, d_sm):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's records differ from the host rule")


if __name__ == "__main__":
    main()
