#!/usr/bin/env python3
"""Sub-pixel circle fits on the Hough circles' own workload (DESIGN.md sections 18 and 25): 128 x 3840x2160 synth_batch, sigma
1.4, thresholds 50 / 150, radii 10..100, cell_shift 1, circle threshold 30, support threshold 20, min_dist 10, centres_max
256, device resident.

  radius, accept  the two per-candidate parts of the circles (canny_hip_hough_circles_profile_get), per call
  fit             the one part of the circle fits behind them (canny_hip_circle_fits_profile_get), per call, for three
                  settings: band 1 / REFINED_ONLY, the same with a trim of 64, and band 4 / trim 64 / every pixel

All are HIP-event times of the SAME calls in one process, ROUNDS rounds of STEPS calls after a warm-up; medians and ranges
over the rounds.  Frame 0's fits are compared with the host rule on the same call's map and smoothed plane.
    python tools/probe_circle_fits.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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
MIN_R, MAX_R, CELL_SHIFT, THRESHOLD, SUPPORT, MIN_DIST, CENTRES_MAX = 10, 100, 1, 30, 20, 10, 256
SETTINGS = {"band1_refined": (1, 0, 2), "band1_refined_trim64": (1, 64, 2), "band4_all_trim64": (4, 64, 0)}
ROUNDS, STEPS = 5, 3


def main():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    slots = N * CENTRES_MAX
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_rec, d_counts, d_fit = ctx.malloc(24 * slots), ctx.malloc(4 * N), ctx.malloc(32 * slots)
    ctx.h2d(d_in, frames)

    def fits(setting):
        band, trim_q8, options = SETTINGS[setting]
        ctx.dev_canny_hough_circle_fits(d_in, SIGMA, LO, HI, H, W, N, MIN_R, MAX_R, CELL_SHIFT, THRESHOLD, SUPPORT, MIN_DIST,
                                        CENTRES_MAX, band, trim_q8, options, d_fit, d_rec, d_counts, d_edges=d_edges)

    for s in SETTINGS:  # warm-up: workspaces, code objects
        fits(s)
    rounds = []
    for _ in range(ROUNDS):
        row = {}
        for s in SETTINGS:
            ctx.synchronize()
            ctx.profile_reset()
            ctx.set_option("profile_stage_mask", (1 << 28) | (1 << 29) | (1 << 30))
            ctx.profile_enable(True)
            for _ in range(STEPS):
                fits(s)
            ctx.synchronize()
            radius, accept = (ctx.hough_circles_profile_get(p)[0] / STEPS for p in (2, 3))
            fit = ctx.circle_fits_profile_get(capi.CIRCLE_FIT_PART_FIT)[0] / STEPS
            ctx.profile_enable(False)
            ctx.set_option("profile_stage_mask", 0)
            row.update({"radius_ms": round(radius, 4), "accept_ms": round(accept, 4), f"fit_{s}_ms": round(fit, 4)})
        rounds.append(row)
    stats = {}
    same = True
    d_sm = ctx.malloc(2 * H * W)
    ctx.dev_gaussian(d_in, SIGMA, H, W, 1, d_sm)
    plane = np.empty((H, W), np.int16)
    ctx.d2h(plane, d_sm)
    for s, (band, trim_q8, options) in SETTINGS.items():
        fits(s)
        cnt = np.empty(N, np.int32)
        rec = np.empty((N, CENTRES_MAX, 6), np.int32)
        fit = np.empty((N, CENTRES_MAX, 8), np.int32)
        edges0 = np.empty((H, W), np.int16)
        ctx.d2h(cnt, d_counts)
        ctx.d2h(rec, d_rec)
        ctx.d2h(fit, d_fit)
        ctx.d2h(edges0, d_edges)
        all_fits = np.concatenate([fit[f, :cnt[f]] for f in range(N)])
        all_recs = np.concatenate([rec[f, :cnt[f]] for f in range(N)])
        u = capi.circle_fits_unpack(all_fits)
        ok = ~u["degenerate"] & ~u["invalid"]
        # frame 0 against the host rule on the same call's smoothed plane and map
        want = capi.circle_fits_from_plane(np.packbits(edges0 != 0, axis=-1), plane, rec[0, :cnt[0]], band, trim_q8, options)
        same = same and bool(np.array_equal(fit[0, :cnt[0]], want))
        stats[s] = {"circles": int(cnt.sum()), "fitted_pixels": int(u["n"].sum()), "degenerate": int(u["degenerate"].sum()),
                    "trim_failed": int(u["trim_failed"].sum()), "radius_median": int(np.median(all_recs[:, 2])) if len(all_recs) else None,
                    "rms_px_median": round(float(np.median(u["rms"][ok])), 4) if ok.any() else None,
                    "full_circles": int((u["sector_count"][ok] == 16).sum())}

    def med(key):
        v = [r[key] for r in rounds]
        return {"median": round(statistics.median(v), 4), "min": min(v), "max": max(v)}

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "radii": [MIN_R, MAX_R],
              "cell_shift": CELL_SHIFT, "threshold": THRESHOLD, "support_threshold": SUPPORT, "min_dist": MIN_DIST,
              "centres_max": CENTRES_MAX, "rounds": ROUNDS, "steps": STEPS, "queue_capacity": capi.circle_fits_queue_capacity(),
              "settings": {s: list(v) for s, v in SETTINGS.items()}, "stats": stats, "frame0_equals_the_host_rule": same,
              "radius_ms": med("radius_ms"), "accept_ms": med("accept_ms")}
    for s in SETTINGS:
        result[f"fit_{s}_ms"] = med(f"fit_{s}_ms")
        result[f"fit_{s}_ns_per_pixel"] = round(1e6 * result[f"fit_{s}_ms"]["median"] / max(stats[s]["fitted_pixels"], 1), 3)
    result["per_round"] = rounds
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_rec, d_counts, d_fit, d_sm):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's fits differ from the host rule")


if __name__ == "__main__":
    main()
