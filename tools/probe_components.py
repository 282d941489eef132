#!/usr/bin/env python3
"""Connected components on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device
resident: what the four parts of the labelling cost behind dev_canny, for min_area 1 and 20, with
the label plane and without it (records + filtered map only).

HIP-event times via components_profile_get (0 link, 1 resolve, 2 number, 3 write), "profile_stage_mask" set to those four
slots, in ONE process: ROUNDS rounds of STEPS calls of dev_canny_components after a warm-up, the variants alternating
within each round.  Two yardsticks from the same process: the HYST_FINALIZE launch of dev_hysteresis on a candidate plane
of the same shape (2 B/px written) and canny_hip_probe_copy of 4 B/px.  Frame 0's labels and records are compared with
the numpy rule (tests/components_rule.py) applied to the s16 map of the same call.
    python tools/probe_components.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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
ROUNDS, STEPS = 5, 3
VARIANTS = {"labels_min1": (1, True), "labels_min20": (20, True), "nolabels_min1": (1, False), "nolabels_min20": (20, False)}
PARTS = ("link", "resolve", "number", "write")


def main():
    import components_rule as rule
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges, d_labels, d_kept, d_off = (ctx.malloc(px), ctx.malloc(px * 2), ctx.malloc(px * 4), ctx.malloc(px),
                                              ctx.malloc(8 * (N + 1)))
    d_sm, d_cand, d_copy = ctx.malloc(px * 2), ctx.malloc(px * 2), ctx.malloc(px * 4)
    ctx.h2d(d_in, frames)
    offsets = np.empty(N + 1, np.uint64)
    # counts first: the record buffer is sized from them
    totals = {}
    for min_area in (1, 20):
        ctx.dev_canny_components(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, 0, 0, 0, d_off, d_edges)
        ctx.d2h(offsets, d_off)
        totals[min_area] = int(offsets[-1])
    d_stats = ctx.malloc(24 * max(totals[1], 1))
    ctx.dev_canny_points(d_in, SIGMA, LO, HI, H, W, N, 0, 0, d_off, d_edges)
    ctx.d2h(offsets, d_off)
    edge_px = int(offsets[-1])
    ctx.dev_gaussian(d_in, SIGMA, H, W, N, d_sm)

    def call(variant):
        min_area, with_labels = VARIANTS[variant]
        ctx.dev_canny_components(d_in, SIGMA, LO, HI, H, W, N, min_area, d_labels if with_labels else 0, d_kept, d_stats,
                                 totals[min_area], d_off, d_edges)

    def measure(variant):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 0b1111 << 13)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            call(variant)
        ctx.synchronize()
        ms = [ctx.components_profile_get(p)[0] / STEPS for p in range(4)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    def finalize_ms():
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", 1 << capi.STAGE_HYST_FINALIZE)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            ctx.dev_sobel_nms(d_sm, H, W, N, d_cand)  # dev_hysteresis works in place: a fresh candidate plane per call
            ctx.dev_hysteresis(d_cand, H, W, N, LO, HI)
        ms, launches = ctx.profile_get(capi.STAGE_HYST_FINALIZE)
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms / max(launches, 1)

    for v in VARIANTS:  # warm-up: workspaces, code objects
        call(v)
    finalize_ms()
    per_round = {v: [] for v in VARIANTS}
    fin, copy = [], []
    for _ in range(ROUNDS):
        for v in VARIANTS:
            per_round[v].append(measure(v))
        fin.append(finalize_ms())
        copy.append(ctx.probe_copy(d_labels, d_copy, px * 4, 5))

    # the timed output is the right one: frame 0 against the rule applied to the s16 map of the same call
    call("labels_min20")
    edges0, labels0 = np.empty((H, W), np.int16), np.empty((H, W), np.int32)
    ctx.d2h(edges0, d_edges)
    ctx.d2h(labels0, d_labels)
    ctx.d2h(offsets, d_off)
    stats0 = np.empty((int(offsets[1]), 6), np.int32)
    if stats0.size:
        ctx.d2h(stats0, d_stats)
    want_l, want_s = rule.components(edges0, 20)
    same = bool(np.array_equal(labels0, want_l) and np.array_equal(stats0, want_s))

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(), "edge_pixels": edge_px,
              "components_per_frame": {str(m): round(t / N, 1) for m, t in totals.items()},
              "frame0_equals_numpy_rule": same,
              "finalize_ms_per_launch": {"median": round(statistics.median(fin), 4), "min": round(min(fin), 4),
                                         "max": round(max(fin), 4)},
              "copy_4B_per_px_ms": {"median": round(statistics.median(copy), 4), "min": round(min(copy), 4),
                                    "max": round(max(copy), 4)}}
    for v, rounds in per_round.items():
        min_area, with_labels = VARIANTS[v]
        for i, part in enumerate(PARTS):
            vals = [r[i] for r in rounds]
            result[f"{v}_{part}_ms"] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4),
                                        "max": round(max(vals), 4)}
        result[f"{v}_total_ms"] = round(sum(result[f"{v}_{p}_ms"]["median"] for p in PARTS), 4)
        # bytes the outputs take: the label plane (4 B/px), the filtered map (1 B/px), the records
        result[f"{v}_output_bytes"] = px * (4 if with_labels else 0) + px + 24 * totals[min_area]
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_labels, d_kept, d_off, d_sm, d_cand, d_copy, d_stats):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's components differ from the numpy rule")


if __name__ == "__main__":
    main()
