#!/usr/bin/env python3
"""Measures the corner descriptors and their matching and appends one JSON line per variant to
profiles/descriptors.jsonl.

One process; per variant a warm-up, then five rounds of three calls with the variants alternating within each round;
HIP-event times of the four parts through canny_hip_descriptors_profile_get (reset before every call).  Variants:
corners_max 256 and 4096, upright and steered, on the corners (Shi-Tomasi, block 3, quality_q16 655, min_dist 10) of a
synth_batch of 3840 x 2160 frames (sigma 1.4, thresholds 50 / 150); the descriptors through
canny_hip_dev_corner_descriptors on the plane a dev_canny call left, the matching over the frames - 1 consecutive pairs
(64, 205, cross-check).  Yardsticks from the same process: the dev_canny step and the corners call (wall clock around a
synchronised call).

--frames N          frames of the batch (default 128)
--box NAME          recorded in every line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from canny_edge_amd import capi  # noqa: E402
from canny_edge_amd.synth import synth_batch  # noqa: E402

H, W = 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
# VALU instructions of desc_match_kernel's inner loop per candidate and lane, read from the gfx950 ISA
VALU_PER_CANDIDATE = 24.25   # 97 in the loop body, which is unrolled over four candidates


def wall(ctx, fn, repeat=3):
    out = []
    for k in range(repeat + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if k:
            out.append(1e3 * (time.perf_counter() - t0))
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "descriptors.jsonl"))
    args = ap.parse_args()

    n = args.frames
    frames = synth_batch(n, H, W)
    pairs = capi.consecutive_pairs(n)
    with capi.Context(0) as ctx:
        d_img, d_edges = ctx.malloc(frames.nbytes), ctx.malloc(2 * frames.size)
        ctx.h2d(d_img, frames)
        canny_ms = wall(ctx, lambda: ctx.dev_canny(d_img, SIGMA, LO, HI, H, W, n, d_edges))
        plane_u8 = ctx.get_option("last_canny_smoothed_u8")
        variants = []
        for cmax in (256, 4096):
            d_rec, d_cnt = ctx.malloc(8 * 4 * cmax * n), ctx.malloc(4 * n)
            corners_ms = wall(ctx, lambda: ctx.dev_corners_plane(0, n, H, W, 0, 3, 0, 655, 0, 10, cmax, d_rec, d_cnt))
            cnt = np.empty(n, np.int32)
            ctx.d2h(cnt, d_cnt)
            for steered in (0, 1):
                variants.append(dict(cmax=cmax, steered=steered, d_rec=d_rec, d_cnt=d_cnt, counts=cnt, corners_ms=corners_ms,
                                     d_desc=ctx.malloc(8 * 4 * cmax * n), d_meta=ctx.malloc(4 * cmax * n),
                                     d_m=ctx.malloc(4 * 4 * cmax * max(n - 1, 1)), d_pc=ctx.malloc(4 * max(n - 1, 1)),
                                     ms={p: [] for p in capi.DESC_PARTS}))
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30

        def call(v):
            ctx.profile_reset()
            ctx.dev_corner_descriptors(0, n, H, W, v["d_rec"], v["d_cnt"], v["cmax"], v["d_desc"], v["d_meta"], v["steered"])
            if len(pairs):
                ctx.dev_match_descriptors(v["d_desc"], v["d_cnt"], n, v["cmax"], v["d_desc"], v["d_cnt"], n, v["cmax"], pairs,
                                          v["d_m"], v["d_pc"], 64, 205, capi.MATCH_CROSS_CHECK)
            return [ctx.descriptors_profile_get(p)[0] for p in range(len(capi.DESC_PARTS))]

        for v in variants:
            call(v)
            acc = np.zeros(max(n - 1, 1), np.int32)
            if len(pairs):
                ctx.d2h(acc, v["d_pc"])
            c = v["counts"].astype(np.int64)
            v["corners"], v["accepted"] = int(c.sum()), int(acc.sum()) if len(pairs) else 0
            v["descriptor_pairs"] = int((c[:-1] * c[1:]).sum())
            print(f"warm: corners_max {v['cmax']} steered {v['steered']}: {v['corners']} corners, {v['accepted']} matches "
                  f"accepted over {len(pairs)} pairs", flush=True)
        for rnd in range(5):
            print(f"round {rnd + 1} of 5", flush=True)
            for v in variants:
                for _ in range(3):
                    for name, ms in zip(capi.DESC_PARTS, call(v)):
                        v["ms"][name].append(ms)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for v in variants:
                total = [sum(x) for x in zip(*v["ms"].values())]
                match_ms = statistics.median(v["ms"]["match"])
                rate = v["descriptor_pairs"] / (match_ms * 1e-3) if match_ms > 0 else 0.0
                line = dict(box=args.box, frames=n, height=H, width=W, corners_max=v["cmax"], steered=v["steered"],
                            pairs=len(pairs), max_distance=64, ratio_q8=205, cross_check=1, plane_u8=plane_u8,
                            calls=len(total), corners=v["corners"], accepted=v["accepted"],
                            descriptor_pairs=v["descriptor_pairs"],
                            ms={k: dict(median=statistics.median(x), min=min(x), max=max(x)) for k, x in v["ms"].items()},
                            total_ms=dict(median=statistics.median(total), min=min(total), max=max(total)),
                            match_descriptor_pairs_per_s=rate,
                            match_valu_lane_instructions_per_s=rate * VALU_PER_CANDIDATE,
                            valu_per_candidate=VALU_PER_CANDIDATE,
                            dev_canny_wall_ms=canny_ms, corners_wall_ms=v["corners_ms"],
                            times="HIP events around each part's launches; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line))


if __name__ == "__main__":
    main()
