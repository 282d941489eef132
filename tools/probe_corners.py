#!/usr/bin/env python3
"""Measures the corners and appends one JSON line per variant to profiles/corners.jsonl.

One process; per variant a warm-up call, then five rounds of three calls with the variants alternating within each round;
HIP-event times of the four parts through canny_hip_corners_profile_get (reset before every call).  Variants: Shi-Tomasi
and Harris (k_q8 10) for blocks 3 and 7 at corners_max 256, and Shi-Tomasi block 3 at corners_max 4096, through
canny_hip_dev_corners_plane on the plane a dev_canny call left, on a synth_batch of 3840 x 2160 frames (sigma 1.4,
thresholds 50 / 150; quality_q16 655, min_dist 10).  Yardsticks from the same process: the dev_canny step (wall clock
around a synchronised call) and canny_hip_probe_copy of the 1 B/px plane.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners.jsonl"))
    args = ap.parse_args()

    n = args.frames
    frames = synth_batch(n, H, W)
    with capi.Context(0) as ctx:
        d_img, d_edges = ctx.malloc(frames.nbytes), ctx.malloc(2 * frames.size)
        ctx.h2d(d_img, frames)
        canny_ms = []
        for k in range(4):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.dev_canny(d_img, SIGMA, LO, HI, H, W, n, d_edges)
            ctx.synchronize()
            if k:
                canny_ms.append(1e3 * (time.perf_counter() - t0))
        plane_u8 = ctx.get_option("last_canny_smoothed_u8")
        copy_ms = ctx.probe_copy(d_img, d_edges, frames.size // 16 * 16, 5)   # the plane's bytes, read + written
        cmax_all = 4096
        d_rec, d_cnt = ctx.malloc(8 * 4 * cmax_all * n), ctx.malloc(8 * n)
        d_max = ctx.malloc(8 * n)

        variants = [dict(mode=m, block=b, k_q8=k, cmax=c, ms={p: [] for p in capi.CORNER_PARTS})
                    for m, k in ((0, 0), (1, 10)) for b in (3, 7) for c in (256,)]
        variants.append(dict(mode=0, block=3, k_q8=0, cmax=cmax_all, ms={p: [] for p in capi.CORNER_PARTS}))
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30: only corners run here

        def call(v):
            ctx.profile_reset()
            ctx.dev_corners_plane(0, n, H, W, v["mode"], v["block"], v["k_q8"], 655, 0, 10, v["cmax"], d_rec, d_cnt,
                                  d_cnt + 4 * n, d_max)
            return [ctx.corners_profile_get(p)[0] for p in range(len(capi.CORNER_PARTS))]

        for v in variants:
            call(v)
            cnt = np.empty(2 * n, np.int32)
            ctx.d2h(cnt, d_cnt)
            v["corners"], v["candidates"] = int(cnt[:n].sum()), int(cnt[n:].sum())
            v["frames_over_corners_max"] = int((cnt[n:] > v["cmax"]).sum())
            print(f"warm: mode {v['mode']} block {v['block']} corners_max {v['cmax']}: {v['corners']} corners of "
                  f"{v['candidates']} candidates", flush=True)
        for rnd in range(5):
            print(f"round {rnd + 1} of 5", flush=True)
            for v in variants:
                for _ in range(3):
                    for name, ms in zip(capi.CORNER_PARTS, call(v)):
                        v["ms"][name].append(ms)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for v in variants:
                total = [sum(x) for x in zip(*v["ms"].values())]
                line = dict(box=args.box, frames=n, height=H, width=W, mode=("min_eigen", "harris")[v["mode"]],
                            block=v["block"], k_q8=v["k_q8"], quality_q16=655, min_dist=10, corners_max=v["cmax"],
                            plane_u8=plane_u8, calls=len(total), corners=v["corners"], candidates=v["candidates"],
                            frames_over_corners_max=v["frames_over_corners_max"],
                            ms={k: dict(median=statistics.median(x), min=min(x), max=max(x)) for k, x in v["ms"].items()},
                            total_ms=dict(median=statistics.median(total), min=min(total), max=max(total)),
                            gpix_per_s_max_pass=n * H * W / (statistics.median(v["ms"]["max"]) * 1e6),
                            dev_canny_wall_ms=dict(median=statistics.median(canny_ms), min=min(canny_ms), max=max(canny_ms)),
                            probe_copy_plane_ms=copy_ms,
                            times="HIP events around each part's launches; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line))


if __name__ == "__main__":
    main()
