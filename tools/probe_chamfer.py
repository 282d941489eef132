#!/usr/bin/env python3
"""Measures the chamfer matching and appends one JSON line per variant to profiles/chamfer.jsonl.

One process; per variant a warm-up call, then five rounds of three calls with the variants alternating within each round;
HIP-event times of the four parts through canny_hip_chamfer_profile_get (reset before every call).  Variants: the direct
and the tiled route for T = 1 and 8 ring templates of K = 64, 256 and 1024 points on a synth_batch of 3840 x 2160 frames
(sigma 1.4, thresholds 50 / 150), plus T = 8, K = 256 on one frame.  Yardsticks from the same process: dev_canny_edt alone
(wall clock around a synchronised call) and canny_hip_probe_copy of the cost plane's bytes.

--frames N          frames of the batch (default 128)
--max-lookups L     shrink a variant's batch so that one call makes at most L look-ups (frames * pixels * T * K); the line
                    records the frames actually used.  0 (default): no limit
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
ROUTES = {1: "direct", 2: "tiled"}


def ring(k):
    """k points on a circle of radius k / 5.6 (about one per boundary pixel), rounded; duplicates stay."""
    r = k / 5.6
    a = 2 * np.pi * np.arange(k) / k
    return np.stack([np.rint(r * np.cos(a)), np.rint(r * np.sin(a))], axis=1).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--max-lookups", type=float, default=0)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer.jsonl"))
    args = ap.parse_args()

    frames = synth_batch(args.frames, H, W)
    px = H * W
    with capi.Context(0) as ctx:
        d_img, d_dist2 = ctx.malloc(frames.nbytes), ctx.malloc(4 * frames.size)
        ctx.h2d(d_img, frames)
        mm = 256
        d_rec, d_cnt = ctx.malloc(4 * 6 * mm * args.frames), ctx.malloc(8 * args.frames)
        edt_ms = []
        for k in range(4):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.dev_canny_edt(d_img, 1.4, 50, 150, H, W, args.frames, d_dist2, 0, 0)
            ctx.synchronize()
            if k:
                edt_ms.append(1e3 * (time.perf_counter() - t0))
        d_tmp = ctx.malloc(2 * frames.size)
        copy_ms = ctx.probe_copy(d_dist2, d_tmp, (2 * frames.size) // 16 * 16, 5)   # the cost plane's bytes, read + written
        ctx.free(d_tmp)

        variants = []
        for n, T, K in [(args.frames, T, K) for T in (1, 8) for K in (64, 256, 1024)] + [(1, 8, 256)]:
            if args.max_lookups and n > 1:
                n = int(max(1, min(n, args.max_lookups // (px * T * K))))
            cset = ctx.chamfer_set_create([ring(K)] * T)
            for route in ROUTES:
                variants.append(dict(n=n, T=T, K=K, route=route, cset=cset, ms={p: [] for p in capi.CHAMFER_PARTS}))
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30: only chamfer runs here

        def call(v):
            ctx.set_option("chamfer_route", v["route"])
            ctx.profile_reset()
            ctx.dev_chamfer_dist2(d_dist2, v["n"], H, W, v["cset"], 160, 24, 8, mm, d_rec, d_cnt, d_cnt + 4 * args.frames)
            return [ctx.chamfer_profile_get(p)[0] for p in range(len(capi.CHAMFER_PARTS))]

        for v in variants:
            call(v)
            print(f"warm: {v['n']} frames, T {v['T']}, K {v['K']}, {ROUTES[v['route']]}", flush=True)
        for rnd in range(5):
            print(f"round {rnd + 1} of 5", flush=True)
            for v in variants:
                for _ in range(3):
                    for name, ms in zip(capi.CHAMFER_PARTS, call(v)):
                        v["ms"][name].append(ms)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for v in variants:
                score = v["ms"]["score"]
                lookups = v["n"] * px * v["T"] * v["K"]
                line = dict(box=args.box, frames=v["n"], height=H, width=W, templates=v["T"], points=v["K"],
                            route=ROUTES[v["route"]], calls=len(score),
                            ms={k: dict(median=statistics.median(x), min=min(x), max=max(x)) for k, x in v["ms"].items()},
                            lookups=lookups, lookups_per_s=lookups / (statistics.median(score) * 1e-3),
                            lds_read_bytes_per_s=(2 * lookups / (statistics.median(score) * 1e-3)
                                                  if v["route"] == 2 else None),
                            canny_edt_wall_ms=dict(median=statistics.median(edt_ms), min=min(edt_ms), max=max(edt_ms),
                                                   frames=args.frames),
                            probe_copy_cost_plane_ms=copy_ms, probe_copy_frames=args.frames,
                            times="HIP events around each part's launches; look-up rates are inferred from them, no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line))


if __name__ == "__main__":
    main()
