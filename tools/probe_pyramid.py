#!/usr/bin/env python3
"""Times the image pyramid calls (canny_hip_profile_part_get, group "pyramid") on a batch of u8 planes:
  dev_pyr_down under the direct and the tiled route,
  dev_pyramid with 5 levels under both routes,
  dev_pyr_up of level 1 to the full size,
and in the same rounds a plain device copy (canny_hip_probe_copy) of one batch of planes.  pyrDown moves 1.25 bytes per source
pixel where the copy moves 2: every pyrDown line states its time over 0.625 x the copy's.  HIP events around the call's
launches, one warm-up call per variant, then rounds that alternate over all variants.  Appends one JSON line per variant to
profiles/pyramid.jsonl.

    python tools/probe_pyramid.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from canny_edge_amd import capi  # noqa: E402
from canny_edge_amd.synth import synth_frame  # noqa: E402

ROUTES = (("direct", capi.PYR_ROUTE_DIRECT), ("tiled", capi.PYR_ROUTE_TILED))
LEVELS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    fpx = h * w
    distinct = min(n, 4)
    info, total = capi.pyramid_layout(n, h, w, LEVELS)
    h1, w1 = int(info[0][0]), int(info[0][1])
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 0x7FFFFFFF)   # the parts behind the polygons go by bit 30
        d_frames, d_pyr, d_up = ctx.malloc(n * fpx + 16), ctx.malloc(total + 16), ctx.malloc(n * fpx + 16)
        frames = [synth_frame(h, w, 42 + i) for i in range(distinct)]   # the benchmark's frames, in turn
        for f in range(n):
            ctx.h2d(d_frames + f * fpx, frames[f % distinct])
        variants = [dict(call="pyr_down", route=r, ms=[], copy=[]) for r in ROUTES]
        variants += [dict(call="pyramid", route=r, ms=[], copy=[]) for r in ROUTES]
        variants += [dict(call="pyr_up", route=("one", 0), ms=[], copy=[])]

        def call(v):
            ctx.profile_reset()
            ctx.set_option("pyramid_route", v["route"][1])
            if v["call"] == "pyr_down":
                ctx.dev_pyr_down(d_frames, n, h, w, d_pyr)
            elif v["call"] == "pyramid":
                ctx.dev_pyramid(d_frames, n, h, w, LEVELS, d_pyr)
            else:
                ctx.dev_pyr_up(d_pyr, n, h1, w1, h, w, d_up)             # level 1 lies at offset 0
            ctx.set_option("pyramid_route", 0)
            return ctx.profile_part("pyramid", capi.PYR_PART_UP if v["call"] == "pyr_up" else capi.PYR_PART_DOWN)[0]

        for v in variants:
            print("warm-up", v["call"], v["route"][0], flush=True)
            call(v)
        ctx.probe_copy(d_frames, d_up, (n * fpx) & ~15, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v))
                v["copy"].append(ctx.probe_copy(d_frames, d_up, (n * fpx) & ~15, args.calls))
        cp = statistics.median([c for v in variants for c in v["copy"]])
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        # bytes moved per source pixel of level 0: read once, a quarter written; the pyramid repeats that a quarter the size
        moved = {"pyr_down": 1.25, "pyramid": sum(1.25 / 4 ** l for l in range(LEVELS)), "pyr_up": 1.25}
        with open(args.out, "a") as f:
            for v in variants:
                ms = statistics.median(v["ms"])
                floor = cp * moved[v["call"]] / 2.0
                line = dict(box=args.box, frames=n, height=h, width=w, call=v["call"], route=v["route"][0],
                            levels=LEVELS if v["call"] == "pyramid" else 1, auto_route=capi.pyramid_plan(n, h, w).aux,
                            calls=len(v["ms"]), ms=stat(v["ms"]), copy_ms=cp, bytes_per_source_pixel=moved[v["call"]],
                            over_copy=ms / cp if cp > 0 else 0.0, over_copy_of_the_same_bytes=ms / floor if floor > 0 else 0.0,
                            source_gpx_per_s=n * fpx / ms / 1e6 if ms > 0 else 0.0)
                line["times"] = ("HIP events around the call's launches (parts of group pyramid); the copy is canny_hip_probe_copy "
                                 "of one batch of planes (2 bytes a pixel), the median over all rounds; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
