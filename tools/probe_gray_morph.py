#!/usr/bin/env python3
"""Times the grey-level morphology (canny_hip_profile_part_get, group "gray_morph") on a batch of u8 planes, under the general
route and the fast one:
  ERODE by 3 x 3, 5 x 5, 7 x 7, 15 x 15 and 31 x 31 rectangles and a 15 x 15 ellipse (which runs the general kernel under both
  settings),
  BLACKHAT by 15 x 15 (two steps and the difference), MEDIAN 3 x 3 and 5 x 5 (REPLICATE),
and in the same rounds a plain device copy (canny_hip_probe_copy) of the same bytes.  HIP events around the call's launches,
one warm-up call per variant, then rounds that alternate over all variants.  Appends one JSON line per variant to
profiles/gray_morph.jsonl.

    python tools/probe_gray_morph.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
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

ROUTES = (("general", capi.GRAY_ROUTE_GENERAL), ("fast", capi.GRAY_ROUTE_FAST))
CASES = (("erode", capi.GRAY_ERODE, capi.MORPH_RECT, 3), ("erode", capi.GRAY_ERODE, capi.MORPH_RECT, 5),
         ("erode", capi.GRAY_ERODE, capi.MORPH_RECT, 7), ("erode", capi.GRAY_ERODE, capi.MORPH_RECT, 15),
         ("erode", capi.GRAY_ERODE, capi.MORPH_RECT, 31), ("erode", capi.GRAY_ERODE, capi.MORPH_ELLIPSE, 15),
         ("blackhat", capi.GRAY_BLACKHAT, capi.MORPH_RECT, 15), ("median", capi.GRAY_MEDIAN, capi.MORPH_RECT, 3),
         ("median", capi.GRAY_MEDIAN, capi.MORPH_RECT, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gray_morph.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    fpx = h * w
    distinct = min(n, 4)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 0x7FFFFFFF)   # the parts behind the polygons go by bit 30
        d_frames, d_out, d_copy = ctx.malloc(n * fpx + 16), ctx.malloc(n * fpx + 16), ctx.malloc(n * fpx + 16)
        frames = [synth_frame(h, w, 42 + i) for i in range(distinct)]   # the benchmark's frames, in turn
        for f in range(n):
            ctx.h2d(d_frames + f * fpx, frames[f % distinct])
        variants = [dict(case=case, op=op, shape=shape, k=k, route=route, rows=capi.morph_element(shape, k, k), ms=[], copy=[])
                    for case, op, shape, k in CASES for route in ROUTES]

        def call(v):
            ctx.profile_reset()
            ctx.set_option("gray_morph_route", v["route"][1])
            border = capi.GRAY_BORDER_REPLICATE if v["op"] == capi.GRAY_MEDIAN else capi.GRAY_BORDER_NEUTRAL
            ctx.dev_gray_morph(d_frames, n, h, w, v["op"], v["rows"], v["k"], v["k"], d_out, border)
            return ctx.profile_part("gray_morph", 0)[0]

        for v in variants:
            print("warm-up", v["case"], capi.MORPH_SHAPES[v["shape"]], v["k"], v["route"][0], flush=True)
            call(v)
        ctx.probe_copy(d_frames, d_copy, (n * fpx) & ~15, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v))
                v["copy"].append(ctx.probe_copy(d_frames, d_copy, (n * fpx) & ~15, args.calls))
        cp = statistics.median([c for v in variants for c in v["copy"]])
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms = statistics.median(v["ms"])
                steps = 2 if v["op"] == capi.GRAY_BLACKHAT else 1
                line = dict(box=args.box, frames=n, height=h, width=w, op=capi.GRAY_OPS[v["op"]], shape=capi.MORPH_SHAPES[v["shape"]],
                            kw=v["k"], kh=v["k"], route=v["route"][0], auto_route=capi.gray_morph_plan(n, h, w, v["op"], v["k"], v["k"]).aux,
                            steps=steps, calls=len(v["ms"]), ms=stat(v["ms"]), ms_per_step=ms / steps, copy_ms=cp,
                            over_copy=ms / cp if cp > 0 else 0.0, gpx_per_s=n * fpx * steps / ms / 1e6 if ms > 0 else 0.0)
                line["times"] = ("HIP events around the call's launches (part steps of group gray_morph); the copy is "
                                 "canny_hip_probe_copy of one batch of planes, the median over all rounds; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
