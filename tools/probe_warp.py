#!/usr/bin/env python3
"""Times the warp (canny_hip_warp_profile_get, part WARP) on a batch of frames warped onto themselves by one transform per
case -- the identity, a sub-pixel shift, a 1 degree turn with scale 1.01 about the centre, a quarter turn, half scale -- for
both interpolations and routes 1 (direct) and 2 (tiled), and beside each, in the same run, a plain device copy of the same
1 B/px in + 1 B/px out (canny_hip_probe_copy): the yardstick.  HIP events around the launch, one warm-up call per variant, then
rounds that alternate over all variants; appends one JSON line per variant to profiles/warp.jsonl.

    python tools/probe_warp.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from canny_edge_amd import capi  # noqa: E402

ONE = 65536


def about_centre(a11, a12, a21, a22, cx, cy):
    return (a11, a12, int(round(cx * ONE - a11 * cx - a12 * cy)), a21, a22, int(round(cy * ONE - a21 * cx - a22 * cy)))


def cases(h, w):
    """name -> (coefficients, source height, source width): the quarter turn reads frames of the turned geometry."""
    c, s = math.cos(math.radians(1.0)) * 1.01, math.sin(math.radians(1.0)) * 1.01
    turn = about_centre(int(round(c * ONE)), int(round(-s * ONE)), int(round(s * ONE)), int(round(c * ONE)), (w - 1) / 2,
                        (h - 1) / 2)
    return {"identity": ((ONE, 0, 0, 0, ONE, 0), h, w),
            "shift": ((ONE, 0, int(round(-6.977 * ONE)), 0, ONE, int(round(-3.977 * ONE))), h, w),
            "turn1": (turn, h, w),
            "quarter": ((0, ONE, 0, -ONE, 0, (w - 1) * ONE), w, h),
            "half": ((2 * ONE, 0, 0, 0, 2 * ONE, 0), h, w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    nbytes = n * h * w
    rng = np.random.default_rng(32)
    frame = rng.integers(0, 256, (h, w), dtype=np.uint8)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        d_src, d_out, d_valid = ctx.malloc(nbytes), ctx.malloc(nbytes), ctx.malloc(n * h * ((w + 7) // 8))
        for f in range(n):   # the same plane with a per-frame offset: a quarter-turned source has the same bytes
            ctx.h2d(d_src + f * h * w, (frame + f).astype(np.uint8))
        variants = []
        for name, (coef, sh, sw) in cases(h, w).items():
            rec = np.array([[1, f, *coef] for f in range(n)], np.int64)
            d_x = ctx.malloc(rec.nbytes)
            ctx.h2d(d_x, rec)
            for interp in (capi.WARP_NEAREST, capi.WARP_BILINEAR):
                for route in (capi.WARP_ROUTE_DIRECT, capi.WARP_ROUTE_TILED):
                    variants.append(dict(case=name, interp=interp, route=route, d_x=d_x, sh=sh, sw=sw, ms=[], copy=[]))

        def call(v):
            ctx.set_option("warp_route", v["route"])
            ctx.profile_reset()
            ctx.dev_warp_frames(d_src, n, v["sh"], v["sw"], v["d_x"], n, h, w, d_out, d_valid, v["interp"], 0)
            return ctx.warp_profile_get(capi.WARP_PARTS.index("warp"))[0]

        for v in variants:   # warm-up, and the share of valid pixels
            call(v)
            bits = np.empty(h * ((w + 7) // 8), np.uint8)
            ctx.d2h(bits, d_valid)
            v["valid"] = float(np.unpackbits(bits.reshape(h, -1), axis=1)[:, :w].mean())
        ctx.probe_copy(d_src, d_out, nbytes, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v))
                v["copy"].append(ctx.probe_copy(d_src, d_out, nbytes, args.calls))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms, copy = statistics.median(v["ms"]), statistics.median(v["copy"])
                line = dict(box=args.box, frames=n, height=h, width=w, case=v["case"],
                            interp=("nearest", "bilinear")[v["interp"]], route=("auto", "direct", "tiled")[v["route"]],
                            valid_share=v["valid"], calls=len(v["ms"]), warp_ms=stat(v["ms"]), copy_ms=stat(v["copy"]),
                            warp_over_copy=ms / copy if copy > 0 else 0.0, gpx_per_s=nbytes / (ms * 1e6) if ms > 0 else 0.0,
                            times="HIP events around the launch; the copy is canny_hip_probe_copy of the same bytes; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
