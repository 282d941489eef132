#!/usr/bin/env python3
"""Times the binarization (canny_hip_profile_part_get, group "binarize") on a batch of random u8 frames: FIXED, OTSU (its
three parts: histogram, select, map) and ADAPTIVE_MEAN with square windows of 3, 15, 31, 101 and 255 under both routes
(straightforward, marching) -- and beside each variant, in the same round, a plain device copy (canny_hip_probe_copy) that
moves the same number of bytes: a call must read the frames once (1 B a pixel) and write the bits once (1/8 B a pixel), so
the copy reads and writes 9/16 B a pixel.  HIP events around the call's launches, one warm-up call per variant, then rounds
that alternate over all variants; appends one JSON line per variant to profiles/binarize.jsonl.

The straightforward route costs kw * kh loads a pixel: from window 15 on it runs on the first frames of the batch only
(`frames_run`), fewer rounds, and `ms` is scaled to the whole batch (`scaled` says so).

    python tools/probe_binarize.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from canny_edge_amd import capi  # noqa: E402

ROUTES = ("auto", "direct", "march")
WINDOWS = (3, 15, 31, 101, 255)
DIRECT_FRAMES = {3: 128, 15: 16, 31: 4, 101: 1, 255: 1}   # at most this many frames under the straightforward route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binarize.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    fpx, fbytes = h * w, h * ((w + 7) // 8)
    rng = np.random.default_rng(36)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        d_in = ctx.malloc(n * fpx + 16)
        frames = [rng.integers(0, 256, fpx, dtype=np.uint8) for _ in range(min(n, 8))]   # eight random frames, in turn
        for f in range(n):
            ctx.h2d(d_in + f * fpx, frames[f % len(frames)])
        d_out, d_counts, d_thr = ctx.malloc(n * fbytes + 16), ctx.malloc(n * 8), ctx.malloc(n * 4)
        d_copy = ctx.malloc(n * fpx + 16)
        variants = [dict(method=capi.BIN_FIXED, c=127, k=3, route=0, frames=n), dict(method=capi.BIN_OTSU, c=0, k=3, route=0, frames=n)]
        for k in WINDOWS:
            variants.append(dict(method=capi.BIN_ADAPTIVE_MEAN, c=7, k=k, route=capi.BIN_ROUTE_MARCH, frames=n))
            variants.append(dict(method=capi.BIN_ADAPTIVE_MEAN, c=7, k=k, route=capi.BIN_ROUTE_DIRECT, frames=min(n, DIRECT_FRAMES[k])))
        for v in variants:
            v.update(ms=[], parts=[], copy=[], counts=None, slow=v["route"] == capi.BIN_ROUTE_DIRECT and v["k"] >= 15)

        def call(v):
            ctx.profile_reset()
            ctx.set_option("binarize_route", v["route"])
            ctx.dev_binarize(d_in, v["frames"], h, w, v["method"], v["c"], d_out, d_counts, d_thr, v["k"], v["k"], 0)
            parts = [ctx.profile_part("binarize", p)[0] for p in range(3)]
            return sum(parts), parts

        def copy_of(v, launches):
            nbytes = (v["frames"] * (fpx + fbytes) // 2) & ~15
            return ctx.probe_copy(d_in, d_copy, nbytes, launches)

        for v in variants:   # warm-up; the counts of the output say that the call did its work
            call(v)
            c = np.zeros(v["frames"], np.int64)
            ctx.d2h(c, d_counts)
            v["counts"] = int(c.sum())
        copy_of(variants[0], 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                if v["slow"] and rnd >= 2:
                    continue
                for _ in range(1 if v["slow"] else args.calls):
                    ms, parts = call(v)
                    v["ms"].append(ms)
                    v["parts"].append(parts)
                v["copy"].append(copy_of(v, args.calls))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                scale = n / v["frames"]
                ms, cp = statistics.median(v["ms"]) * scale, statistics.median(v["copy"]) * scale
                moved = n * (fpx + fbytes)
                line = dict(box=args.box, frames=n, height=h, width=w, method=capi.BIN_METHODS[v["method"]], window=v["k"],
                            route=ROUTES[v["route"]], frames_run=v["frames"], scaled=v["frames"] != n, bytes_moved=moved,
                            set_bits_out=v["counts"], calls=len(v["ms"]), ms=stat([x * scale for x in v["ms"]]),
                            parts_ms=dict(zip(capi.BIN_PARTS, (statistics.median(p[i] for p in v["parts"]) * scale for i in range(3)))),
                            copy_ms=stat([x * scale for x in v["copy"]]), over_copy=ms / cp if cp > 0 else 0.0,
                            gb_per_s=moved / (ms * 1e6) if ms > 0 else 0.0,
                            times="HIP events around the call's launches; the copy is canny_hip_probe_copy of (pixels + bit bytes) "
                                  "/ 2 bytes of the frames that ran; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
