#!/usr/bin/env python3
"""Times the binary morphology (canny_hip_morph_profile_get) on a batch of random bit maps of two densities: ERODE and OPEN with
RECT 3 x 3, 7 x 7, 15 x 15 and 31 x 31 under both routes (general, separable), ELLIPSE 7 x 7 and 31 x 31 and a random 31 x 31
mask under the general route -- and beside each variant, in the same round, a plain device copy (canny_hip_probe_copy) of one
bit-map batch: a primitive step must read the batch once and write it once, which is what a copy of its bytes does, so the
yardstick of a call is that copy times its primitive steps.  HIP events around the call's launches, one warm-up call per
variant, then rounds that alternate over all variants; appends one JSON line per variant to profiles/morph.jsonl.

    python tools/probe_morph.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
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

ROUTES = ("auto", "general", "separable")


def elements():
    rng = np.random.default_rng(34)
    a = rng.random((31, 31)) < 0.5
    a[15, 15] = True
    rnd = np.array([sum(int(v) << i for i, v in enumerate(r)) for r in a], np.uint32)
    el = [("rect%dx%d" % (k, k), capi.morph_element(capi.MORPH_RECT, k), k, True) for k in (3, 7, 15, 31)]
    el += [("ellipse%dx%d" % (k, k), capi.morph_element(capi.MORPH_ELLIPSE, k), k, False) for k in (7, 31)]
    return el + [("random31x31", rnd, 31, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    fbytes = h * ((w + 7) // 8)
    nbytes = n * fbytes
    rng = np.random.default_rng(33)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        d_in = {}
        for density in (0.05, 0.5):
            d_in[density] = ctx.malloc(nbytes + 16)
            maps = [np.packbits(rng.random(fbytes * 8) < density) for _ in range(min(n, 8))]   # eight random maps, in turn
            for f in range(n):
                ctx.h2d(d_in[density] + f * fbytes, maps[f % len(maps)])
        d_out, d_counts = ctx.malloc(nbytes + 16), ctx.malloc(n * 8)
        variants = []
        for density in (0.05, 0.5):
            for op, steps in ((capi.MORPH_ERODE, 1), (capi.MORPH_OPEN, 2)):
                for name, rows, k, rect in elements():
                    for route in ((capi.MORPH_ROUTE_GENERAL, capi.MORPH_ROUTE_SEPARABLE) if rect else (capi.MORPH_ROUTE_GENERAL,)):
                        variants.append(dict(density=density, op=op, steps=steps, element=name, rows=rows, k=k, route=route, ms=[],
                                             copy=[], counts=None))

        def call(v):
            ctx.profile_reset()
            ctx.set_option("morph_route", v["route"])
            ctx.dev_morph_bits(d_in[v["density"]], n, h, w, v["op"], v["rows"], v["k"], v["k"], d_out, d_counts,
                               capi.MORPH_BORDER_NEUTRAL, 1)
            return ctx.morph_profile(0)[0]

        copy_bytes = nbytes & ~15
        for v in variants:   # warm-up; the counts of the output say that the call did its work
            call(v)
            c = np.zeros(n, np.int64)
            ctx.d2h(c, d_counts)
            v["counts"] = int(c.sum())
        ctx.probe_copy(d_in[0.5], d_out, copy_bytes, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v))
                v["copy"].append(ctx.probe_copy(d_in[v["density"]], d_out, copy_bytes, args.calls))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms, cp = statistics.median(v["ms"]), statistics.median(v["copy"]) * v["steps"]
                line = dict(box=args.box, frames=n, height=h, width=w, density=v["density"], op=capi.MORPH_OPS[v["op"]],
                            element=v["element"], route=ROUTES[v["route"]], steps=v["steps"], bytes_moved=2 * nbytes * v["steps"],
                            set_bits_out=v["counts"], calls=len(v["ms"]), ms=stat(v["ms"]), copy_ms_one_step=stat(v["copy"]),
                            over_copy=ms / cp if cp > 0 else 0.0, gb_per_s=2 * nbytes * v["steps"] / (ms * 1e6) if ms > 0 else 0.0,
                            times="HIP events around the call's launches; the copy is canny_hip_probe_copy of one bit-map batch, "
                                  "taken times the primitive steps; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
