#!/usr/bin/env python3
"""Times the thinning (canny_hip_profile_part_get, group "thin") on a batch of bit maps: the strong plane a dev_canny of the
benchmark's synthetic frames leaves in the context, the same frames binarized (OTSU), and a lattice of strokes 4, 8, 16 and 32
pixels thick -- GUOHALL to the fixed point (max_iterations = 0) under the stepwise route and the fused route at 1, 2, 4 and 8
full iterations a launch, and beside each variant, in the same round, a plain device copy (canny_hip_probe_copy) of one
bit-map batch: a sub-iteration cannot read and write less.  A second call with max_iterations = D + 1 runs the same iterations
with every launch queued up front and none that every frame skips: the difference is what the poll chunks cost.  HIP events
around the call's launches, one warm-up call per variant, then rounds that alternate over all variants; appends one JSON line
per variant to profiles/thin.jsonl.

    python tools/probe_thin.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
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
from canny_edge_amd.synth import synth_frame  # noqa: E402

SETTINGS = (("stepwise", capi.THIN_ROUTE_STEPWISE, 0), ("fused1", capi.THIN_ROUTE_FUSED, 1), ("fused2", capi.THIN_ROUTE_FUSED, 2),
            ("fused4", capi.THIN_ROUTE_FUSED, 4), ("fused8", capi.THIN_ROUTE_FUSED, 8), ("auto", capi.THIN_ROUTE_AUTO, 0))
THICKNESSES = (4, 8, 16, 32)
SIGMA, LO, HI = 1.4, 50, 150


def strokes(h, w, t, shift):
    """A lattice of horizontal and vertical strokes t thick, 4 t apart, moved by `shift` pixels."""
    yy, xx = np.mgrid[:h, :w]
    return ((yy + shift) % (4 * t) < t) | ((xx + 2 * shift) % (4 * t) < t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    fpx, fbytes = h * w, h * ((w + 7) // 8)
    distinct = min(n, 4)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        d_frames, d_edges = ctx.malloc(n * fpx + 16), ctx.malloc(2 * n * fpx + 16)
        frames = [synth_frame(h, w, 42 + i) for i in range(distinct)]   # the benchmark's frames, in turn
        for f in range(n):
            ctx.h2d(d_frames + f * fpx, frames[f % distinct])
        d_out, d_info, d_copy = ctx.malloc(n * fbytes + 16), ctx.malloc(n * 32), ctx.malloc(n * fbytes + 16)
        inputs = {"strong": None}   # name -> device bit maps; None: the context's strong plane
        inputs["binarized"] = ctx.malloc(n * fbytes + 16)
        ctx.dev_binarize(d_frames, n, h, w, capi.BIN_OTSU, 0, inputs["binarized"])
        for t in THICKNESSES:
            inputs["strokes%d" % t] = d = ctx.malloc(n * fbytes + 16)
            maps = [np.packbits(strokes(h, w, t, 3 * i), axis=-1) for i in range(distinct)]
            for f in range(n):
                ctx.h2d(d + f * fbytes, maps[f % distinct])
        ctx.dev_canny(d_frames, SIGMA, LO, HI, h, w, n, d_edges)   # leaves the strong plane; nothing below disturbs it
        ctx.synchronize()
        variants = [dict(input=name, setting=s, ms=[], ms_exact=[], copy=[]) for name in inputs for s in SETTINGS]

        def call(v, k):
            ctx.profile_reset()
            ctx.set_option("thin_route", v["setting"][1])
            ctx.set_option("thin_fuse", v["setting"][2])
            d = inputs[v["input"]]
            if d is None:
                ctx.dev_canny_thin(n, h, w, capi.THIN_GUOHALL, d_out, d_info, k)
            else:
                ctx.dev_thin_bits(d, n, h, w, capi.THIN_GUOHALL, d_out, d_info, k)
            parts = [ctx.profile_part("thin", p)[0] for p in range(2)]   # synchronises
            return sum(parts), parts

        for v in variants:   # warm-up; info says what the call did
            call(v, 0)
            info = np.zeros((n, 4), np.int64)
            ctx.d2h(info, d_info)
            v.update(iterations=int(info[:, 1].max()), set_bits_out=int(info[:, 0].sum()), deleted=int(info[:, 2].sum()))
            call(v, v["iterations"] + 1)
        ctx.probe_copy(d_out, d_copy, (n * fbytes) & ~15, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v, 0)[0])
                    v["ms_exact"].append(call(v, v["iterations"] + 1)[0])
                v["copy"].append(ctx.probe_copy(d_out, d_copy, (n * fbytes) & ~15, args.calls))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms, exact, cp = (statistics.median(v[key]) for key in ("ms", "ms_exact", "copy"))
                its = v["iterations"]
                line = dict(box=args.box, frames=n, height=h, width=w, method="guohall", input=v["input"], setting=v["setting"][0],
                            aux=capi.thin_plan(n, h, w).aux, iterations=its, set_bits_out=v["set_bits_out"], deleted=v["deleted"],
                            calls=len(v["ms"]), ms=stat(v["ms"]), ms_exact=stat(v["ms_exact"]),
                            ms_per_iteration=exact / (its + 1), skip_share=1.0 - exact / ms if ms > 0 else 0.0,
                            copy_ms=stat(v["copy"]), over_copy=ms / cp if cp > 0 else 0.0,
                            per_iteration_over_copy=exact / (its + 1) / cp if cp > 0 else 0.0,
                            times="HIP events around the call's launches (parts passes + info); ms: max_iterations = 0; ms_exact: "
                                  "max_iterations = iterations + 1, the same iterations queued up front; the copy is "
                                  "canny_hip_probe_copy of one bit-map batch; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
