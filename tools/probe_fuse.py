#!/usr/bin/env python3
"""Times the temporal fusion (canny_hip_fuse_profile_get) on a stack of random frames: every op over disjoint groups of 4, 8,
16, 32 and 64 frames, with and without valid bit maps, the MEDIAN under both routes wherever both exist, and the change mask
alone -- and beside each variant, in the same round, a plain device copy (canny_hip_probe_copy) that moves the same number of
bytes the call must move (frames + valid bits in, fused + count out; a copy of N bytes reads N and writes N, so N is half of
that sum, rounded down to 16 bytes): the yardstick.  The mask is taken against the planes and counts that the last fuse
variant left in its buffers (random frames: nearly every valid pixel differs by more than the threshold, so the set-bit
density is high and arbitrary; it is what the ballots and the adds to `changed` see).  HIP events around the launch, one
warm-up call per variant, then rounds that alternate over all variants; appends one JSON line per variant to
profiles/fuse.jsonl.

    python tools/probe_fuse.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
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

OPS = ("mean", "median", "min", "max")
ROUTES = ("auto", "registers", "passes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--groups", default="4,8,16,32,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    plane, vplane = h * w, h * ((w + 7) // 8)
    rng = np.random.default_rng(33)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        lens = [int(g) for g in args.groups.split(",") if int(g) <= n]
        # the largest yardstick copy: every frame and bit map in, two planes a group out, halved; the frames' buffer is its
        # source and is allocated that long (the tail is never initialised and only ever copied)
        copy_bytes = (n * (plane + vplane) + 2 * max([n // g for g in lens] + [n]) * plane) // 2 + 16
        d_frames, d_valid = ctx.malloc(max(n * plane, copy_bytes)), ctx.malloc(n * vplane)
        out_planes = max([n // g for g in lens] + [-(-n // min(16, n))])   # the most groups of any variant; the mask's planes
        d_fused, d_count = ctx.malloc(out_planes * plane + 16), ctx.malloc(out_planes * plane + 16)
        d_mask, d_changed, d_copy = ctx.malloc(n * vplane), ctx.malloc(n * 8), ctx.malloc(max(n * plane, copy_bytes))
        for f in range(n):   # independent random frames and bit maps (about 3 in 4 pixels valid)
            ctx.h2d(d_frames + f * plane, rng.integers(0, 256, plane, dtype=np.uint8))
            ctx.h2d(d_valid + f * vplane, rng.integers(0, 256, vplane, dtype=np.uint8) | rng.integers(0, 256, vplane, dtype=np.uint8))
        variants = []
        for group_len in lens:
            groups = n // group_len
            for valid in (False, True):
                moved = groups * group_len * (plane + (vplane if valid else 0)) + 2 * groups * plane
                for op in range(4):
                    both = op == capi.FUSE_MEDIAN and group_len <= 32
                    for route in ((capi.FUSE_ROUTE_REGISTERS, capi.FUSE_ROUTE_PASSES) if both else (capi.FUSE_ROUTE_AUTO,)):
                        variants.append(dict(what="fuse", op=op, group_len=group_len, valid=valid, route=route, moved=moved,
                                             ms=[], copy=[]))
        for valid in (False, True):   # the mask of every frame against one plane per 16 frames, with its counts
            per = min(16, n)
            moved = n * (plane + (vplane if valid else 0)) + 2 * -(-n // per) * plane + n * vplane
            variants.append(dict(what="mask", op=-1, group_len=per, valid=valid, route=0, moved=moved, ms=[], copy=[]))

        def call(v):
            ctx.profile_reset()
            if v["what"] == "fuse":
                ctx.set_option("fuse_route", v["route"])
                ctx.dev_fuse_frames(d_frames, d_valid if v["valid"] else 0, n, h, w, v["group_len"], v["group_len"], d_fused,
                                    d_count, v["op"], 0, 1)
                return ctx.fuse_profile("fuse")[0]
            ctx.dev_change_mask(d_frames, d_valid if v["valid"] else 0, n, h, w, d_fused, d_count, v["group_len"], d_mask,
                                d_changed, 40, 1)
            return ctx.fuse_profile("mask")[0]

        def copy(v):
            assert v["moved"] // 2 <= copy_bytes
            return ctx.probe_copy(d_frames, d_copy, (v["moved"] // 2) & ~15, args.calls)

        for v in variants:   # warm-up
            call(v)
        ctx.probe_copy(d_frames, d_copy, n * plane // 2, 2)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                for _ in range(args.calls):
                    v["ms"].append(call(v))
                v["copy"].append(copy(v))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms, cp = statistics.median(v["ms"]), statistics.median(v["copy"])
                line = dict(box=args.box, frames=n, height=h, width=w, what=v["what"],
                            op=OPS[v["op"]] if v["op"] >= 0 else "mask", group_len=v["group_len"], valid_bits=v["valid"],
                            route=ROUTES[v["route"]], bytes_moved=v["moved"], calls=len(v["ms"]), ms=stat(v["ms"]),
                            copy_ms=stat(v["copy"]), over_copy=ms / cp if cp > 0 else 0.0,
                            gb_per_s=v["moved"] / (ms * 1e6) if ms > 0 else 0.0,
                            times="HIP events around the launch; the copy is canny_hip_probe_copy of bytes_moved / 2; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
