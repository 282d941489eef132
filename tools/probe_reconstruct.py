#!/usr/bin/env python3
"""Times the reconstruction (canny_hip_profile_part_get, group "reconstruct") on a batch of bit maps, under the stepwise route
and the tile flood:
  (a) FILL_HOLES and CLEAR_BORDER of the benchmark's synthetic frames binarized by OTSU,
  (b) SEEDED on the strong plane a dev_canny of those frames leaves in the context, every 97th edge pixel a marker,
  (c) SEEDED on blobs with a grid of markers 16 pixels apart,
  (d) the worst case, a full-frame zigzag seeded at its first pixel (tile flood only, one call),
  (f) the floor: SEEDED with an empty marker on (a)'s mask -- the init, one launch that stages every tile, three that every
      frame skips, the poll and the finish,
and beside each mask (e) canny_hip_dev_components_bits on it, the yardstick: a label pass answers the same question at 4 bytes
a pixel.  In the same rounds a plain device copy (canny_hip_probe_copy) of one bit-map batch.  HIP events around the call's
launches, one warm-up call per variant, then rounds that alternate over all variants; the stepwise route and the zigzag run
--slow-calls calls in all.  Appends one JSON line per variant to profiles/reconstruct.jsonl.

    python tools/probe_reconstruct.py [--frames 128] [--height 2160] [--width 3840] [--box NAME]
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

SIGMA, LO, HI = 1.4, 50, 150
ROUTES = (("stepwise", capi.RECON_ROUTE_STEPWISE), ("tiles", capi.RECON_ROUTE_TILES))


def zigzag(h, w):
    a = np.zeros((h, w), bool)
    a[:, 0::2] = True
    cols = np.arange(1, w - 1, 2)
    a[h - 1, cols[0::2]] = True
    a[0, cols[1::2]] = True
    return a


def blobs(h, w, seed):
    from scipy.ndimage import uniform_filter
    return uniform_filter(np.random.default_rng(seed).random((h, w)), 9) > 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--slow-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.jsonl"))
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width
    rb = (w + 7) // 8
    fpx, fbytes = h * w, h * rb
    distinct = min(n, 4)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_sample_interval", 1)
        ctx.set_option("profile_stage_mask", 0x7FFFFFFF)   # every group: the components have a bit of their own, the
        #                                                    parts behind the polygons go by bit 30
        d_frames, d_edges = ctx.malloc(n * fpx + 16), ctx.malloc(2 * n * fpx + 16)
        frames = [synth_frame(h, w, 42 + i) for i in range(distinct)]   # the benchmark's frames, in turn
        for f in range(n):
            ctx.h2d(d_frames + f * fpx, frames[f % distinct])
        d_out, d_info, d_copy = ctx.malloc(n * fbytes + 16), ctx.malloc(n * 24), ctx.malloc(n * fbytes + 16)
        d_labels, d_off = ctx.malloc(n * fpx * 4 + 16), ctx.malloc((n + 1) * 8)

        def upload(maps):
            """distinct bool [h, w] maps, in turn -> device bit maps of the batch"""
            d = ctx.malloc(n * fbytes + 16)
            packed = [np.packbits(m, axis=-1) for m in maps]
            for f in range(n):
                ctx.h2d(d + f * fbytes, packed[f % len(packed)])
            return d

        masks, markers = {}, {}   # name -> device bit maps; "strong": the context's strong plane
        masks["otsu"] = ctx.malloc(n * fbytes + 16)
        ctx.dev_binarize(d_frames, n, h, w, capi.BIN_OTSU, 0, masks["otsu"])
        markers["empty"] = upload([np.zeros((h, w), bool)])
        masks["strong"] = ctx.malloc(n * fbytes + 16)   # the same bits as the plane, for the label pass and the markers
        ctx.dev_canny_bits(d_frames, SIGMA, LO, HI, h, w, n, masks["strong"])
        edge_maps = []
        for i in range(distinct):
            bits = np.zeros(fbytes, np.uint8)
            ctx.d2h(bits, masks["strong"] + i * fbytes)
            e = np.unpackbits(bits.reshape(h, rb), axis=-1)[:, :w].astype(bool)
            k = np.zeros_like(e)
            k.reshape(-1)[np.flatnonzero(e)[::97]] = True
            edge_maps.append(k)
        markers["edges97"] = upload(edge_maps)
        blob_maps = [blobs(h, w, i) for i in range(distinct)]
        grid = np.zeros((h, w), bool)
        grid[::16, ::16] = True
        masks["blobs"], markers["grid16"] = upload(blob_maps), upload([m & grid for m in blob_maps])
        z = zigzag(h, w)
        first = np.zeros_like(z)
        first[0, 0] = True
        masks["zigzag"], markers["first"] = upload([z]), upload([first])
        ctx.dev_canny(d_frames, SIGMA, LO, HI, h, w, n, d_edges)   # leaves the strong plane; nothing below disturbs it
        ctx.synchronize()

        cases = [("a_fill", "otsu", None, capi.RECON_FILL_HOLES, False), ("a_clear", "otsu", None, capi.RECON_CLEAR_BORDER, False),
                 ("b_strong", "strong", "edges97", capi.RECON_SEEDED, False), ("c_blobs", "blobs", "grid16", capi.RECON_SEEDED, False),
                 ("d_zigzag", "zigzag", "first", capi.RECON_SEEDED, True), ("f_floor", "otsu", "empty", capi.RECON_SEEDED, False)]
        variants = []
        for case, mask, marker, op, tiles_only in cases:
            for route in ROUTES:
                if tiles_only and route[0] != "tiles":
                    continue
                slow = route[0] == "stepwise" or tiles_only
                variants.append(dict(kind="reconstruct", case=case, mask=mask, marker=marker, op=op, route=route, slow=slow, ms=[],
                                     parts=[], copy=[]))
        for mask in masks:
            variants.append(dict(kind="components", case="e_components", mask=mask, slow=False, ms=[], copy=[]))

        def call(v):
            ctx.profile_reset()
            if v["kind"] == "components":
                ctx.dev_components_bits(masks[v["mask"]], h, w, n, 1, d_labels, 0, 0, 0, d_off)
                return sum(ctx.components_profile_get(p)[0] for p in range(4)), None
            ctx.set_option("reconstruct_route", v["route"][1])
            d_marker = markers[v["marker"]] if v["marker"] else 0
            if v["mask"] == "strong":
                ctx.dev_canny_reconstruct(d_marker, n, h, w, v["op"], 8, d_out, d_info)
            else:
                ctx.dev_reconstruct_bits(d_marker, masks[v["mask"]], n, h, w, v["op"], 8, d_out, d_info)
            parts = [ctx.profile_part("reconstruct", p)[0] for p in range(2)]
            return sum(parts), parts

        for v in variants:   # warm-up (it counts as the one call of a slow variant); info says what the call did
            print("warm-up", v["case"], v["mask"], v.get("route", ("", 0))[0], flush=True)
            ms, parts = call(v)
            if v["kind"] == "reconstruct":
                info = np.zeros((n, 3), np.int64)
                ctx.d2h(info, d_info)
                v.update(launches=ctx.get_option("last_reconstruct_launches"), set_bits_out=int(info[:, 0].sum()),
                         set_bits_mask=int(info[:, 1].sum()), start=int(info[:, 2].sum()))
            if v["slow"]:
                v["ms"].append(ms), v["parts"].append(parts)
        ctx.probe_copy(d_out, d_copy, (n * fbytes) & ~15, 2)
        slow_left = args.slow_calls - 1
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in variants:
                if v["slow"] and rnd >= slow_left:
                    continue
                for _ in range(1 if v["slow"] else args.calls):
                    ms, parts = call(v)
                    v["ms"].append(ms)
                    if parts:
                        v["parts"].append(parts)
                v["copy"].append(ctx.probe_copy(d_out, d_copy, (n * fbytes) & ~15, args.calls))
        cp = statistics.median([c for v in variants for c in v["copy"]])
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in variants:
                ms = statistics.median(v["ms"])
                line = dict(box=args.box, frames=n, height=h, width=w, kind=v["kind"], case=v["case"], mask=v["mask"], connectivity=8,
                            calls=len(v["ms"]), ms=stat(v["ms"]), copy_ms=cp, over_copy=ms / cp if cp > 0 else 0.0)
                if v["kind"] == "reconstruct":
                    line.update(marker=v["marker"], op=capi.RECON_OPS[v["op"]], route=v["route"][0],
                                auto_route=capi.reconstruct_plan(n, h, w).aux, launches=v["launches"],
                                ms_sweeps=statistics.median(p[0] for p in v["parts"]),
                                ms_info=statistics.median(p[1] for p in v["parts"]), ms_per_launch=ms / v["launches"],
                                set_bits_out=v["set_bits_out"], set_bits_mask=v["set_bits_mask"], start=v["start"])
                line["times"] = ("HIP events around the call's launches (reconstruct: parts sweeps + info, the polls between the "
                                 "chunks included; components: its four parts); the copy is canny_hip_probe_copy of one bit-map "
                                 "batch, the median over all rounds; no counters")
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
