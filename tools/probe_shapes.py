#!/usr/bin/env python3
"""Contour shape measures on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150),
device resident: what the three parts cost behind the contours call, for min_area 1 and 20.

HIP-event times via shapes_profile_get (0 measure, 1 scan, 2 emit) and, as the yardstick in the same process,
polygons_profile_get (0 simplify, 1 scan, 2 emit; ratio_q16 1311) and contours_profile_get (0 label, 1 count, 2 write, 3
stats; count and write are the two chain walks): "profile_stage_mask" is set to those slots, ROUNDS rounds of STEPS calls
of dev_canny_shapes and of dev_canny_polygons after a warm-up, the variants alternating within each round -- 15 calls per
figure.  Reported besides: the shapes stage as a multiple of one chain walk and of the polygons sum, the hull vertices per
frame, the bytes of shape output against the bytes of chain points, and the one-wave-per-chain tail on its own: the 1024 x
1024 serpentine (one chain of 1024^2 - 1 points) through dev_shapes_bits.  Frame 0's shapes are compared with
canny_hip_shapes_from_chains applied to the chains of the same call.
    python tools/probe_shapes.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
EPS_Q8, RATIO_Q16 = 0, 1311
ROUNDS, STEPS = 5, 3
MIN_AREAS = (1, 20)
CONTOUR_PARTS = ("label", "count", "write", "stats")
POLYGON_PARTS = ("simplify", "scan", "emit")
SHAPE_PARTS = ("measure", "scan", "emit")
MASK = (0b1111 << 22) | (1 << 30)
WORDS = 20


def _summary(vals):
    return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}


def main():
    import components_rule as cr
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_off, d_poff = ctx.malloc(8 * (N + 1)), ctx.malloc(8 * (N + 1))
    ctx.h2d(d_in, frames)
    offsets, point_offsets = np.empty(N + 1, np.uint64), np.empty(N + 1, np.uint64)
    totals, point_totals = {}, {}
    for min_area in MIN_AREAS:   # counts first: the buffers are sized from them
        ctx.dev_canny_contours(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, 0, d_off, 0, 0, 0, d_poff, d_edges)
        ctx.d2h(offsets, d_off)
        ctx.d2h(point_offsets, d_poff)
        totals[min_area], point_totals[min_area] = int(offsets[-1]), int(point_offsets[-1])
    K, P = max(totals[1], 1), max(point_totals[1], 1)
    d_chain, d_points = ctx.malloc(8 * (K + 1)), ctx.malloc(4 * P)
    d_hoff, d_hull, d_meas = ctx.malloc(8 * (K + 1)), ctx.malloc(4 * P), ctx.malloc(8 * WORDS * K)

    def shapes(min_area):
        ctx.dev_canny_shapes(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, totals[min_area], d_off, d_chain, d_points,
                             point_totals[min_area], d_poff, d_hoff, d_hull, point_totals[min_area], d_meas, d_edges)

    def polygons(min_area):   # the yardstick writes into the same buffers: 4 words per record fit into 20
        ctx.dev_canny_polygons(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, totals[min_area], d_off, d_chain, d_points,
                               point_totals[min_area], d_poff, EPS_Q8, RATIO_Q16, d_hoff, d_hull, point_totals[min_area],
                               d_meas, d_edges)

    def measure(fn, arg, steps=STEPS):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", MASK)
        ctx.profile_enable(True)
        for _ in range(steps):
            fn(arg)
        ctx.synchronize()
        ms = ([ctx.contours_profile_get(p)[0] / steps for p in range(4)],
              [ctx.polygons_profile_get(p)[0] / steps for p in range(3)],
              [ctx.shapes_profile_get(p)[0] / steps for p in range(3)])
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for m in MIN_AREAS:   # warm-up: workspaces, code objects
        shapes(m)
        polygons(m)
    rounds = {m: [] for m in MIN_AREAS}
    for _ in range(ROUNDS):
        for m in MIN_AREAS:
            s, p = measure(shapes, m), measure(polygons, m)
            rounds[m].append((s[0], p[1], s[2]))

    # the timed output is the right one: frame 0 against the host rule applied to the chains of the same call
    hull_totals, same = {}, True
    for m in MIN_AREAS:
        shapes(m)
        ctx.d2h(offsets, d_off)
        k_all, k0 = int(offsets[-1]), int(offsets[1])
        hoff = np.empty(k_all + 1, np.uint64)
        ctx.d2h(hoff, d_hoff)
        hull_totals[m] = int(hoff[-1])
        chain0 = np.empty(k0 + 1, np.uint64)
        ctx.d2h(chain0, d_chain)
        points0, hull0 = np.empty(max(int(chain0[-1]), 1), np.int32), np.empty(max(int(hoff[k0]), 1), np.int32)
        meas0 = np.empty((max(k0, 1), WORDS), np.int64)
        ctx.d2h(points0, d_points)
        ctx.d2h(hull0, d_hull)
        ctx.d2h(meas0, d_meas)
        w_hoff, w_hull, w_meas = capi.shapes_from_chains(chain0, points0[:int(chain0[-1])], W, H)
        same = same and bool(np.array_equal(hoff[:k0 + 1], w_hoff) and np.array_equal(hull0[:int(hoff[k0])], w_hull)
                             and np.array_equal(meas0[:k0], w_meas))

    # the one-wave-per-chain tail
    s = 1024
    serp = np.packbits(cr.serpentine(s, s), axis=-1)
    steps = capi.contours_from_bits(serp, s, s, 1, capacity=0, point_capacity=0)[4]
    d_bits, d_spts, d_sch = ctx.malloc(serp.nbytes), ctx.malloc(4 * steps), ctx.malloc(16)
    d_shoff, d_shull, d_smeas = ctx.malloc(16), ctx.malloc(4 * steps), ctx.malloc(8 * WORDS)
    ctx.h2d(d_bits, serp)

    def serpentine_call(_):
        ctx.dev_shapes_bits(d_bits, s, s, 1, 1, 0, 1, d_off, d_sch, d_spts, steps, d_poff, d_shoff, d_shull, steps, d_smeas)

    serpentine_call(None)
    meas = np.empty(WORDS, np.int64)
    ctx.d2h(meas, d_smeas)
    got = [measure(serpentine_call, None, steps=1) for _ in range(ROUNDS)]
    serpentine = {"chain_points": steps, "hull_vertices": int(meas[0]), "s20": int(meas[11]),
                  "contours_count_ms": _summary([g[0][1] for g in got]),
                  "contours_write_ms": _summary([g[0][2] for g in got])}
    for i, part in enumerate(SHAPE_PARTS):
        serpentine[f"{part}_ms"] = _summary([g[2][i] for g in got])

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(),
              "components_per_frame": {str(m): round(t / N, 1) for m, t in totals.items()},
              "chain_points_per_frame": {str(m): round(t / N, 1) for m, t in point_totals.items()},
              "hull_vertices_per_frame": {str(m): round(t / N, 1) for m, t in hull_totals.items()},
              "frame0_equals_the_host_rule": same, "serpentine_1024": serpentine}
    for m in MIN_AREAS:
        for i, part in enumerate(CONTOUR_PARTS):
            result[f"min{m}_contours_{part}_ms"] = _summary([r[0][i] for r in rounds[m]])
        for i, part in enumerate(POLYGON_PARTS):
            result[f"min{m}_polygons_{part}_ms"] = _summary([r[1][i] for r in rounds[m]])
        for i, part in enumerate(SHAPE_PARTS):
            result[f"min{m}_{part}_ms"] = _summary([r[2][i] for r in rounds[m]])
        total = sum(result[f"min{m}_{p}_ms"]["median"] for p in SHAPE_PARTS)
        pg = sum(result[f"min{m}_polygons_{p}_ms"]["median"] for p in POLYGON_PARTS)
        walk = result[f"min{m}_contours_write_ms"]["median"]
        result[f"min{m}_shapes_total_ms"] = round(total, 4)
        result[f"min{m}_polygons_total_ms"] = round(pg, 4)
        result[f"min{m}_shapes_over_one_walk"] = round(total / walk, 3) if walk else None
        result[f"min{m}_shapes_over_polygons"] = round(total / pg, 3) if pg else None
        result[f"min{m}_shape_output_bytes"] = 4 * hull_totals[m] + 8 * (totals[m] + 1) + 8 * WORDS * totals[m]
        result[f"min{m}_chain_point_bytes"] = 4 * point_totals[m]
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_off, d_poff, d_chain, d_points, d_hoff, d_hull, d_meas, d_bits, d_spts, d_sch, d_shoff,
              d_shull, d_smeas):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's shapes differ from the host rule")


if __name__ == "__main__":
    main()
