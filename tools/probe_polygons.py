#!/usr/bin/env python3
"""Polygon approximation of the contour chains on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4,
thresholds 50 / 150, ratio_q16 1311 = 0.02 of the chain's length), device resident: what the three parts cost behind the
contours call, for min_area 1 and 20.

HIP-event times via polygons_profile_get (0 simplify, 1 scan, 2 emit) and, from the same calls, contours_profile_get (0
label, 1 count, 2 write, 3 stats) as the yardstick: "profile_stage_mask" is set to those slots, in ONE process, ROUNDS rounds
of STEPS calls of dev_canny_polygons after a warm-up, the variants alternating within each round.  Reported besides: the
vertices per frame, the bytes of polygon output against the bytes of chain points, and the one-wave-per-chain tail on its
own: the 1024 x 1024 serpentine (one chain of 1024^2 - 1 points) through dev_polygons_bits, at the call's own ratio (where
the tolerance reaches its cap and two vertices remain) and at one pixel absolute (where every turning point is a vertex).
Frame 0's polygons are compared with canny_hip_polygons_from_chains applied to the chains of the same call.
    python tools/probe_polygons.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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
MASK = (0b1111 << 22) | (1 << 30)


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
    d_voff, d_verts, d_meas = ctx.malloc(8 * (K + 1)), ctx.malloc(4 * P), ctx.malloc(32 * K)

    def call(min_area):
        ctx.dev_canny_polygons(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, totals[min_area], d_off, d_chain, d_points,
                               point_totals[min_area], d_poff, EPS_Q8, RATIO_Q16, d_voff, d_verts, point_totals[min_area],
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
              [ctx.polygons_profile_get(p)[0] / steps for p in range(3)])
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for m in MIN_AREAS:   # warm-up: workspaces, code objects
        call(m)
    rounds = {m: [] for m in MIN_AREAS}
    for _ in range(ROUNDS):
        for m in MIN_AREAS:
            rounds[m].append(measure(call, m))

    # the timed output is the right one: frame 0 against the host rule applied to the chains of the same call
    vertex_totals, same = {}, True
    for m in MIN_AREAS:
        call(m)
        ctx.d2h(offsets, d_off)
        k_all, k0 = int(offsets[-1]), int(offsets[1])
        voff = np.empty(k_all + 1, np.uint64)
        ctx.d2h(voff, d_voff)
        vertex_totals[m] = int(voff[-1])
        chain0 = np.empty(k0 + 1, np.uint64)
        ctx.d2h(chain0, d_chain)
        points0, verts0 = np.empty(max(int(chain0[-1]), 1), np.int32), np.empty(max(int(voff[k0]), 1), np.int32)
        meas0 = np.empty((max(k0, 1), 4), np.int64)
        ctx.d2h(points0, d_points)
        ctx.d2h(verts0, d_verts)
        ctx.d2h(meas0, d_meas)
        w_voff, w_verts, w_meas = capi.polygons_from_chains(chain0, points0[:int(chain0[-1])], W, H, EPS_Q8, RATIO_Q16)
        same = same and bool(np.array_equal(voff[:k0 + 1], w_voff) and np.array_equal(verts0[:int(voff[k0])], w_verts)
                             and np.array_equal(meas0[:k0], w_meas))

    # the one-wave-per-chain tail
    s = 1024
    serp = np.packbits(cr.serpentine(s, s), axis=-1)
    steps = capi.contours_from_bits(serp, s, s, 1, capacity=0, point_capacity=0)[4]
    d_bits, d_spts, d_sch = ctx.malloc(serp.nbytes), ctx.malloc(4 * steps), ctx.malloc(16)
    d_svoff, d_sverts, d_smeas = ctx.malloc(16), ctx.malloc(4 * steps), ctx.malloc(32)
    ctx.h2d(d_bits, serp)

    def serpentine_call(tol):
        ctx.dev_polygons_bits(d_bits, s, s, 1, 1, 0, 1, d_off, d_sch, d_spts, steps, d_poff, tol[0], tol[1], d_svoff,
                              d_sverts, steps, d_smeas)

    serpentine = {"chain_points": steps}
    for name, tol, n_rounds in (("ratio_0.02", (EPS_Q8, RATIO_Q16), ROUNDS), ("epsilon_1px", (256, 0), 2)):
        serpentine_call(tol)
        meas = np.empty(4, np.int64)
        ctx.d2h(meas, d_smeas)
        got = [measure(serpentine_call, tol, steps=1) for _ in range(n_rounds)]
        serpentine[name] = {"vertices": int(meas[0]), "length_q8": int(meas[1]),
                            "contours_count_ms": _summary([g[0][1] for g in got]),
                            "contours_write_ms": _summary([g[0][2] for g in got])}
        for i, part in enumerate(POLYGON_PARTS):
            serpentine[name][f"{part}_ms"] = _summary([g[1][i] for g in got])

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "epsilon_q8": EPS_Q8,
              "ratio_q16": RATIO_Q16, "rounds": ROUNDS, "steps": STEPS, "host": socket.gethostname(),
              "components_per_frame": {str(m): round(t / N, 1) for m, t in totals.items()},
              "chain_points_per_frame": {str(m): round(t / N, 1) for m, t in point_totals.items()},
              "vertices_per_frame": {str(m): round(t / N, 1) for m, t in vertex_totals.items()},
              "frame0_equals_the_host_rule": same, "serpentine_1024": serpentine}
    for m in MIN_AREAS:
        for i, part in enumerate(CONTOUR_PARTS):
            result[f"min{m}_contours_{part}_ms"] = _summary([r[0][i] for r in rounds[m]])
        for i, part in enumerate(POLYGON_PARTS):
            result[f"min{m}_{part}_ms"] = _summary([r[1][i] for r in rounds[m]])
        result[f"min{m}_polygons_total_ms"] = round(sum(result[f"min{m}_{p}_ms"]["median"] for p in POLYGON_PARTS), 4)
        result[f"min{m}_contours_total_ms"] = round(sum(result[f"min{m}_contours_{p}_ms"]["median"] for p in CONTOUR_PARTS), 4)
        result[f"min{m}_polygon_output_bytes"] = 4 * vertex_totals[m] + 8 * (totals[m] + 1) + 32 * totals[m]
        result[f"min{m}_chain_point_bytes"] = 4 * point_totals[m]
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_off, d_poff, d_chain, d_points, d_voff, d_verts, d_meas, d_bits, d_spts, d_sch, d_svoff,
              d_sverts, d_smeas):
        ctx.free(p)
    if not same:
        raise SystemExit("frame 0's polygons differ from the host rule")


if __name__ == "__main__":
    main()
