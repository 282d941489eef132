#!/usr/bin/env python3
"""Outer contour chains on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device
resident: what the four parts cost behind dev_canny, for min_area 1 and 20.

HIP-event times via contours_profile_get (0 label, 1 count, 2 write, 3 stats), "profile_stage_mask" set to those four
slots, in ONE process: ROUNDS rounds of STEPS calls of dev_canny_contours after a warm-up, the variants alternating within
each round.  Two yardsticks from the same process, the ones section 14 used: the dev_canny_components call without a label
plane (records + filtered map; the sum of its four parts) and canny_hip_probe_copy of 4 B/px.  The longest chain of the
batch is recorded, and the single-thread tail on its own: the 1024 x 1024 serpentine (one chain of 1024^2 - 1 points, its
length checked against canny_hip_contours_from_bits) through the bits route, whose count and write parts divided by the
chain length are the time per step of one walking thread.  Frame 0's chains are compared with the rule
(tests/contours_rule.py) applied to the s16 map of the same call.
    python tools/probe_contours.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
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
ROUNDS, STEPS = 5, 3
MIN_AREAS = (1, 20)
PARTS = ("label", "count", "write", "stats")
CONTOUR_MASK, CC_MASK = 0b1111 << 22, 0b1111 << 13


def _summary(vals):
    return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}


def main():
    import components_rule as cr
    import contours_rule as rule
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges, d_kept = ctx.malloc(px), ctx.malloc(px * 2), ctx.malloc(px)
    d_off, d_poff = ctx.malloc(8 * (N + 1)), ctx.malloc(8 * (N + 1))
    d_copy_src, d_copy_dst = ctx.malloc(px * 4), ctx.malloc(px * 4)
    ctx.h2d(d_in, frames)
    offsets, point_offsets = np.empty(N + 1, np.uint64), np.empty(N + 1, np.uint64)
    # counts first: the buffers are sized from them
    totals, point_totals = {}, {}
    for min_area in MIN_AREAS:
        ctx.dev_canny_contours(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, 0, d_off, 0, 0, 0, d_poff, d_edges)
        ctx.d2h(offsets, d_off)
        ctx.d2h(point_offsets, d_poff)
        totals[min_area], point_totals[min_area] = int(offsets[-1]), int(point_offsets[-1])
    K, P = max(totals[1], 1), max(point_totals[1], 1)
    d_stats, d_chain, d_points = ctx.malloc(24 * K), ctx.malloc(8 * (K + 1)), ctx.malloc(4 * P)

    def call(min_area):
        ctx.dev_canny_contours(d_in, SIGMA, LO, HI, H, W, N, min_area, d_stats, totals[min_area], d_off, d_chain, d_points,
                               point_totals[min_area], d_poff, d_edges)

    def components_call(min_area):
        ctx.dev_canny_components(d_in, SIGMA, LO, HI, H, W, N, min_area, 0, d_kept, d_stats, totals[min_area], d_off,
                                 d_edges)

    def measure(fn, arg, mask, getter):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", mask)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            fn(arg)
        ctx.synchronize()
        ms = [getter(p)[0] / STEPS for p in range(4)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for m in MIN_AREAS:  # warm-up: workspaces, code objects
        call(m)
        components_call(m)
    rounds = {m: [] for m in MIN_AREAS}
    cc_rounds = {m: [] for m in MIN_AREAS}
    copy = []
    for _ in range(ROUNDS):
        for m in MIN_AREAS:
            rounds[m].append(measure(call, m, CONTOUR_MASK, ctx.contours_profile_get))
            cc_rounds[m].append(sum(measure(components_call, m, CC_MASK, ctx.components_profile_get)))
        copy.append(ctx.probe_copy(d_copy_src, d_copy_dst, px * 4, 5))

    # the timed output is the right one: frame 0 against the rule applied to the s16 map of the same call
    call(20)
    edges0 = np.empty((H, W), np.int16)
    ctx.d2h(edges0, d_edges)
    ctx.d2h(offsets, d_off)
    ctx.d2h(point_offsets, d_poff)
    k0, p0 = int(offsets[1]), int(point_offsets[1])
    chain0, points0 = np.empty(k0 + 1, np.uint64), np.empty(max(p0, 1), np.int32)
    ctx.d2h(chain0, d_chain)
    ctx.d2h(points0, d_points)
    want = rule.csr(edges0[None], 20)
    same = bool(np.array_equal(chain0, want[2]) and np.array_equal(points0[:p0], want[3]) and p0 == want[3].size)
    chain_all = np.empty(totals[20] + 1, np.uint64)
    ctx.d2h(chain_all, d_chain)
    longest20 = int(np.diff(chain_all).max()) if totals[20] else 0
    call(1)
    chain_all = np.empty(totals[1] + 1, np.uint64)
    ctx.d2h(chain_all, d_chain)
    longest1 = int(np.diff(chain_all).max()) if totals[1] else 0

    # the single-thread tail: one chain, walked out and back
    s = 1024
    serp = np.packbits(cr.serpentine(s, s), axis=-1)
    steps = capi.contours_from_bits(serp, s, s, 1, capacity=0, point_capacity=0)[4]
    d_bits, d_spts, d_sch = ctx.malloc(serp.nbytes), ctx.malloc(4 * steps), ctx.malloc(16)
    ctx.h2d(d_bits, serp)

    def serpentine_call(_):
        ctx.dev_contours_bits(d_bits, s, s, 1, 1, 0, 1, d_off, d_sch, d_spts, steps, d_poff)

    serpentine_call(0)
    ctx.d2h(point_offsets[:2], d_poff)
    serp_ok = int(point_offsets[1]) == steps
    serp_rounds = [measure(serpentine_call, 0, CONTOUR_MASK, ctx.contours_profile_get) for _ in range(ROUNDS)]
    serp_count, serp_write = [r[1] for r in serp_rounds], [r[2] for r in serp_rounds]

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(),
              "components_per_frame": {str(m): round(t / N, 1) for m, t in totals.items()},
              "chain_points_per_frame": {str(m): round(t / N, 1) for m, t in point_totals.items()},
              "longest_chain": {"1": longest1, "20": longest20},
              "frame0_equals_the_rule": same,
              "copy_4B_per_px_ms": _summary(copy),
              "serpentine_1024": {"chain_points": steps, "length_is_right": serp_ok, "count_ms": _summary(serp_count),
                                  "write_ms": _summary(serp_write),
                                  "count_ns_per_step": round(statistics.median(serp_count) * 1e6 / steps, 1),
                                  "write_ns_per_step": round(statistics.median(serp_write) * 1e6 / steps, 1)}}
    for m in MIN_AREAS:
        for i, part in enumerate(PARTS):
            result[f"min{m}_{part}_ms"] = _summary([r[i] for r in rounds[m]])
        result[f"min{m}_total_ms"] = round(sum(result[f"min{m}_{p}_ms"]["median"] for p in PARTS), 4)
        result[f"min{m}_components_call_ms"] = _summary(cc_rounds[m])
        result[f"min{m}_output_bytes"] = 24 * totals[m] + 8 * (totals[m] + 1) + 4 * point_totals[m] + 16 * (N + 1)
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_kept, d_off, d_poff, d_copy_src, d_copy_dst, d_stats, d_chain, d_points, d_bits, d_spts,
              d_sch):
        ctx.free(p)
    if not (same and serp_ok):
        raise SystemExit("frame 0's chains differ from the rule, or the serpentine's length is wrong")


if __name__ == "__main__":
    main()
