#!/usr/bin/env python3
"""Edge curves on the benchmark's own shape (128 x 3840x2160 synth_batch, sigma 1.4, thresholds 50 / 150), device resident:
what the two parts cost behind dev_canny, for min_length 1 and 10.

HIP-event times via curves_profile_get (0 count, 1 write), "profile_stage_mask" set to their bit, in ONE process: ROUNDS
rounds of STEPS calls of dev_canny_curves after a warm-up, the variants alternating within each round.  Two yardsticks from
the same process: the dev_canny_contours call at min_area 1 (the sum of its four parts; section 17) and
canny_hip_probe_copy of 4 B/px.  Curves and points per frame and the longest curve of the batch are recorded, and the
single-thread tail on its own: the 1024 x 1024 serpentine (one open curve, its length checked against
canny_hip_curves_from_bits) through the bits route, whose count and write parts divided by the curve's length are the time
per point of one walking lane (the count part walks the curve from both ends, the write part three times: from both ends
for the lengths, once more to store).  Frame 0's curves are compared with the rule (tests/curves_rule.py) applied to the
s16 map of the same call.
    python tools/probe_curves.py [out.jsonl]   (one JSON line; appended to out.jsonl)"""
import json
import os
import socket
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 128, 2160, 3840
SIGMA, LO, HI = 1.4, 50, 150
ROUNDS, STEPS = 5, 3
MIN_LENGTHS = (1, 10)
PARTS = ("count", "write")
CONTOUR_PARTS = 4
CURVE_MASK, CONTOUR_MASK = 1 << 30, 0b1111 << 22


def _summary(vals):
    return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}


def main():
    import components_rule as cr
    import curves_rule as rule
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = capi.Context(0)
    px = N * H * W
    frames = synth_batch(N, H, W, seed=42, distinct=16)
    d_in, d_edges = ctx.malloc(px), ctx.malloc(px * 2)
    d_off, d_poff = ctx.malloc(8 * (N + 1)), ctx.malloc(8 * (N + 1))
    d_copy_src, d_copy_dst = ctx.malloc(px * 4), ctx.malloc(px * 4)
    ctx.h2d(d_in, frames)
    offsets, point_offsets = np.empty(N + 1, np.uint64), np.empty(N + 1, np.uint64)
    # counts first: the buffers are sized from them
    totals, point_totals = {}, {}
    for m in MIN_LENGTHS:
        ctx.dev_canny_curves(d_in, SIGMA, LO, HI, H, W, N, m, 0, 0, d_off, 0, 0, 0, d_poff, d_edges)
        ctx.d2h(offsets, d_off)
        ctx.d2h(point_offsets, d_poff)
        totals[m], point_totals[m] = int(offsets[-1]), int(point_offsets[-1])
    ctx.dev_canny_contours(d_in, SIGMA, LO, HI, H, W, N, 1, 0, 0, d_off, 0, 0, 0, d_poff, d_edges)
    ctx.d2h(offsets, d_off)
    ctx.d2h(point_offsets, d_poff)
    ct_total, ct_points = int(offsets[-1]), int(point_offsets[-1])
    K, P = max(totals[1], ct_total, 1), max(point_totals[1], ct_points, 1)
    d_rec, d_chain, d_points = ctx.malloc(24 * K), ctx.malloc(8 * (K + 1)), ctx.malloc(4 * P)

    def call(m):
        ctx.dev_canny_curves(d_in, SIGMA, LO, HI, H, W, N, m, d_rec, totals[m], d_off, d_chain, d_points, point_totals[m],
                             d_poff, d_edges)

    def contours_call(_):
        ctx.dev_canny_contours(d_in, SIGMA, LO, HI, H, W, N, 1, d_rec, ct_total, d_off, d_chain, d_points, ct_points, d_poff,
                               d_edges)

    def measure(fn, arg, mask, getter, parts):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.set_option("profile_stage_mask", mask)
        ctx.profile_enable(True)
        for _ in range(STEPS):
            fn(arg)
        ctx.synchronize()
        ms = [getter(p)[0] / STEPS for p in range(parts)]
        ctx.profile_enable(False)
        ctx.set_option("profile_stage_mask", 0)
        return ms

    for m in MIN_LENGTHS:  # warm-up: workspaces, code objects
        call(m)
    contours_call(0)
    rounds = {m: [] for m in MIN_LENGTHS}
    ct_rounds, copy = [], []
    for _ in range(ROUNDS):
        for m in MIN_LENGTHS:
            rounds[m].append(measure(call, m, CURVE_MASK, ctx.curves_profile_get, len(PARTS)))
        ct_rounds.append(sum(measure(contours_call, 0, CONTOUR_MASK, ctx.contours_profile_get, CONTOUR_PARTS)))
        copy.append(ctx.probe_copy(d_copy_src, d_copy_dst, px * 4, 5))

    # the timed output is the right one: frame 0 against the rule applied to the s16 map of the same call
    longest = {}
    for m in MIN_LENGTHS[::-1]:
        call(m)
        chain_all = np.empty(totals[m] + 1, np.uint64)
        ctx.d2h(chain_all, d_chain)
        longest[m] = int(np.diff(chain_all).max()) if totals[m] else 0
    edges0 = np.empty((H, W), np.int16)   # the last call was min_length 1
    ctx.d2h(edges0, d_edges)
    ctx.d2h(offsets, d_off)
    ctx.d2h(point_offsets, d_poff)
    k0, p0 = int(offsets[1]), int(point_offsets[1])
    rec0, chain0, points0 = np.empty(max(k0, 1) * 4, np.int32), np.empty(k0 + 1, np.uint64), np.empty(max(p0, 1), np.int32)
    ctx.d2h(rec0, d_rec)
    ctx.d2h(chain0, d_chain)
    ctx.d2h(points0, d_points)
    want = rule.csr(edges0[None], 1)
    same = bool(np.array_equal(chain0, want[2]) and np.array_equal(points0[:p0], want[3]) and p0 == want[3].size and
                np.array_equal(rec0[:k0 * 4].reshape(k0, 4), want[0]))
    flags0 = want[0][:, rule.FLAGS] if k0 else np.zeros(0, np.int32)

    # the single-thread tail: one open curve from corner to corner
    s = 1024
    serp = np.packbits(cr.serpentine(s, s), axis=-1)
    steps = capi.curves_from_bits(serp, s, s, 1, capacity=0, point_capacity=0)[4]
    d_bits, d_spts, d_sch = ctx.malloc(serp.nbytes), ctx.malloc(4 * steps), ctx.malloc(16)
    ctx.h2d(d_bits, serp)

    def serpentine_call(_):
        ctx.dev_curves_bits(d_bits, s, s, 1, 1, 0, 1, d_off, d_sch, d_spts, steps, d_poff)

    serpentine_call(0)
    ctx.d2h(point_offsets[:2], d_poff)
    serp_ok = int(point_offsets[1]) == steps
    serp_rounds = [measure(serpentine_call, 0, CURVE_MASK, ctx.curves_profile_get, len(PARTS)) for _ in range(ROUNDS)]
    serp_count, serp_write = [r[0] for r in serp_rounds], [r[1] for r in serp_rounds]

    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "thresholds": [LO, HI], "rounds": ROUNDS,
              "steps": STEPS, "host": socket.gethostname(),
              "curves_per_frame": {str(m): round(t / N, 1) for m, t in totals.items()},
              "curve_points_per_frame": {str(m): round(t / N, 1) for m, t in point_totals.items()},
              "contours_per_frame": round(ct_total / N, 1), "contour_points_per_frame": round(ct_points / N, 1),
              "longest_curve": {str(m): v for m, v in longest.items()},
              "frame0": {"curves": k0, "points": p0, "closed": int((flags0 & rule.CLOSED != 0).sum()),
                         "isolated": int((flags0 & rule.ISOLATED != 0).sum()),
                         "with_a_junction": int((flags0 & (rule.START_JUNCTION | rule.END_JUNCTION) != 0).sum())},
              "frame0_equals_the_rule": same,
              "contours_call_min_area_1_ms": _summary(ct_rounds),
              "copy_4B_per_px_ms": _summary(copy),
              "serpentine_1024": {"curve_points": steps, "length_is_right": serp_ok, "count_ms": _summary(serp_count),
                                  "write_ms": _summary(serp_write),
                                  "count_ns_per_point": round(statistics.median(serp_count) * 1e6 / steps, 1),
                                  "write_ns_per_point": round(statistics.median(serp_write) * 1e6 / steps, 1)}}
    for m in MIN_LENGTHS:
        for i, part in enumerate(PARTS):
            result[f"min{m}_{part}_ms"] = _summary([r[i] for r in rounds[m]])
        result[f"min{m}_total_ms"] = round(sum(result[f"min{m}_{p}_ms"]["median"] for p in PARTS), 4)
        result[f"min{m}_output_bytes"] = 16 * totals[m] + 8 * (totals[m] + 1) + 4 * point_totals[m] + 16 * (N + 1)
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    for p in (d_in, d_edges, d_off, d_poff, d_copy_src, d_copy_dst, d_rec, d_chain, d_points, d_bits, d_spts, d_sch):
        ctx.free(p)
    if not (same and serp_ok):
        raise SystemExit("frame 0's curves differ from the rule, or the serpentine's length is wrong")


if __name__ == "__main__":
    main()
