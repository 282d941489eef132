#!/usr/bin/env python3
"""Times the three parts of the motion estimate (canny_hip_motion_profile_get) on synthetic batches: 127 consecutive pairs
of 128 frames, every query slot a correspondence, 70 % of them following a similarity.  Beside it, for scale, the matcher's
forward launch (CANNY_HIP_DESC_PART_MATCH) on random descriptor sets of the same batch shape, in the same run.  HIP events
around each part's launches, one warm-up call, then rounds x calls; appends one JSON line per case to profiles/motion.jsonl.

    python tools/probe_motion.py [--frames 128] [--box NAME]
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

CASES = ((256, 1024), (4096, 4096))  # (correspondences per pair, hypotheses)


def batch(rng, n, count):
    """Records [n, count, 4], every frame the one before under (x, y) -> (x + 3, y + 2) turned a little, 30 % replaced; the
    match rows [n - 1, count, 4] send slot i to slot perm(i)."""
    rec = np.zeros((n, count, 4), np.int64)
    rows = np.zeros((n - 1, count, 4), np.int32)
    pts = rng.integers(200, 3000, (count, 2))
    rec[0, :, :2] = pts
    for f in range(1, n):
        perm = rng.permutation(count)
        nxt = np.stack([pts[:, 0] + 3 - pts[:, 1] // 64, pts[:, 1] + 2 + pts[:, 0] // 64], 1)
        wrong = rng.random(count) < 0.3
        nxt[wrong] = rng.integers(0, 3400, (int(wrong.sum()), 2))
        nxt = np.clip(nxt, 0, 65535)   # every slot stays a correspondence
        rec[f, perm, :2] = nxt
        rows[f - 1, :, 0], rows[f - 1, :, 3] = perm, 15
        pts = rec[f, :, :2].copy()
    return rec, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--box", default="unnamed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion.jsonl"))
    args = ap.parse_args()
    n = args.frames
    pairs = capi.consecutive_pairs(n)
    rng = np.random.default_rng(31)
    with capi.Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.set_option("profile_stage_mask", 1 << 30)   # the parts behind the polygons go by bit 30
        cases = []
        for count, hyp in CASES:
            rec, rows = batch(rng, n, count)
            desc = rng.integers(0, 1 << 63, (n, count, 4), dtype=np.int64).astype(np.uint64)
            v = dict(count=count, hyp=hyp, ms={m: {p: [] for p in capi.MOTION_PARTS} for m in range(3)}, match=[])
            for name, a in (("d_rec", rec), ("d_rows", rows), ("d_desc", desc), ("d_cnt", np.full(n, count, np.int32))):
                v[name] = ctx.malloc(a.nbytes)
                ctx.h2d(v[name], a)
            v["d_motion"], v["d_in"] = ctx.malloc(8 * 16 * len(pairs)), ctx.malloc(4 * count * len(pairs))
            v["d_m"], v["d_pc"] = ctx.malloc(16 * count * len(pairs)), ctx.malloc(4 * len(pairs))
            cases.append(v)

        def call(v, model):
            ctx.profile_reset()
            ctx.dev_estimate_motion(v["d_rec"], v["d_cnt"], n, v["count"], v["d_rec"], v["d_cnt"], n, v["count"], pairs,
                                    v["d_rows"], v["d_motion"], v["d_in"], model, 32, v["hyp"], 1)
            return [ctx.motion_profile_get(p)[0] for p in range(len(capi.MOTION_PARTS))]

        def match(v):
            ctx.profile_reset()
            ctx.dev_match_descriptors(v["d_desc"], v["d_cnt"], n, v["count"], v["d_desc"], v["d_cnt"], n, v["count"], pairs,
                                      v["d_m"], v["d_pc"], 64, 205, capi.MATCH_CROSS_CHECK)
            return ctx.descriptors_profile_get(capi.DESC_PARTS.index("match"))[0]

        for v in cases:   # warm-up, and what the batch gives
            v["inliers"] = {}
            for model in range(3):
                call(v, model)
                out = np.empty((len(pairs), 16), np.int64)
                ctx.d2h(out, v["d_motion"])
                v["inliers"][model] = float(out[:, 2].mean())
                assert (out[:, 1] == v["count"]).all() and (out[:, 0] & 1).all()
            match(v)
        for rnd in range(args.rounds):
            print(f"round {rnd + 1} of {args.rounds}", flush=True)
            for v in cases:
                for _ in range(3):
                    for model in range(3):
                        for name, ms in zip(capi.MOTION_PARTS, call(v, model)):
                            v["ms"][model][name].append(ms)
                    v["match"].append(match(v))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        stat = lambda x: dict(median=statistics.median(x), min=min(x), max=max(x))
        with open(args.out, "a") as f:
            for v in cases:
                tests = len(pairs) * v["count"] * v["hyp"]
                for model in range(3):
                    score = statistics.median(v["ms"][model]["score"])
                    line = dict(box=args.box, frames=n, pairs=len(pairs), correspondences=v["count"], hypotheses=v["hyp"],
                                model=model, thr_q4=32, mean_inliers=v["inliers"][model], calls=len(v["match"]),
                                ms={k: stat(x) for k, x in v["ms"][model].items()}, residual_tests=tests,
                                residual_tests_per_s=tests / (score * 1e-3) if score > 0 else 0.0,
                                matcher_match_ms=stat(v["match"]),
                                times="HIP events around each part's launches; no counters")
                    f.write(json.dumps(line) + "\n")
                    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
