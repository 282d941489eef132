#!/usr/bin/env python3
"""Per-frame thresholds on 128 x 3840x2160, device resident: what explicit pairs and the two automatic rules cost against
the fixed-threshold dev_canny.

  fixed     dev_canny(50, 150)
  explicit  dev_canny_thresholds, a different pair per frame
  median    dev_canny_auto("median", 0.67, 1.33)   (+ intensity histogram of the u8 smoothed plane, select)
  quantile  dev_canny_auto("quantile", 0.7, 0.9)   (+ Sobel magnitude histogram of the same plane, select)

on textured synth frames and on constant frames (every lane of a histogram pass hits one bin).  The cases are
interleaved, ROUNDS rounds of STEPS calls each, wall time per call with the stream drained before and after; then the
HYST_CLASSIFY stage events of the automatic cases (the histogram and select passes are timed there).  The kernel times
are set per process (README), so the parent runs the measurement in PROCESSES fresh child processes one after the other
and reports per-case medians over all of them:
    python tools/probe_auto_thresholds.py [out.jsonl] [--processes 3]   (one JSON line; appended to out.jsonl)"""
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 128, 2160, 3840
ROUNDS, STEPS = 5, 5
SIGMA = 1.4
CASES = ("fixed", "explicit", "median", "quantile")


def child():
    from canny_edge_amd import capi
    from canny_edge_amd.synth import synth_batch

    ctx = capi.Context(0)
    px = N * H * W
    d_out, d_thr = ctx.malloc(px * 2), ctx.malloc(N * 8)
    pairs = np.array([(10 + (7 * f) % 60, 100 + (13 * f) % 120) for f in range(N)], np.int32)
    d_pairs = ctx.malloc(pairs.nbytes)
    ctx.h2d(d_pairs, pairs)
    inputs = {"textured": synth_batch(N, H, W, seed=42, distinct=4), "constant": np.full((N, H, W), 128, np.uint8)}
    d_in = ctx.malloc(px)

    def run(kind):
        if kind == "fixed":
            ctx.dev_canny(d_in, SIGMA, 50, 150, H, W, N, d_out)
        elif kind == "explicit":
            ctx.dev_canny_thresholds(d_in, SIGMA, d_pairs, H, W, N, d_out)
        elif kind == "median":
            ctx.dev_canny_auto(d_in, SIGMA, "median", 0.67, 1.33, H, W, N, d_out, d_thr)
        else:
            ctx.dev_canny_auto(d_in, SIGMA, "quantile", 0.7, 0.9, H, W, N, d_out, d_thr)

    def timed(kind):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            run(kind)
        ctx.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    result = {}
    for name, frames in inputs.items():
        ctx.h2d(d_in, frames)
        for k in CASES:
            run(k)  # warm-up (workspaces, code objects)
        rounds = [{k: round(timed(k), 4) for k in CASES} for _ in range(ROUNDS)]
        stage = {}
        for k in ("median", "quantile"):
            ctx.synchronize()
            ctx.profile_reset()
            ctx.set_option("profile_stage_mask", 1 << capi.STAGE_HYST_CLASSIFY)
            ctx.profile_enable(True)
            for _ in range(STEPS):
                run(k)
            ctx.synchronize()
            stage[k] = round(ctx.profile_get(capi.STAGE_HYST_CLASSIFY)[0] / STEPS, 4)
            ctx.profile_enable(False)
            ctx.set_option("profile_stage_mask", 0)
        thr = np.empty((N, 2), np.int32)
        ctx.synchronize()
        ctx.d2h(thr, d_thr)
        result[name] = {"rounds_ms": rounds, "hist_select_ms": stage, "quantile_pair_frame0": thr[0].tolist()}
    print(json.dumps(result))


def main():
    out = None
    procs = 3
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--processes":
            procs = int(args.pop(0))
        else:
            out = a
    runs = []
    for _ in range(procs):  # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child process failed with status {r.returncode}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    result = {"frames": N, "height": H, "width": W, "sigma": SIGMA, "rounds": ROUNDS, "steps": STEPS,
              "processes": procs}
    for name in ("textured", "constant"):
        med = {k: round(statistics.median(rd[k] for run in runs for rd in run[name]["rounds_ms"]), 4) for k in CASES}
        hs = {k: round(statistics.median(run[name]["hist_select_ms"][k] for run in runs), 4)
              for k in ("median", "quantile")}
        result[name] = {"median_ms": med,
                        "over_fixed_ms": {k: round(med[k] - med["fixed"], 4) for k in CASES[1:]},
                        "hist_select_stage_ms": hs,
                        "per_process_ms": [{k: round(statistics.median(rd[k] for rd in run[name]["rounds_ms"]), 4)
                                            for k in CASES} for run in runs]}
    result["constant_over_textured"] = {k: round(result["constant"]["median_ms"][k] /
                                                 result["textured"]["median_ms"][k], 3) for k in CASES}
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main()
