#!/usr/bin/env python3
"""Colour input on 128 x 3840x2160, device resident: what the fused Gaussian (BGR rows converted as they are loaded)
costs against the gray pipeline and against two-pass (standalone conversion, then the gray pipeline).

  (a) dev_canny on the gray plane
  (b) dev_canny_color BGR, fuse_gray = 1 (fused where the window allows: sigma 1.0 = window 7 is fused, sigma 1.4 =
      window 11 is not, see DESIGN.md "Colour input")
  (c) dev_canny_color BGR, fuse_gray = 0 (two-pass)

(a)(b)(c) are interleaved, ROUNDS rounds of STEPS calls each, wall time per call with the stream drained before and
after.  Then the per-stage events (GAUSSIAN, TO_GRAY) of (b) and (c), and host -> host canny_batch_color_bits against
canny_batch_bits with pinned input.  The kernel times are set per process (README), so run this in several processes:
    python tools/probe_colour_input.py [out.json]   (one JSON object; appended as a line to out.json if given)"""
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from canny_edge_amd import capi  # noqa: E402
from canny_edge_amd.synth import synth_frame  # noqa: E402

N, H, W = 128, 2160, 3840
ROUNDS, STEPS = 5, 5
N_H2H = 32
px = N * H * W

ctx = capi.Context(0)
base = [np.stack([synth_frame(H, W, 3 * s + k) for k in range(3)], axis=-1) for s in range(4)]  # B, G, R planes
bgr = np.stack([base[i % 4] for i in range(N)])
gray = np.stack([ctx.to_gray(b) for b in base])
gray = np.stack([gray[i % 4] for i in range(N)])
d_bgr, d_gray, d_out = ctx.malloc(bgr.nbytes), ctx.malloc(gray.nbytes), ctx.malloc(px * 2)
ctx.h2d(d_bgr, bgr)
ctx.h2d(d_gray, gray)


def run(kind, sigma):
    if kind == "a":
        ctx.dev_canny(d_gray, sigma, 50, 150, H, W, N, d_out)
    else:
        ctx.set_option("fuse_gray", 1 if kind == "b" else 0)
        ctx.dev_canny_color(d_bgr, capi.LAYOUT_BGR8, sigma, 50, 150, H, W, N, d_out)


def timed(kind, sigma):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        run(kind, sigma)
    ctx.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


result = {"frames": N, "height": H, "width": W, "rounds": ROUNDS, "steps": STEPS}
for sigma in (1.0, 1.4):
    for k in "abc":
        run(k, sigma)  # warm-up (workspaces, code objects)
    rounds = []
    for _ in range(ROUNDS):
        r = {k: round(timed(k, sigma), 4) for k in "abc"}
        ctx.set_option("fuse_gray", 1)
        run("b", sigma)
        r["fused"] = ctx.get_option("last_canny_fused_gray")
        rounds.append(r)
    stages = {}
    for k in "bc":
        ctx.synchronize()
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(STEPS):
            run(k, sigma)
        ctx.synchronize()
        stages[k] = {name: round(ctx.profile_get(s)[0] / STEPS, 4)
                     for s, name in ((capi.STAGE_GAUSSIAN, "gaussian"), (capi.STAGE_TO_GRAY, "to_gray"),
                                     (capi.STAGE_SOBEL_NMS, "sobel_nms"))}
        ctx.profile_enable(False)
    ctx.set_option("fuse_gray", 1)
    result[f"sigma_{sigma}"] = {"rounds_ms": rounds, "b_beats_c_every_round": all(r["b"] < r["c"] for r in rounds),
                                "stage_ms": stages}

# host -> host, pinned input, bit maps out
h_bgr = ctx.pinned_array((N_H2H, H, W, 3), np.uint8)
h_bgr[...] = bgr[:N_H2H]
h_gray = ctx.pinned_array((N_H2H, H, W), np.uint8)
h_gray[...] = gray[:N_H2H]
h2h = {}
for name, fn in (("gray_bits", lambda: ctx.canny_batch(h_gray, 1.4, 50, 150, bits=True)),
                 ("bgr_bits", lambda: ctx.canny_batch_color(h_bgr, 1.4, 50, 150, "bgr", fmt="bits"))):
    fn()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    h2h[name] = {"ms": round(best * 1e3, 3), "gpix_per_s": round(N_H2H * H * W / best / 1e9, 2)}
result["host_to_host_pinned_32x4k"] = h2h
line = json.dumps(result)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "a") as f:
        f.write(line + "\n")
