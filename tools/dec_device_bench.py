#!/usr/bin/env python3
"""Decode a batch of 1080p Q75 frames into host RGBA buffers (decode_rgb_batch_into,
reused buffers: the baseline) and straight into device tensors
(decode_batch_device): u8 HWC 4 channels, u8 / f16 / f32 CHW 3 channels.

Every leg is warmed once, then the legs run alternately `--reps` times each; one
JSON line with decodes/s per leg (all repeats, median, min, max).  A device leg
holds when its median is not below the baseline's median by more than the
baseline's own spread (max - min) across its repeats.

    python tools/dec_device_bench.py [frames=1024] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # torch's HIP runtime first, then the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-webp_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp  # noqa: E402
from zwebp.synth import synth_rgba  # noqa: E402

F, w, h = a.frames, 1920, 1080
ctx = zwebp.Context(0)
imgs = [synth_rgba(w, h, 0x5EED0000 + i) for i in range(8)]
streams = zwebp.encode_batch(imgs, w, h, zwebp.ColorType.Rgba8, 75, 4, ctx=ctx)
vp8 = [streams[i % len(streams)] for i in range(F)]

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
scale = [1.0 / (255.0 * s) for s in STD]
bias = [-m / s for m, s in zip(MEAN, STD)]
bufs = [np.empty(w * h * 4, np.uint8) for _ in range(F)]
outs = {
    "device_u8_hwc_c4": torch.empty((F, h, w, 4), dtype=torch.uint8, device=dev),
    "device_u8_chw_c3": torch.empty((F, 3, h, w), dtype=torch.uint8, device=dev),
    "device_f16_chw_c3": torch.empty((F, 3, h, w), dtype=torch.float16, device=dev),
    "device_f32_chw_c3": torch.empty((F, 3, h, w), dtype=torch.float32, device=dev),
}
legs = [("decode_rgb_batch_into_rgba", lambda: zwebp.decode_rgb_batch_into(vp8, bufs, 4, ctx=ctx))]
for name, t in outs.items():
    fl = "u8" not in name
    legs.append((name, lambda t=t, fl=fl: zwebp.decode_batch_device(vp8, t, scale=scale if fl else None,
                                                                    bias=bias if fl else None, ctx=ctx)))
kernel_ms = {}
for name, fn in legs:  # warm-up: staging, pool, scratch
    fn()
rates = {name: [] for name, _ in legs}
parse_ms = {name: [] for name, _ in legs}  # host parse, wall ms summed over chunks
token_ms = {name: [] for name, _ in legs}  # device token parse
for _ in range(a.reps):
    for name, fn in legs:
        t0 = time.perf_counter()
        fn()
        rates[name].append(F / (time.perf_counter() - t0))
        kernel_ms[name] = zwebp.decode_rgb_kernel_ms(ctx=ctx)
        parse_ms[name].append(round(zwebp.decode_stage_times(ctx=ctx)[0], 1))
        token_ms[name].append(round(zwebp.decode_token_ms(ctx=ctx), 1))

res = {"workload": f"{F} frames {w}x{h} Q75 m4 (8 distinct synth_rgba images), {a.reps} alternating repeats",
       "legs": {}}
base = rates[legs[0][0]]
bmed, spread = statistics.median(base), max(base) - min(base)
for name, _ in legs:
    r = rates[name]
    res["legs"][name] = {"decodes_per_s": [round(x, 1) for x in r], "median": round(statistics.median(r), 1),
                         "min": round(min(r), 1), "max": round(max(r), 1),
                         "rgb_kernel_ms_last_batch": round(kernel_ms[name], 3),
                         "host_parse_ms": parse_ms[name], "device_token_ms": token_ms[name]}
    if name != legs[0][0]:
        res["legs"][name]["not_below_baseline"] = statistics.median(r) >= bmed - spread
res["baseline"] = {"leg": legs[0][0], "median": round(bmed, 1), "spread": round(spread, 1)}
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
