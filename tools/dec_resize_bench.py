#!/usr/bin/env python3
"""Decode a batch of 1080p Q75 frames to 224x224 CHW f16 (ImageNet scale and bias) two ways
in one run:

  fused         decode_batch_device_resized: k_yuv2rgb_resize writes the 224x224 batch
                tensor from the decoded planes;
  full_interp   what the library offered before: decode_batch_device at full size into a
                [N, 3, 1080, 1920] f16 tensor, then torch.nn.functional.interpolate
                (bilinear, antialias=False) into the batch tensor (in slices of 128 frames);
  fused_mixed   the fused entry over the same number of frames in 4 sizes, interleaved:
                one decode pass per size.

Every leg is warmed once, then the legs run alternately `--reps` times each; one JSON line
with wall ms and decodes/s per leg (all repeats, median, min, max) and the conversion
kernels' device time (decode_rgb_kernel_ms: k_yuv2rgb_resize for the fused legs,
k_yuv2rgb_dev for full_interp, beside torch's device time for the interpolate slices).
The two routes resample by different rules (the fused one in integers, torch in floats),
so the tool reports their largest difference, not equality.

--antialias runs the same three legs with antialiasing on both routes: the fused legs
through antialias=True (k_resize_aa_weights + k_yuv2rgb_resize_aa, the triangle rule),
full_interp through interpolate(antialias=True); the result then also carries the fused
kernels' device time over k_yuv2rgb_dev's on the same frames.

    python tools/dec_resize_bench.py [frames=1024] [--reps 5] [--antialias] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # torch's HIP runtime first, then the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-webp_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--antialias", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp  # noqa: E402
from zwebp.synth import synth_rgba  # noqa: E402

F, w, h, OW, OH = a.frames, 1920, 1080, 224, 224
SIZES = ((1920, 1080), (1600, 900), (1280, 720), (1024, 768))
ctx = zwebp.Context(0)


def streams_of(sw, sh):
    imgs = [synth_rgba(sw, sh, 0x5EED0000 + i) for i in range(8)]
    return zwebp.encode_batch(imgs, sw, sh, zwebp.ColorType.Rgba8, 75, 4, ctx=ctx)


by_size = [streams_of(sw, sh) for (sw, sh) in SIZES]
vp8 = [by_size[0][i % 8] for i in range(F)]
mixed = [by_size[i % 4][(i // 4) % 8] for i in range(F)]

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
scale = [1.0 / (255.0 * s) for s in STD]
bias = [-m / s for m, s in zip(MEAN, STD)]
full = torch.empty((F, 3, h, w), dtype=torch.float16, device=dev)
out_fused = torch.empty((F, 3, OH, OW), dtype=torch.float16, device=dev)
out_interp = torch.empty((F, 3, OH, OW), dtype=torch.float16, device=dev)
out_mixed = torch.empty((F, 3, OH, OW), dtype=torch.float16, device=dev)


def fused():
    zwebp.decode_batch_device_resized(vp8, None, out_fused, scale=scale, bias=bias, ctx=ctx, antialias=a.antialias)


interp_ms = []  # device time of the interpolate and copy slices (torch events)


def full_interp():
    zwebp.decode_batch_device(vp8, full, scale=scale, bias=bias, ctx=ctx)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(0, F, 128):
        out_interp[i:i + 128] = torch.nn.functional.interpolate(full[i:i + 128], size=(OH, OW), mode="bilinear",
                                                                antialias=a.antialias, align_corners=False)
    e1.record()
    torch.cuda.synchronize()
    interp_ms.append(e0.elapsed_time(e1))


def fused_mixed():
    zwebp.decode_batch_device_resized(mixed, None, out_mixed, scale=scale, bias=bias, ctx=ctx, antialias=a.antialias)


legs = [("fused", fused), ("full_interp", full_interp), ("fused_mixed", fused_mixed)]
for _, fn in legs:  # warm-up: staging, pool, scratch, torch's kernels
    fn()
interp_ms.clear()
ms = {name: [] for name, _ in legs}
kernel_ms = {name: [] for name, _ in legs}
for _ in range(a.reps):
    for name, fn in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t0) * 1e3)
        kernel_ms[name].append(zwebp.decode_rgb_kernel_ms(ctx=ctx))

diff = (out_fused.float() - out_interp.float()).abs()
FUSED_KERNEL = "k_resize_aa_weights + k_yuv2rgb_resize_aa" if a.antialias else "k_yuv2rgb_resize"
res = {"antialias": bool(a.antialias),
       "workload": f"{F} frames {w}x{h} Q75 m4 (8 distinct synth_rgba images) -> {OW}x{OH} CHW f16, "
                   f"{a.reps} alternating repeats; fused_mixed: {F} frames of "
                   + ", ".join(f"{sw}x{sh}" for sw, sh in SIZES) + " interleaved",
       "legs": {}}
for name, _ in legs:
    m, k = ms[name], kernel_ms[name]
    res["legs"][name] = {"wall_ms": [round(x, 1) for x in m], "median_ms": round(statistics.median(m), 1),
                         "min_ms": round(min(m), 1), "max_ms": round(max(m), 1),
                         "decodes_per_s_median": round(F / statistics.median(m) * 1e3, 1),
                         "rgb_kernel": "k_yuv2rgb_dev" if name == "full_interp" else FUSED_KERNEL,
                         "rgb_kernel_ms": [round(x, 3) for x in k],
                         "rgb_kernel_ms_median": round(statistics.median(k), 3)}
res["legs"]["full_interp"]["interpolate_device_ms"] = [round(x, 3) for x in interp_ms]
res["legs"]["full_interp"]["interpolate_device_ms_median"] = round(statistics.median(interp_ms), 3)
res["fused_over_full_interp"] = round(statistics.median(ms["full_interp"]) / statistics.median(ms["fused"]), 3)
res["fused_kernel_ms_over_yuv2rgb_dev_ms"] = round(statistics.median(kernel_ms["fused"])
                                                   / statistics.median(kernel_ms["full_interp"]), 3)
res["fused_vs_interp_max_abs_diff"] = round(float(diff.max()), 4)
res["fused_vs_interp_mean_abs_diff"] = round(float(diff.mean()), 6)
res["full_size_tensor_bytes"] = full.numel() * full.element_size()
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
