#!/usr/bin/env python3
"""Encode a batch of 1080p frames that already sit in HBM as a torch tensor, by two
routes, and time the ingest kernel.

Route comparison (wall time, all repeats, median, min, max), per source tensor
(CHW f16 holding v / 255, CHW f32 holding (v / 255 - mean) / std, HWC u8 x 4):
  device      zwebp.encode_batch_device(tensor): one call, its pipeline created inside;
  set_input   a Pipeline made once, set_input(tensor) + encode() per repeat;
  torch_copy  today's route: torch ops to a packed u8 HWC image (permute, scale, bias,
              round, clamp, cast), a device copy into Pipeline.input_ptr, encode(), on
              a Pipeline made once.
The routes' bitstreams are compared equal outside the timed region.

Ingest kernel: Pipeline.kernel_times()[0] (the mean device time of one rgb2yuv launch,
launch_frames frames) over run_device() repeats for every layout x dtype, next to the
fraction of 8 TB/s its traffic makes (tensor bytes read + 1.5 B/pixel written), and
k_rgb2yuv_rows<3> / <4> from the packed buffer in the same run.  The HWC u8 x 4 tensor
path issues the loads of k_rgb2yuv_rows<4>: it holds when its median is not above that
kernel's by more than that kernel's own spread (max - min).

    python tools/enc_device_bench.py [frames=256] [--reps 5] [--out FILE]
"""
import argparse
import ctypes
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
ap.add_argument("frames", nargs="?", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp  # noqa: E402
from zwebp.synth import synth_rgba  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch has loaded)
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipMemcpy.restype = ctypes.c_int

F, w, h = a.frames, 1920, 1080
Q, M = 75, 4
ctx = zwebp.Context(0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [255.0 * s for s in STD]
BIAS = [255.0 * m for m in MEAN]

distinct = torch.from_numpy(np.stack([synth_rgba(w, h, 0x5EED0000 + i) for i in range(8)])).to(dev)
u8 = distinct[torch.arange(F, device=dev) % 8].contiguous()  # [F, h, w, 4]
mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
scale_t = torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)
bias_t = torch.tensor(BIAS, device=dev).view(1, 3, 1, 1)
chw = u8[..., :3].permute(0, 3, 1, 2).contiguous()
src = {
    "chw_f16": ((chw.float() / 255.0).half(), 255.0, None),
    "chw_f32": (((chw.float() / 255.0) - mean_t) / std_t, SCALE, BIAS),
    "hwc_u8_c4": (u8, None, None),
}
del chw
torch.cuda.synchronize()

pipe3 = zwebp.Pipeline(F, w, h, zwebp.ColorType.Rgb8, Q, M, ctx=ctx)
pipe4 = zwebp.Pipeline(F, w, h, zwebp.ColorType.Rgba8, Q, M, ctx=ctx)


def to_packed(name):
    # today's caller-side chain: the packed u8 HWC image of the source
    t = src[name][0]
    if name == "chw_f16":
        return (t.float() * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    if name == "chw_f32":
        return (t * scale_t + bias_t).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return t


def pipe_of(name):
    return pipe4 if name == "hwc_u8_c4" else pipe3


def copy_in(p, packed):
    torch.cuda.synchronize()
    rc = hip.hipMemcpy(p.input_ptr, packed.data_ptr(), packed.numel(), 3)  # device to device
    assert rc == 0, rc
    torch.cuda.synchronize()


def route_device(name):
    t, s, b = src[name]
    return zwebp.encode_batch_device(t, Q, M, "hwc" if name.startswith("hwc") else "chw", s, b, ctx=ctx)


def route_set_input(name):
    t, s, b = src[name]
    p = pipe_of(name)
    p.set_input(t, "hwc" if name.startswith("hwc") else "chw", s, b)
    p.encode()
    p.set_input(None)
    return p


def route_torch_copy(name):
    p = pipe_of(name)
    copy_in(p, to_packed(name))
    p.encode()
    return p


legs = []
for name in src:
    legs.append((name + ".device", lambda name=name: route_device(name)))
    legs.append((name + ".set_input", lambda name=name: route_set_input(name)))
    legs.append((name + ".torch_copy", lambda name=name: route_torch_copy(name)))

# warm-up, and the routes' outputs compared (outside the timed region)
equal = {}
for name in src:
    d = route_device(name)
    s = [route_set_input(name).output(i) for i in range(F)]
    t = [route_torch_copy(name).output(i) for i in range(F)]
    equal[name] = d == s == t
    assert equal[name], name + ": the routes' bitstreams differ"

ms = {n: [] for n, _ in legs}
for _ in range(a.reps):
    for n, fn in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms[n].append(1e3 * (time.perf_counter() - t0))


def stats(v, nd=3):
    return {"all": [round(x, nd) for x in v], "median": round(statistics.median(v), nd), "min": round(min(v), nd),
            "max": round(max(v), nd), "spread": round(max(v) - min(v), nd)}


res = {"workload": f"{F} frames {w}x{h} Q{Q} m{M} (8 distinct synth_rgba images), {a.reps} alternating repeats",
       "routes_wall_ms": {n: stats(v, 2) for n, v in ms.items()}, "routes_equal": equal}
for name in src:
    d, t = statistics.median(ms[name + ".set_input"]), statistics.median(ms[name + ".torch_copy"])
    res["routes_wall_ms"][name + ".set_input_over_torch_copy"] = round(d / t, 4)

# ---- the ingest kernel alone ----
ES = {"u8": 1, "f16": 2, "f32": 4}
kern = {}


def kernel_leg(p, reps):
    v = []
    for _ in range(reps + 1):  # (the first run warms)
        p.run_device()
        v.append(p.kernel_times()[0])
    return v[1:]


def traffic(v, read_bytes, lf):
    st = stats(v, 4)
    tot = lf * (read_bytes + 1.5 * w * h)
    st["launch_frames"] = lf
    st["bytes_per_launch"] = int(tot)
    st["tb_per_s"] = round(tot / (st["median"] * 1e-3) / 1e12, 3)
    st["fraction_of_8_tb_s"] = round(st["tb_per_s"] / 8.0, 3)
    return st


for layout in ("hwc", "chw"):
    for dt, tdt in (("u8", torch.uint8), ("f16", torch.float16), ("f32", torch.float32)):
        for ch in (3, 4):
            shape = (F, h, w, ch) if layout == "hwc" else (F, ch, h, w)
            if dt == "u8":
                t = (u8[..., :ch] if layout == "hwc" else u8[..., :ch].permute(0, 3, 1, 2)).contiguous()
            else:
                t = torch.empty(shape, dtype=tdt, device=dev)
                t.copy_(u8[..., :ch] if layout == "hwc" else u8[..., :ch].permute(0, 3, 1, 2))
            p = pipe3 if ch == 3 else pipe4
            p.set_input(t, layout, 1.0, 0.0)
            read = w * h * ES[dt] * (ch if layout == "hwc" else 3)  # (plane 3 of a CHW tensor is never read)
            kern[f"k_rgb2yuv_dev {layout} {dt} c{ch}"] = traffic(kernel_leg(p, a.reps), read, p.launch_frames)
            p.set_input(None)
            del t
for p, bpp in ((pipe3, 3), (pipe4, 4)):
    copy_in(p, u8[..., :bpp].contiguous())
    kern[f"k_rgb2yuv_rows<{bpp}> packed buffer"] = traffic(kernel_leg(p, a.reps), w * h * bpp, p.launch_frames)
res["ingest_kernel_ms"] = kern
rows4, dev4 = kern["k_rgb2yuv_rows<4> packed buffer"], kern["k_rgb2yuv_dev hwc u8 c4"]
res["hwc_u8_c4_vs_rows4"] = {"dev_median_ms": dev4["median"], "rows4_median_ms": rows4["median"],
                             "rows4_spread_ms": rows4["spread"],
                             "not_slower": dev4["median"] <= rows4["median"] + rows4["spread"]}
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
