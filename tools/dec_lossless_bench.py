#!/usr/bin/env python3
"""What a lossless (VP8L) file costs in the device decode, and against the route
a user had before it: a batch of 1080p lossless files through
decode_webp_batch_device(lossless=True) into CHW u8 and f16 tensors, and in the
same run the full host decode of the same files on the same host threads (the
decode_frame path, zwebp.dbg_vp8l_decode from a thread pool of
zwebp.host_threads() workers), one upload of the ARGB words, and a torch
permute and cast to the same tensor.

The files: the product's own lossless encodes (WebPEncoder, default params) of
8 of the bench's synthetic frames, and libwebp's lossless encodes (PIL) of the
same frames where PIL is installed, each cycled to `frames` files.  Every leg
is warmed once, then the legs run alternately `--reps` times; one JSON line
with decodes/s per leg (all repeats, median, min, max) and, for the device
legs, zwebp.decode_lossless_times of the last repeat (host entropy decode wall
ms, transform kernels ms, store kernel ms, summed over the chunks).

    python tools/dec_lossless_bench.py [frames=256] [--reps 5] [--out FILE]
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

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

F, w, h = a.frames, 1920, 1080
ctx = zwebp.Context(0)
L = zwebp.load_library()
NT = zwebp.host_threads()
imgs = [np.ascontiguousarray(synth_rgba(w, h, 0x5EED0000 + i)[..., :3]) for i in range(8)]


def cycle(files):
    return [files[i % len(files)] for i in range(F)]


enc = zwebp.WebPEncoder(ctx=ctx)  # default params: lossless
sources = {"own": [bytes(enc.encode(img, w, h, zwebp.ColorType.Rgb8)) for img in imgs]}
res = {"workload": f"{F} lossless files {w}x{h} (8 distinct images), {a.reps} alternating repeats",
       "host_threads": NT, "files": {}, "legs": {}}
try:
    from PIL import Image
    lib = []
    for img in imgs:
        b = io.BytesIO()
        Image.fromarray(img).save(b, "WEBP", lossless=True, quality=75, method=4)
        lib.append(b.getvalue())
    sources["libwebp"] = lib
except ImportError:
    res["libwebp"] = "PIL not installed: leg skipped"

outs = {"u8": torch.empty((F, 3, h, w), dtype=torch.uint8, device=dev),
        "f16": torch.empty((F, 3, h, w), dtype=torch.float16, device=dev)}
scale, bias = [1.0 / 255.0] * 4, [0.0] * 4
argb = np.empty((F, h, w), np.uint32)  # the host route's decoded frames


def host_route(payloads, dt):
    """decode_frame on every file over the host threads, one upload, permute and cast on the device."""
    def one(i):
        p = payloads[i]
        ww, hh = ctypes.c_uint32(), ctypes.c_uint32()
        rc = L.zw_dbg_vp8l_decode(p, len(p), argb[i].ctypes.data, ctypes.byref(ww), ctypes.byref(hh))
        assert rc == 0 and (ww.value, hh.value) == (w, h)
    with ThreadPoolExecutor(NT) as pool:
        list(pool.map(one, range(F)))
    t = torch.from_numpy(argb).to(dev)                       # words 0xAARRGGBB: bytes B, G, R, A
    rgb = t.view(torch.uint8).view(F, h, w, 4)[..., [2, 1, 0]].permute(0, 3, 1, 2)
    if dt == "u8":
        outs[dt].copy_(rgb)
    else:
        outs[dt].copy_(rgb.to(torch.float32) * (1.0 / 255.0))
    torch.cuda.synchronize(dev)


legs = []
for sname, files in sources.items():
    infos = [zwebp.webp_parse(f, lossless=True) for f in files]
    tf = [[[t, b] for t, b, _ in zwebp.dbg_vp8l_read_coded(f[i["vp8_offset"]:i["vp8_offset"] + i["vp8_len"]])[3]]
          for f, i in zip(files, infos)]
    res["files"][sname] = {"mean_bytes": round(sum(len(f) for f in files) / len(files)), "transforms": tf[0]}
    fl = cycle(files)
    pl = cycle([f[i["vp8_offset"]:i["vp8_offset"] + i["vp8_len"]] for f, i in zip(files, infos)])
    for dt, t in outs.items():
        kw = {} if dt == "u8" else {"scale": scale, "bias": bias}
        legs.append((f"{sname}_device_chw_{dt}", True,
                     lambda fl=fl, t=t, kw=kw: zwebp.decode_webp_batch_device(fl, t, lossless=True, ctx=ctx, **kw)))
        legs.append((f"{sname}_host_route_chw_{dt}", False, lambda pl=pl, dt=dt: host_route(pl, dt)))

# the two routes give the same tensor
checks = {}
for name, is_dev, fn in legs:
    fn()
    dt = name.rsplit("_", 1)[1]
    checks[name] = outs[dt][: min(F, 8)].clone()
for sname in sources:
    for dt in outs:
        res["legs"].setdefault(f"{sname}_device_chw_{dt}", {})["equals_host_route"] = bool(
            torch.equal(checks[f"{sname}_device_chw_{dt}"], checks[f"{sname}_host_route_chw_{dt}"]))
del checks

rates = {n: [] for n, _, _ in legs}
extra = {}
for _ in range(a.reps):
    for name, is_dev, fn in legs:
        t0 = time.perf_counter()
        fn()
        rates[name].append(F / (time.perf_counter() - t0))
        if is_dev:
            ms = zwebp.decode_lossless_times(ctx=ctx)
            extra[name] = {"lossless_times_ms": {"host_entropy": round(ms[0], 1), "transform_kernels": round(ms[1], 3),
                                                 "store_kernel": round(ms[2], 3)}}
for name, _, _ in legs:
    r = rates[name]
    res["legs"].setdefault(name, {}).update({"decodes_per_s": [round(x, 1) for x in r],
                                             "median": round(statistics.median(r), 1), "min": round(min(r), 1),
                                             "max": round(max(r), 1), **extra.get(name, {})})

line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
