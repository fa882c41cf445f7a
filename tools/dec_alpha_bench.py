#!/usr/bin/env python3
"""What alpha costs in the device decode: a batch of 1080p lossy files with an
ALPH chunk through decode_webp_batch_device(alpha=True) (CHW, u8 and f16)
against the same files' VP8 payloads through decode_batch_device(channels=4) in
the same run.

The files: the product's own RGBA encodes (encode_webp_batch) of 8 synthetic
images with a soft alpha, and libwebp's encodes (PIL, alpha_quality=100) of the
same images, each cycled to `frames` files.  Every leg is warmed once, then the
legs run alternately `--reps` times; one JSON line with decodes/s per leg (all
repeats, median, min, max), zwebp.decode_alpha_times (host ALPH wall ms, filter
kernels ms, store kernel ms) and the host parse ms of each alpha leg's last
repeat.  Then, per filter, a batch of files whose ALPH chunks are raw data with
that filter (built here with the forward filter): the filter kernels' device
time from HIP events around their launches (decode_alpha_times()[1]), median of
`--reps` runs.  A kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/dec_alpha_bench.py 64 --reps 1 --only-filters) names the same launches.

    python tools/dec_alpha_bench.py [frames=256] [--reps 5] [--out FILE] [--only-filters]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # torch's HIP runtime first, then the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-webp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--only-filters", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp  # noqa: E402
from zwebp.synth import synth_rgba  # noqa: E402
import alpha_ref as R  # noqa: E402

F, w, h = a.frames, 1920, 1080
ctx = zwebp.Context(0)
yy, xx = np.mgrid[0:h, 0:w]
imgs = []
for i in range(8):
    img = synth_rgba(w, h, 0x5EED0000 + i).copy()
    soft = np.clip(255 - np.hypot(xx - w * (0.3 + 0.05 * i), yy - h * 0.5) * (0.2 + 0.02 * i), 0, 255)
    img[..., 3] = soft.astype(np.uint8)
    imgs.append(img)


def cycle(files):
    return [files[i % len(files)] for i in range(F)]


def payloads(files):
    out = []
    for f in files:
        info = zwebp.webp_parse(f, alpha=True)
        out.append(f[info["vp8_offset"]:info["vp8_offset"] + info["vp8_len"]])
    return out


res = {"workload": f"{F} files {w}x{h} Q75 with alpha (8 distinct images), {a.reps} alternating repeats",
       "host_threads": zwebp.host_threads(), "legs": {}, "filters": {}}
outs = {"u8": torch.empty((F, 4, h, w), dtype=torch.uint8, device=dev),
        "f16": torch.empty((F, 4, h, w), dtype=torch.float16, device=dev)}
scale, bias = [1.0 / 255.0] * 4, [0.0] * 4

if not a.only_filters:
    own = [bytes(b) for b in zwebp.encode_webp_batch(imgs, w, h, zwebp.ColorType.Rgba8, 75, 4, ctx=ctx)]
    sources = {"own": own}
    try:
        from PIL import Image
        lib = []
        for img in imgs:
            b = io.BytesIO()
            Image.fromarray(img).save(b, "WEBP", quality=75, alpha_quality=100, method=4)
            lib.append(b.getvalue())
        sources["libwebp"] = lib
    except ImportError:
        res["libwebp"] = "PIL not installed: leg skipped"
    res["alph"] = {}
    legs = []
    for sname, files in sources.items():
        al = [zwebp.webp_parse(f, alpha=True) for f in files]
        res["alph"][sname] = {"header_bytes": sorted({f[i["alph_offset"]] for f, i in zip(files, al)}),
                              "mean_alph_bytes": round(sum(i["alph_len"] for i in al) / len(al)),
                              "mean_vp8_bytes": round(sum(i["vp8_len"] for i in al) / len(al))}
        fl, vp = cycle(files), cycle(payloads(files))
        for dt, t in outs.items():
            kw = {} if dt == "u8" else {"scale": scale, "bias": bias}
            legs.append((f"{sname}_alpha_chw_{dt}", True,
                         lambda fl=fl, t=t, kw=kw: zwebp.decode_webp_batch_device(fl, t, alpha=True, ctx=ctx, **kw)))
            legs.append((f"{sname}_opaque_chw_{dt}", False,
                         lambda vp=vp, t=t, kw=kw: zwebp.decode_batch_device(vp, t, ctx=ctx, **kw)))
    for _, _, fn in legs:
        fn()
    rates = {n: [] for n, _, _ in legs}
    extra = {}
    for _ in range(a.reps):
        for name, is_alpha, fn in legs:
            t0 = time.perf_counter()
            fn()
            rates[name].append(F / (time.perf_counter() - t0))
            extra[name] = {"host_parse_ms": round(zwebp.decode_stage_times(ctx=ctx)[0], 1)}
            if is_alpha:
                ms = zwebp.decode_alpha_times(ctx=ctx)
                extra[name]["alpha_times_ms"] = {"host_alph": round(ms[0], 1), "filter_kernels": round(ms[1], 3),
                                                 "store_kernel": round(ms[2], 3)}
    for name, _, _ in legs:
        r = rates[name]
        res["legs"][name] = {"decodes_per_s": [round(x, 1) for x in r], "median": round(statistics.median(r), 1),
                             "min": round(min(r), 1), "max": round(max(r), 1), **extra[name]}
    for sname in sources:
        for dt in outs:
            al, op = res["legs"][f"{sname}_alpha_chw_{dt}"]["median"], res["legs"][f"{sname}_opaque_chw_{dt}"]["median"]
            res["legs"][f"{sname}_alpha_chw_{dt}"]["ms_per_batch_over_opaque"] = round(F / al * 1e3 - F / op * 1e3, 1)

# ---- the filter kernels, each on a batch whose frames all use that filter ----
own_vp8 = zwebp.encode_batch(imgs, w, h, zwebp.ColorType.Rgba8, 75, 4, ctx=ctx)
for filt, fname in ((1, "horizontal"), (2, "vertical"), (3, "gradient")):
    files = cycle([R.webp_with_alph(bytes(v), R.raw_alph(img[..., 3], filt), w, h) for v, img in zip(own_vp8, imgs)])
    t = outs["u8"]
    zwebp.decode_webp_batch_device(files, t, alpha=True, ctx=ctx)
    ms = []
    for _ in range(a.reps):
        zwebp.decode_webp_batch_device(files, t, alpha=True, ctx=ctx)
        ms.append(zwebp.decode_alpha_times(ctx=ctx))
    check = t[0, 3].cpu().numpy()
    res["filters"][fname] = {"filter_kernels_ms_per_batch": round(statistics.median(m[1] for m in ms), 3),
                             "store_kernel_ms_per_batch": round(statistics.median(m[2] for m in ms), 3),
                             "alpha_equals_input": bool(np.array_equal(check, imgs[0][..., 3]))}

line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
