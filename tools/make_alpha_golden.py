#!/usr/bin/env python3
"""Writes the alpha-decode fixtures tests/golden/alpha/ and their manifest
tests/golden/decode_alpha.json.  Run by hand when the fixtures change; the tests
need only its output.

    python tools/make_alpha_golden.py --gallery DIR --gallery-png DIR

Fixtures:
  gallery_N.webp   the reference crate's tests/images/gallery2/N_webp_a.webp
                   (--gallery), lossy with an ALPH chunk; their RGBA digest is
                   taken from the crate's own decode, tests/reference/gallery2/
                   N_webp_a.png (--gallery-png).
  alpha_*.webp     97x61 lossy + alpha encodes made here with PIL / libwebp, one
                   per kind of ALPH chunk found among the candidates (header byte
                   and VP8L transform list): raw data, filters, the colour-indexing
                   transform with 1 / 2 / 4 / 8-bit indices, the predictor
                   transform, no transform, the preprocessing bit.
  ll_*.webp        small lossless files for the headered VP8L hook (noise, natural
                   content, a palette): cross-colour, subtract-green, colour cache.

Manifest, per file: width, height, kind ("alph" | "vp8l"), and for "alph"
  header       the ALPH header byte
  filter       its filtering method
  transforms   the VP8L transform types in bitstream order (tools/vp8l_check.cpp)
  prefilter    SHA-256 of the plane before the filter is undone
  alpha        SHA-256 of the final alpha plane
  rgba         SHA-256 of the RGBA image (gallery: the crate's PNG; else libwebp)
for "vp8l": transforms and argb, SHA-256 of the pixels as little-endian 0xAARRGGBB.

The digests come from libwebp (PIL) and the crate's PNGs, never from the
product: the final alpha is libwebp's, and the pre-filter plane is the forward
filter (tests/alpha_ref.py) of that alpha, which the filter's rule determines
uniquely.  Only the transform list is read with the product's own reader."""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alpha_ref as R  # noqa: E402

W, H = 97, 61


def build_check(tmp):
    exe = os.path.join(tmp, "vp8l_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tools", "vp8l_check.cpp"),
                           os.path.join(ROOT, "image-webp_amd", "csrc", "zw_vp8l_dec.cpp"), "-o", exe])
    return exe


def transforms_of(exe, path):
    out = subprocess.run([exe, "--transforms", path], capture_output=True, text=True, check=True).stdout.split()
    header = int(out[2].split("=")[1])
    tf = out[3].split("=")[1]
    return header, [int(t) for t in tf.split(",")] if tf else []


def rgb_content(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([(xx * 2 + yy) % 256, (yy * 3 + xx // 2) % 256, (xx + yy * 2) % 256], -1).astype(np.int32)
    return np.clip(rgb + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)


def alpha_candidates(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    radial = np.clip(255 - np.hypot(xx - W / 2, yy - H / 2) * 5, 0, 255).astype(np.uint8)
    soft = ((xx * 255) // (W - 1)).astype(np.uint8)
    yield "noise", rng.integers(0, 256, (H, W), dtype=np.uint8)
    yield "radial", radial
    yield "soft", soft
    yield "vsoft", ((yy * 255) // (H - 1)).astype(np.uint8)
    yield "diag", (((xx + yy) * 255) // (W + H - 2)).astype(np.uint8)
    for n in (2, 3, 4, 12, 16, 17, 33, 60, 156):
        levels = np.linspace(0, 255, n).astype(np.uint8)
        yield f"pal{n}", levels[rng.integers(0, n, (H // 4 + 1, W // 4 + 1))].repeat(4, 0).repeat(4, 1)[:H, :W]
        yield f"palnoise{n}", levels[rng.integers(0, n, (H, W))]


def encode(rgb, alpha, **kw):
    b = io.BytesIO()
    Image.fromarray(np.dstack([rgb, alpha])).save(b, "WEBP", quality=75, **kw)
    return b.getvalue()


def alph_entry(exe, path, data, rgba):
    w, h = rgba.shape[1], rgba.shape[0]
    header, tf = transforms_of(exe, path)
    filt = (header >> 2) & 3
    alpha = np.ascontiguousarray(rgba[..., 3])
    return {"kind": "alph", "width": w, "height": h, "header": header, "filter": filt, "transforms": tf,
            "prefilter": R.sha(R.forward_filter(alpha, filt)), "alpha": R.sha(alpha), "rgba": R.sha(rgba)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", required=True, help="the crate's tests/images/gallery2")
    ap.add_argument("--gallery-png", required=True, help="the crate's tests/reference/gallery2")
    args = ap.parse_args()
    out_dir = os.path.join(ROOT, "tests", "golden", "alpha")
    os.makedirs(out_dir, exist_ok=True)
    manifest = {}
    rng = np.random.default_rng(0xA1FA)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_check(tmp)
        for n in range(1, 6):
            data = open(os.path.join(args.gallery, f"{n}_webp_a.webp"), "rb").read()
            name = f"gallery_{n}.webp"
            path = os.path.join(out_dir, name)
            open(path, "wb").write(data)
            rgba = np.array(Image.open(os.path.join(args.gallery_png, f"{n}_webp_a.png")).convert("RGBA"))
            lib = np.array(Image.open(io.BytesIO(data)).convert("RGBA"))
            assert np.array_equal(lib, rgba), f"{name}: libwebp and the crate's PNG differ"
            manifest[name] = alph_entry(exe, path, data, rgba)
        rgb = rgb_content(rng)
        seen = {}
        for cname, alpha in alpha_candidates(rng):
            for kw in ({"alpha_quality": 100, "method": 4}, {"alpha_quality": 100, "method": 0},
                       {"alpha_quality": 100, "method": 6}, {"alpha_quality": 50, "method": 4}):
                data = encode(rgb, alpha, **kw)
                if R.chunk(data, b"ALPH") is None:
                    continue
                path = os.path.join(tmp, "cand.webp")
                open(path, "wb").write(data)
                header, tf = transforms_of(exe, path)
                bits = None
                if 3 in tf:  # the index width follows the table size: tell the four apart by the file
                    lib = np.array(Image.open(io.BytesIO(data)).convert("RGBA"))[..., 3]
                    k = len(np.unique(lib))
                    bits = 1 if k <= 2 else 2 if k <= 4 else 4 if k <= 16 else 8
                key = (header, tuple(tf), bits)
                if key in seen or len(data) > 8192:
                    continue
                name = "alpha_h%02x_t%s%s.webp" % (header, "".join(map(str, tf)) or "none", f"_b{bits}" if bits else "")
                seen[key] = name
                open(os.path.join(out_dir, name), "wb").write(data)
                rgba = np.array(Image.open(io.BytesIO(data)).convert("RGBA"))
                manifest[name] = alph_entry(exe, os.path.join(out_dir, name), data, rgba)
                manifest[name]["source"] = f"{cname} {kw}"
        yy, xx = np.mgrid[0:H, 0:W]
        natural = np.dstack([rgb, np.clip(255 - np.hypot(xx - 30, yy - 30) * 4, 0, 255).astype(np.uint8)])
        pal = rng.integers(0, 256, (7, 4), dtype=np.uint8)
        lossless = {"ll_noise.webp": rng.integers(0, 256, (H, W, 4), dtype=np.uint8),
                    "ll_natural.webp": natural,
                    "ll_palette.webp": pal[rng.integers(0, 7, (H // 3 + 1, W // 3 + 1))].repeat(3, 0).repeat(3, 1)[:H, :W],
                    "ll_repeat.webp": np.tile(natural[:16, :16], (4, 7, 1))[:H, :W]}
        for name, img in lossless.items():
            b = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(img)).save(b, "WEBP", lossless=True, quality=100, method=6, exact=True)
            path = os.path.join(out_dir, name)
            open(path, "wb").write(b.getvalue())
            _, tf = transforms_of(exe, path)
            px = np.array(Image.open(io.BytesIO(b.getvalue())).convert("RGBA")).astype(np.uint32)
            argb = (px[..., 3] << 24) | (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]
            manifest[name] = {"kind": "vp8l", "width": img.shape[1], "height": img.shape[0], "transforms": tf,
                              "argb": R.sha(argb.astype("<u4"))}
    with open(os.path.join(ROOT, "tests", "golden", "decode_alpha.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, e in sorted(manifest.items()):
        print(name, e.get("header"), e["transforms"], os.path.getsize(os.path.join(out_dir, name)))


if __name__ == "__main__":
    main()
