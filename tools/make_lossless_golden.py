#!/usr/bin/env python3
"""Writes the lossless decode fixtures tests/golden/lossless/*.webp and their
manifest tests/golden/decode_lossless.json.  Runs on a developer machine with
libwebp behind PIL (the encoder and the yardstick decoder); the tests only read
what it wrote.

Images come from numpy formulas and one fixed seed.  libwebp's lossless encoder
chooses the transforms, so the generator asserts at the end that the manifest
covers what the tests need: colour indexing with 1, 2, 4 and 8 bit indices at a
width that is no multiple of the pack count, an image that takes predictor,
cross-colour and subtract-green together, varying alpha with the header bit
set, VP8X containers with and without the alpha flag around a stream whose
alpha varies, and the sizes 1x1, 1x70 and 70x1.

Manifest entry per file:
  width, height  the canvas
  has_alpha      what the container says (bit 28 of the VP8L header for a simple
                 file, the VP8X flag for an extended one)
  transforms     [[type, size_bits or table_size], ...] in bitstream order, read
                 with zwebp.dbg_vp8l_read_coded
  rgba           SHA-256 of libwebp's RGBA decode of the bare VP8L stream
  rgb            SHA-256 of its first three channels
A decoder's channel 3 is the stream's alpha when has_alpha is set and 255 when
it is not."""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-webp_amd"))
import zwebp  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lossless")
MANIFEST = os.path.join(ROOT, "tests", "golden", "decode_lossless.json")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "WEBP", lossless=True, quality=kw.get("quality", 75), method=kw.get("method", 4),
                              exact=True)
    return buf.getvalue()


def encode_with(arr, types):
    """The first of a few encoder settings whose stream carries every transform type of `types`."""
    for kw in ({"quality": 100, "method": 6}, {"quality": 75, "method": 4}, {"quality": 50, "method": 3},
               {"quality": 100, "method": 4}, {"quality": 25, "method": 2}):
        data = encode(arr, **kw)
        _, _, _, tfs = zwebp.dbg_vp8l_read_coded(vp8l_payload(data))
        if set(types) <= {t for t, _, _ in tfs}:
            return data
    raise SystemExit(f"no setting gives the transforms {types}")


def riff(chunks):
    body = b"WEBP"
    for cc, payload in chunks:
        body += cc + len(payload).to_bytes(4, "little") + payload + (b"\0" if len(payload) & 1 else b"")
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def vp8l_payload(data):
    pos = 12
    while pos + 8 <= len(data):
        size = int.from_bytes(data[pos + 4:pos + 8], "little")
        if data[pos:pos + 4] == b"VP8L":
            return data[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    raise SystemExit("no VP8L chunk")


def vp8x(payload, width, height, alpha_flag):
    head = bytes([0x10 if alpha_flag else 0, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + \
        (height - 1).to_bytes(3, "little")
    return riff([(b"VP8X", head), (b"VP8L", payload)])


def natural(w, h, rng, alpha=False, noise=1.0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    # one luminance term under all three channels (green predicts red and blue) and a little chroma
    lum = 128 + 80 * np.sin(xx / 17.0 + yy / 29.0) * np.cos(xx / 41.0 - yy / 13.0) + 20 * np.sin((xx + yy) / 5.0)
    r = lum + 14 * np.sin(xx / 23.0) + rng.normal(0, noise, (h, w))
    g = lum + rng.normal(0, noise, (h, w))
    b = lum - 18 * np.cos(yy / 19.0) + rng.normal(0, noise, (h, w))
    ch = [r, g, b]
    if alpha:
        ch.append(255 * (0.5 + 0.5 * np.sin(xx / 11.0) * np.cos(yy / 7.0)))
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def palette_image(w, h, ncolors, rng):
    table = rng.integers(0, 256, (ncolors, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    idx = ((xx // 3) * 13 + (yy // 2) * 29 + rng.integers(0, 3, (h, w))) % ncolors
    return table[idx]


def main():
    rng = np.random.default_rng(0x10551E55)
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for n in (2, 4, 16, 200):  # 67 columns: no multiple of 8, 4 or 2
        files[f"pal{n}_67x41.webp"] = encode(palette_image(67, 41, n, rng))
    files["natural_130x97.webp"] = encode_with(natural(130, 97, rng), (0, 1, 2))
    files["alpha_varies_96x64.webp"] = encode(natural(96, 64, rng, alpha=True))
    stream = vp8l_payload(encode(natural(75, 50, rng, alpha=True)))
    files["vp8x_alpha_flag_75x50.webp"] = vp8x(stream, 75, 50, True)
    files["vp8x_no_flag_alpha_in_stream_75x50.webp"] = vp8x(stream, 75, 50, False)
    files["one_1x1.webp"] = encode(natural(1, 1, rng))
    files["column_1x70.webp"] = encode(natural(1, 70, rng))
    files["row_70x1.webp"] = encode(natural(70, 1, rng))
    files["wide_300x200.webp"] = encode(natural(300, 200, rng, noise=0.0), quality=100, method=6)  # several bands of rows

    manifest = {}
    for name, data in sorted(files.items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        payload = vp8l_payload(data)
        bare = riff([(b"VP8L", payload)])
        rgba = np.asarray(Image.open(io.BytesIO(bare)).convert("RGBA"))
        info = zwebp.webp_parse(data, lossless=True)
        w, h, _, tfs = zwebp.dbg_vp8l_read_coded(payload)
        assert (w, h) == (rgba.shape[1], rgba.shape[0]) == (info["width"], info["height"])
        manifest[name] = {"width": w, "height": h, "has_alpha": int(info["has_alpha"]),
                          "vp8x": data[12:16] == b"VP8X", "transforms": [[t, b] for t, b, _ in tfs],
                          "rgba": sha(rgba), "rgb": sha(rgba[..., :3]),
                          "alpha_varies": bool((rgba[..., 3] != 255).any())}
        print(name, len(data), manifest[name]["transforms"], "alpha" if manifest[name]["has_alpha"] else "")
        assert len(data) <= 48 << 10, name

    e = manifest
    tables = sorted(b for v in e.values() for t, b in v["transforms"] if t == 3 and v["width"] == 67)
    assert [t <= 2 for t in tables].count(True) and any(2 < t <= 4 for t in tables) and \
        any(4 < t <= 16 for t in tables) and any(16 < t for t in tables), f"index widths 1, 2, 4, 8: {tables}"
    assert any({0, 1, 2} <= {t for t, _ in v["transforms"]} for v in e.values()), "predictor + cross-colour + green"
    assert any(v["has_alpha"] and v["alpha_varies"] and not v["vp8x"] for v in e.values()), "alpha, header bit"
    assert any(v["has_alpha"] and v["vp8x"] for v in e.values()), "VP8X with the alpha flag"
    assert any(not v["has_alpha"] and v["vp8x"] and v["alpha_varies"] for v in e.values()), "VP8X without it"
    for size in ((1, 1), (1, 70), (70, 1)):
        assert any((v["width"], v["height"]) == size for v in e.values()), size
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
