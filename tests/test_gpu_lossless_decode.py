"""Lossless (VP8L) files decoded into device tensors
(zw_webp_decode_batch_device / zw_webp_decode_ex with ZW_WEBP_LOSSLESS;
zwebp.decode_webp_batch_device / decode_rgba / decode_rgb / WebPDecoder with
lossless=True) against the digests of libwebp's decodes in
tests/golden/decode_lossless.json and tests/golden/decode_alpha.json.  All
comparisons are exact.

The cases run in one child process (torch's HIP runtime has to start before the
library loads, as in test_gpu_dec_device.py); each prints a line, and the tests
below look their lines up."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))
with open(os.path.join(ROOT, "tests", "golden", "decode_lossless.json")) as _f:
    NEW = sorted(json.load(_f))
with open(os.path.join(ROOT, "tests", "golden", "decode_alpha.json")) as _f:
    OLD = sorted(k for k, v in json.load(_f).items() if v["kind"] == "vp8l")
FILES = NEW + OLD

_CASES = r"""
import json
import os
import traceback
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp
import alpha_ref as R
from zwebp.synth import synth_rgba

HERE = os.path.dirname(os.path.abspath(R.__file__))
NEW = json.load(open(os.path.join(HERE, "golden", "decode_lossless.json")))
OLD = {k: v for k, v in json.load(open(os.path.join(HERE, "golden", "decode_alpha.json"))).items() if v["kind"] == "vp8l"}
TDT = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
SENT = {"u8": 0xA5, "f16": -1024.0, "f32": -12345.0}
SCALE = [1.0 / 58.0, 1.0 / 57.0, 1.0 / 57.5, 1.0 / 255.0]
BIAS = [-2.1, -2.0, -1.8, 0.125]
ctx = zwebp.Context(0)


def case(name, fn):
    try:
        fn()
        print("case", name, "ok", flush=True)
    except Exception:
        print("case", name, "FAIL", traceback.format_exc().replace("\n", " | "), flush=True)


def code_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except zwebp.DecodingError as e:
        return e.code
    except ValueError:
        return "ValueError"
    return 0


def read(name):
    folder = "lossless" if name in NEW else "alpha"
    return open(os.path.join(HERE, "golden", folder, name), "rb").read()


def riff(chunks):
    body = b"WEBP"
    for cc, payload in chunks:
        body += cc + len(payload).to_bytes(4, "little") + payload + (b"\0" if len(payload) & 1 else b"")
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def vp8x_lossless(payload, width, height, alpha_flag):
    head = bytes([0x10 if alpha_flag else 0, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + (height - 1).to_bytes(3, "little")
    return riff([(b"VP8X", head), (b"VP8L", payload)])


def expected(name):
    # (the file's RGBA as a decoder returns it, has_alpha): the host reader's image, checked
    # against the manifest's digest of libwebp's decode; alpha 255 without the container's flag
    data = read(name)
    info = zwebp.webp_parse(data, lossless=True)
    argb = zwebp.dbg_vp8l_decode(R.chunk(data, b"VP8L"))
    px = np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255, argb >> 24], -1).astype(np.uint8)
    if name in NEW:
        e = NEW[name]
        assert R.sha(px) == e["rgba"] and R.sha(px[..., :3]) == e["rgb"] and info["has_alpha"] == e["has_alpha"]
    else:
        assert R.sha(argb.astype("<u4")) == OLD[name]["argb"]
    if not info["has_alpha"]:
        px[..., 3] = 255
    return data, px, bool(info["has_alpha"])


def fixture(name):
    data, want, has_alpha = expected(name)
    h, w = want.shape[:2]
    e = NEW.get(name)

    def batch():
        t = zwebp.decode_webp_batch_device([data], None, 4, "hwc", "u8", lossless=True, ctx=ctx)
        assert tuple(t.shape) == (1, h, w, 4)
        got = t.cpu().numpy()[0]
        assert np.array_equal(got, want)
        if e is not None:
            assert R.sha(got[..., :3]) == e["rgb"]
            if has_alpha:
                assert R.sha(got) == e["rgba"]
        if not has_alpha:
            assert (got[..., 3] == 255).all()
        t = zwebp.decode_webp_batch_device([data, data], None, 3, "chw", "u8", lossless=True, ctx=ctx)
        assert tuple(t.shape) == (2, 3, h, w)
        chw = t.cpu().numpy()
        for i in range(2):
            assert np.array_equal(chw[i].transpose(1, 2, 0), want[..., :3])
            if e is not None:
                assert R.sha(chw[i].transpose(1, 2, 0)) == e["rgb"]
        ms = zwebp.decode_lossless_times(ctx=ctx)
        assert ms[0] > 0 and ms[2] > 0
        assert code_of(zwebp.decode_webp_batch_device, [data], None, 4, "hwc", "u8", ctx=ctx) == 5  # the default
        assert code_of(zwebp.decode_webp_batch_device, [data], None, 4, "hwc", "u8", alpha=True, ctx=ctx) == 5

    def single():
        img, gw, gh = zwebp.decode_rgba(data, ctx=ctx, lossless=True)
        assert (gw, gh) == (w, h) and np.array_equal(img.reshape(h, w, 4), want)
        img, gw, gh = zwebp.decode_rgb(data, ctx=ctx, lossless=True)
        assert (gw, gh) == (w, h) and np.array_equal(img.reshape(h, w, 3), want[..., :3])
        assert code_of(zwebp.decode_rgba, data, ctx=ctx) == 5 and code_of(zwebp.WebPDecoder, data, ctx=ctx) == 5
        d = zwebp.WebPDecoder(data, ctx=ctx, lossless=True)
        bpp = 4 if has_alpha else 3
        assert d.dimensions() == (w, h) and d.has_alpha() == has_alpha and d.is_lossy() is False
        assert d.output_buffer_size() == w * h * bpp
        assert np.array_equal(d.read_image().reshape(h, w, bpp), want[..., :bpp])
        buf = np.zeros(w * h * bpp, np.uint8)
        d.read_image(buf)
        assert np.array_equal(buf.reshape(h, w, bpp), want[..., :bpp])

    case(f"fixture {name} batch", batch)
    case(f"fixture {name} single", single)


for name in sorted(NEW) + sorted(OLD):
    fixture(name)


# ---- the float dtypes: the stated rule computed with torch on the u8 result ----
def floats(name, layout, dtype):
    data, want, _ = expected(name)
    u8 = torch.from_numpy(want).to(dev)
    v = u8.to(torch.float32) * torch.tensor(SCALE, dtype=torch.float32, device=dev)  # a rounded multiply
    v = v + torch.tensor(BIAS, dtype=torch.float32, device=dev)                      # then a rounded add
    v = v.to(TDT[dtype])                                                             # f16: round to nearest even
    if layout == "chw":
        v = v.permute(2, 0, 1)
    t = zwebp.decode_webp_batch_device([data], None, 4, layout, dtype, scale=SCALE, bias=BIAS, lossless=True, ctx=ctx)
    assert t.dtype == TDT[dtype] and torch.equal(t[0], v.contiguous())


for layout in ("hwc", "chw"):
    for dtype in ("f16", "f32"):
        case(f"floats {layout} {dtype}", lambda l=layout, d=dtype: floats("alpha_varies_96x64.webp", l, d))


# ---- a padded tensor keeps its sentinel in every gap ----
def padded(layout, dtype, ch):
    names = ["vp8x_alpha_flag_75x50.webp", "vp8x_no_flag_alpha_in_stream_75x50.webp", "vp8x_alpha_flag_75x50.webp"]
    files, wants = [], []
    for n in names:
        d, wnt, _ = expected(n)
        files.append(d)
        wants.append(wnt)
    H, W = wants[0].shape[:2]
    n = len(files)
    if layout == "hwc":
        rs = W * ch + 5
        fs, ps = rs * H + 11, 0
        one = (H - 1) * rs + W * ch
        shape, st = (n, H, W, ch), (fs, rs, ch, 1)
    else:
        rs = W + 3
        ps = rs * H + 7
        fs = ps * ch + 13
        one = (ch - 1) * ps + (H - 1) * rs + W
        shape, st = (n, ch, H, W), (fs, ps, rs, 1)
    offset, guard = 3, 64
    total = offset + (n - 1) * fs + one + guard
    scale, bias = (SCALE, BIAS) if dtype != "u8" else (None, None)
    want = torch.full((total,), SENT[dtype], dtype=TDT[dtype], device=dev)
    view = torch.as_strided(want, shape, st, offset)
    for i, wnt in enumerate(wants):
        v = torch.from_numpy(wnt[..., :ch].copy()).to(dev)
        if dtype != "u8":
            v = v.to(torch.float32) * torch.tensor(SCALE[:ch], dtype=torch.float32, device=dev)
            v = (v + torch.tensor(BIAS[:ch], dtype=torch.float32, device=dev)).to(TDT[dtype])
        view[i] = v if layout == "hwc" else v.permute(2, 0, 1)
    buf = torch.full((total,), SENT[dtype], dtype=TDT[dtype], device=dev)
    out = torch.as_strided(buf, shape, st, offset)
    r = zwebp.decode_webp_batch_device(files, out, scale=scale, bias=bias, lossless=True, ctx=ctx)
    assert r is out
    a, b = buf.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the whole buffer: pixels, untouched gaps and guard"


for layout in ("hwc", "chw"):
    for dtype, ch in (("u8", 4), ("u8", 3), ("f16", 4), ("f32", 3)):
        case(f"padded {layout} {dtype} {ch}", lambda l=layout, d=dtype, c=ch: padded(l, d, c))


# ---- lossy, lossless, lossy with alpha and lossless files of one size in one batch ----
W, H = 33, 17


def own_lossless(rgba_or_rgb, w, h):
    enc = zwebp.WebPEncoder(ctx=ctx)  # default params: lossless
    color = zwebp.ColorType.Rgba8 if rgba_or_rgb.shape[-1] == 4 else zwebp.ColorType.Rgb8
    return bytes(enc.encode(rgba_or_rgb, w, h, color))


def mixed():
    enc = zwebp.WebPEncoder(ctx=ctx)
    enc.set_params(zwebp.EncoderParams.lossy(60, 4))
    img = synth_rgba(W, H, 0x5EED0300, "natural").copy()
    img[..., 3] = (np.arange(W)[None, :] * 5 + np.arange(H)[:, None] * 11) % 256
    lossy = bytes(enc.encode(np.ascontiguousarray(img[..., :3]), W, H, zwebp.ColorType.Rgb8))
    vp8 = zwebp.encode_frame_lossy(synth_rgba(W, H, 0x5EED0301), W, H, zwebp.ColorType.Rgba8, 50, 4, ctx=ctx)
    lossy_alpha = R.webp_with_alph(vp8, R.raw_alph(img[..., 3], 1), W, H)
    ll_alpha = own_lossless(img, W, H)
    ll_rgb = own_lossless(np.ascontiguousarray(synth_rgba(W, H, 0x5EED0302)[..., :3]), W, H)
    files = [lossy, ll_alpha, lossy_alpha, ll_rgb, ll_alpha]
    kw = dict(alpha=True, lossless=True, ctx=ctx)
    singles = [zwebp.decode_webp_batch_device([f], None, 4, "hwc", "u8", **kw).cpu().numpy()[0] for f in files]
    assert np.array_equal(singles[1], img), "the product's own lossless file, alpha included"
    assert (singles[0][..., 3] == 255).all() and np.array_equal(singles[2][..., 3], img[..., 3])
    assert (singles[3][..., 3] == 255).all()
    for layout in ("hwc", "chw"):
        t = zwebp.decode_webp_batch_device(files, None, 4, layout, "u8", **kw).cpu().numpy()
        for i, s in enumerate(singles):
            got = t[i] if layout == "hwc" else t[i].transpose(1, 2, 0)
            assert np.array_equal(got, s), (layout, i)
    assert code_of(zwebp.decode_webp_batch_device, files, None, 3, "hwc", "u8", **kw) == 3  # ZW_WEBP_ALPHA needs 4
    t = zwebp.decode_webp_batch_device([lossy, ll_rgb], None, 3, "hwc", "u8", lossless=True, ctx=ctx).cpu().numpy()
    assert np.array_equal(t[0], singles[0][..., :3]) and np.array_equal(t[1], singles[3][..., :3])


case("mixed batch", mixed)


def roundtrip_300x200():
    rgba = synth_rgba(300, 200, 0x5EED0310, "natural").copy()
    rgba[..., 3] = (np.arange(300)[None, :] * 3 + np.arange(200)[:, None] * 7) % 256
    data = own_lossless(rgba, 300, 200)
    t = zwebp.decode_webp_batch_device([data, data], None, 4, "hwc", "u8", lossless=True, ctx=ctx).cpu().numpy()
    assert np.array_equal(t[0], rgba) and np.array_equal(t[1], rgba)
    img, w, h = zwebp.decode_rgba(data, ctx=ctx, lossless=True)
    assert (w, h) == (300, 200) and np.array_equal(img.reshape(200, 300, 4), rgba)


case("roundtrip 300x200", roundtrip_300x200)


def refusals():
    a = read("natural_130x97.webp")
    b = read("alpha_varies_96x64.webp")
    assert code_of(zwebp.decode_webp_batch_device, [a, b], None, 4, "hwc", "u8", lossless=True, ctx=ctx) in (3, "ValueError")
    payload = R.chunk(a, b"VP8L")
    cut = riff([(b"VP8L", payload[:len(payload) // 2])])
    assert code_of(zwebp.decode_webp_batch_device, [cut], None, 4, "hwc", "u8", lossless=True, ctx=ctx) == 15
    assert code_of(zwebp.decode_rgba, cut, ctx=ctx, lossless=True) == 15
    buf = torch.full((2, 97, 130, 4), 0xA5, dtype=torch.uint8, device=dev)
    assert code_of(zwebp.decode_webp_batch_device, [a, cut], buf, lossless=True, ctx=ctx) == 15
    assert (buf[1].cpu().numpy() == 0xA5).all(), "nothing of the damaged file's frame is written"
    bad = riff([(b"VP8L", b"\x2e" + payload[1:])])
    assert code_of(zwebp.decode_webp_batch_device, [bad], None, 4, "hwc", "u8", lossless=True, ctx=ctx) == 28
    assert code_of(zwebp.decode_webp_batch_device, [vp8x_lossless(b"\x2e" + payload[1:], 130, 97, False)], None, 4,
                   "hwc", "u8", lossless=True, ctx=ctx) == 28
    wrong = vp8x_lossless(payload, 131, 97, False)
    assert code_of(zwebp.decode_webp_batch_device, [wrong], None, 4, "hwc", "u8", lossless=True, ctx=ctx) == 21
    assert code_of(zwebp.decode_rgba, wrong, ctx=ctx, lossless=True) == 21
    assert code_of(zwebp.decode_webp_batch_device, [b], None, 3, "hwc", "u8", alpha=True, lossless=True, ctx=ctx) == 3
    # ... and the context still decodes
    _, want, _ = expected("natural_130x97.webp")
    t = zwebp.decode_webp_batch_device([a], None, 4, "hwc", "u8", lossless=True, ctx=ctx)
    assert np.array_equal(t.cpu().numpy()[0], want)


case("refusals", refusals)
print("done", flush=True)
"""


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=600)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "done" in out.stdout, text[-6000:]
    return {ln.split(" ok")[0].split(" FAIL")[0]: ln for ln in out.stdout.splitlines() if ln.startswith("case ")}


def _ok(lines, names):
    for n in names:
        assert f"case {n}" in lines, f"case {n} did not run"
        assert lines[f"case {n}"].endswith(" ok"), lines[f"case {n}"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_gpu_lossless_fixture(lines, name):
    _ok(lines, [f"fixture {name} batch", f"fixture {name} single"])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_gpu_lossless_floats(lines, layout, dtype):
    _ok(lines, [f"floats {layout} {dtype}"])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype,ch", [("u8", 4), ("u8", 3), ("f16", 4), ("f32", 3)])
def test_gpu_lossless_padded(lines, layout, dtype, ch):
    _ok(lines, [f"padded {layout} {dtype} {ch}"])


@pytest.mark.gpu
def test_gpu_lossless_mixed_batch(lines):
    _ok(lines, ["mixed batch"])


@pytest.mark.gpu
def test_gpu_lossless_roundtrip_300x200(lines):
    _ok(lines, ["roundtrip 300x200"])


@pytest.mark.gpu
def test_gpu_lossless_refusals(lines):
    _ok(lines, ["refusals"])
