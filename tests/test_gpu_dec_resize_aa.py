"""Antialiased downscaling in the device-resident crop-and-resize decode
(zw_vp8_decode_batch_device_resized_ex with ZW_RESIZE_TRIANGLE_AA; antialias=True on
zwebp.decode_batch_device_resized / _ptr / decode_webp_batch_device_resized).

Every expected value comes from the oracle's planes (O.decode), its full-frame u8 RGB(A)
image (O.yuv_to_rgb_fancy / O.yuv_to_rgb_simple) and the integer restatement of the
triangle rule (resize_aa_ref.py).  Comparisons are exact (array_equal over the whole
output buffer, sentinel padding and guard included)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))

_CASES = r"""
import ctypes
import os
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp
import oracle_lib as O
import resize_ref as R
import resize_aa_ref as A
from zwebp.synth import synth_rgba

GOLD = os.path.join(os.path.dirname(os.path.abspath(O.__file__)), "golden")
BIL, SIMPLE = zwebp.UpsamplingMethod.Bilinear, zwebp.UpsamplingMethod.Simple
NPDT = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
TDT = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
SENT = {"u8": 0xA5, "f16": -1024.0, "f32": -12345.0}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [1.0 / (255.0 * s) for s in STD] + [1.0 / 255.0]
BIAS = [-m / s for m, s in zip(MEAN, STD)] + [0.0]
ctx = zwebp.Context(0)
ncase = 0


def synth_streams(w, h, n, seed):
    out = []
    for i in range(n):
        rc, s, _ = O.encode(synth_rgba(w, h, seed + i), w, h, 3, 25 + 15 * i, 4)
        assert rc == 0
        out.append(s)
    return out


_rgb = {}


def full_rgb(s, ch, up):
    # the whole frame's u8 image [H, W, ch] from the oracle (computed once per stream and form)
    key = (s, ch, up)
    if key not in _rgb:
        rc, r = O.decode(s)
        assert rc == 0
        w, h = zwebp.vp8_frame_dims(s)
        fn = O.yuv_to_rgb_fancy if up == BIL else O.yuv_to_rgb_simple
        img = np.asarray(fn(r["y"], r["u"], r["v"], w, h, ch)).reshape(h, w, ch)
        img.setflags(write=False)
        _rgb[key] = img
    return _rgb[key]


def reference(streams, windows, ow, oh, ch, up, dtype, rule=A):
    # [N, oh, ow, ch] of `dtype`
    imgs = []
    for i, s in enumerate(streams):
        rgb = full_rgb(s, ch, up)
        win = windows[i] if windows is not None and windows[i] is not None else (0, 0, rgb.shape[1], rgb.shape[0])
        imgs.append(rule.resize(rgb, win, oh, ow, dtype, SCALE, BIAS))
    return np.stack(imgs)


def packed_strides(w, h, ch, layout):
    if layout == "hwc":
        return w * ch * h, 0, w * ch
    return ch * h * w, h * w, w


def span(n, w, h, ch, layout, fs, ps, rs):
    one = (h - 1) * rs + w * ch if layout == "hwc" else (ch - 1) * ps + (h - 1) * rs + w
    return (n - 1) * fs + one


def expected_buffer(total, offset, ref, layout, fs, ps, rs, dtype):
    e = np.full(total, SENT[dtype], NPDT[dtype])
    es = e.itemsize
    n, h, w, ch = ref.shape
    if layout == "hwc":
        v = np.lib.stride_tricks.as_strided(e[offset:], (n, h, w, ch), (fs * es, rs * es, ch * es, es))
        v[...] = ref
    else:
        v = np.lib.stride_tricks.as_strided(e[offset:], (n, ch, h, w), (fs * es, ps * es, rs * es, es))
        v[...] = ref.transpose(0, 3, 1, 2)
    return e


def same(a, b):
    # exact, and bit-exact for the float dtypes
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def case(name, streams, ow, oh, layout="chw", dtype="u8", ch=3, up=BIL, windows=None, strides=None, offset=0, guard=0,
         tensor_out=False):
    # strides None: out=None (the library allocates); else a sentinel-filled buffer with `offset`
    # elements before the images and `guard` after capacity, through the raw-pointer form
    # (capacity = exactly the last addressed element + 1) or, tensor_out, a strided tensor
    global ncase
    n = len(streams)
    ref = reference(streams, windows, ow, oh, ch, up, dtype)
    scale = SCALE[:ch] if dtype != "u8" else None
    bias = BIAS[:ch] if dtype != "u8" else None
    if strides is None:
        t = zwebp.decode_batch_device_resized(streams, (oh, ow), None, windows, ch, layout, dtype, up, scale, bias,
                                              ctx=ctx, antialias=True)
        want_shape = (n, ch, oh, ow) if layout == "chw" else (n, oh, ow, ch)
        assert tuple(t.shape) == want_shape and t.dtype == TDT[dtype] and t.is_contiguous(), name
        got = t.cpu().numpy()
        exp = ref.transpose(0, 3, 1, 2) if layout == "chw" else ref
        assert same(got, np.ascontiguousarray(exp)), name
    else:
        fs, ps, rs = strides
        cap = span(n, ow, oh, ch, layout, fs, ps, rs)
        total = offset + cap + guard
        buf = torch.full((total,), SENT[dtype], dtype=TDT[dtype], device=dev)
        if tensor_out:
            shape, st = ((n, ch, oh, ow), (fs, ps, rs, 1)) if layout == "chw" else ((n, oh, ow, ch), (fs, rs, ch, 1))
            view = torch.as_strided(buf, shape, st, offset)
            r = zwebp.decode_batch_device_resized(streams, None, view, windows, upsampling=up, scale=scale, bias=bias,
                                                  ctx=ctx, antialias=True)
            assert r is view, name
        else:
            torch.cuda.synchronize()
            dims = zwebp.decode_batch_device_resized_ptr(streams, buf.data_ptr() + offset * buf.element_size(), cap,
                                                         ow, oh, windows, ch, layout, dtype, up, scale, bias, fs, ps,
                                                         rs, ctx=ctx, antialias=True)
            assert dims == [zwebp.vp8_frame_dims(s) for s in streams], name
        got = buf.cpu().numpy()
        assert same(got, expected_buffer(total, offset, ref, layout, fs, ps, rs, dtype)), name
    assert zwebp.decode_rgb_kernel_ms(ctx=ctx) > 0, name
    assert zwebp.decode_stage_times(ctx=ctx)[1:] == (0, 0), name
    ncase += 1
    print("case", name, "ok", flush=True)


FORMS = (("hwc", "u8", 3), ("chw", "u8", 3), ("chw", "f16", 4), ("hwc", "f32", 3), ("hwc", "u8", 4), ("chw", "f32", 3))

# ---- sizes: down by 5 and by 23, the edges of 64 columns and 16 rows, upscaling, a ratio just above 1,
# one output pixel (161 taps: more than a wave), 2 x 3; one pixel up, down on one axis and up on the other,
# one row, identity; the edges of a workgroup's 256 columns ----
S1 = synth_streams(1, 1, 2, 0x5EED5000)
S9 = synth_streams(9, 3, 2, 0x5EED5100)
S17 = synth_streams(17, 9, 2, 0x5EED5200)
S8 = synth_streams(8, 1, 2, 0x5EED5300)
W, H = 161, 97
S5 = synth_streams(W, H, 5, 0x5EED2000)
S5_OUTS = ((32, 24), (7, 5), (63, 16), (64, 17), (65, 21), (200, 130), (160, 96), (1, 1), (2, 3))
for streams, (sw, sh), outs in ((S5[:2], (W, H), S5_OUTS), (S1, (1, 1), ((3, 2),)), (S9, (9, 3), ((4, 5),)),
                                (S8, (8, 1), ((16, 1),)), (S17, (17, 9), ((17, 9),))):
    for (ow, oh) in outs:
        for layout, dtype, ch in FORMS:
            case(f"size {sw}x{sh} -> {ow}x{oh} {layout} {dtype} c{ch}", streams, ow, oh, layout, dtype, ch)
for (ow, oh) in ((255, 15), (256, 16), (257, 33)):
    case(f"size {W}x{H} -> {ow}x{oh} chw u8 c3", S5[:1], ow, oh)
    case(f"size {W}x{H} -> {ow}x{oh} hwc f16 c4", S5[:1], ow, oh, "hwc", "f16", 4)
# a span wider than the rows held on chip at once is taken in pieces: taps across the seam
SW = synth_streams(2100, 5, 1, 0x5EED5400)
case("size 2100x5 -> 3x2 chw u8 c3", SW, 3, 2)
case("size 2100x5 -> 300x2 hwc f32 c3", SW, 300, 2, "hwc", "f32", 3)
case("size 2100x5 -> 1x1 chw f32 c4", SW, 1, 1, "chw", "f32", 4)

# identity: a window of the output's size is decode_batch_device's tensor
for streams, (sw, sh) in ((S17, (17, 9)), (S5, (W, H))):
    for layout in ("hwc", "chw"):
        for dtype in ("u8", "f16", "f32"):
            for ch in (3, 4):
                sc = SCALE[:ch] if dtype != "u8" else None
                bi = BIAS[:ch] if dtype != "u8" else None
                a = zwebp.decode_batch_device(streams, None, ch, layout, dtype, BIL, sc, bi, ctx=ctx).cpu().numpy()
                b = zwebp.decode_batch_device_resized(streams, (sh, sw), None, None, ch, layout, dtype, BIL, sc, bi,
                                                      ctx=ctx, antialias=True).cpu().numpy()
                assert same(a, b), (sw, sh, layout, dtype, ch)
print("case identity equals decode_batch_device ok", flush=True)

# ---- windows ----
case("window 1x1 far corner", S5[:2], 3, 2, windows=[(W - 1, H - 1, 1, 1)] * 2)
case("window 1x1 far corner hwc f32", S5[:2], 9, 4, "hwc", "f32", 3, windows=[(W - 1, H - 1, 1, 1)] * 2)
case("window odd origin", S5[:2], 32, 24, windows=[(33, 21, 50, 40)] * 2)
case("window odd origin hwc u8 c4", S5[:2], 32, 24, "hwc", "u8", 4, windows=[(33, 21, 51, 41)] * 2)
case("window odd origin down 7x", S5[:2], 11, 9, windows=[(3, 5, 151, 89)] * 2)
case("window right and bottom edge", S5[:2], 20, 15, windows=[(W - 40, H - 30, 40, 30)] * 2)
case("window right and bottom edge down", S5[:2], 9, 7, windows=[(W - 99, H - 71, 99, 71)] * 2)
case("window per frame", S5[:3], 16, 12, "chw", "f16", 3, windows=[(1, 3, 100, 60), (60, 0, 101, 97), None])
case("window of output size", S5[:2], 32, 24, windows=[(5, 7, 32, 24), (129, 73, 32, 24)])
case("window odd origin simple", S5[:2], 32, 24, "chw", "u8", 3, SIMPLE, windows=[(33, 21, 50, 40)] * 2)

# ---- mixed sizes: grouping and the slot mapping ----
MIX = [S5[0], S17[0], S5[1], S9[0], S1[0], S17[1]]
MIXD = [(W, H), (17, 9), (W, H), (9, 3), (1, 1), (17, 9)]
assert [zwebp.vp8_frame_dims(s) for s in MIX] == MIXD
case("mixed chw u8 c3", MIX, 16, 12)
case("mixed hwc f32 c4", MIX, 16, 12, "hwc", "f32", 4)
case("mixed ptr chw f16 c3", MIX, 16, 12, "chw", "f16", 3, strides=packed_strides(16, 12, 3, "chw"), guard=16)
case("mixed padded chw u8 c3", MIX, 16, 12, strides=(3 * (12 * 19 + 5) + 7, 12 * 19 + 5, 19), guard=16)
MIXW = [(3, 5, 90, 70), (1, 1, 15, 7), None, (0, 0, 9, 3), (0, 0, 1, 1), (16, 8, 1, 1)]
case("mixed windows", MIX, 16, 12, windows=MIXW)
case("mixed windows padded hwc f16 c4", MIX, 16, 12, "hwc", "f16", 4, windows=MIXW, strides=(12 * 71 + 9, 0, 71), guard=16)
case("mixed windows padded chw f32 c3 tensor", MIX, 16, 12, "chw", "f32", 3, windows=MIXW,
     strides=(3 * (12 * 18 + 3) + 5, 12 * 18 + 3, 18), guard=16, tensor_out=True)

# ---- formats: every layout x dtype x channels, simple upsampling ----
for layout in ("hwc", "chw"):
    for dtype in ("u8", "f16", "f32"):
        for ch in (3, 4):
            case(f"161x97 -> 32x24 {layout} {dtype} c{ch}", S5[:2], 32, 24, layout, dtype, ch)
            case(f"simple 161x97 -> 32x24 {layout} {dtype} c{ch}", S5[:2], 32, 24, layout, dtype, ch, SIMPLE)
case("simple 9x3 -> 4x5 chw f16 c4", S9, 4, 5, "chw", "f16", 4, SIMPLE)

# ---- padding: gaps and the guard after capacity keep the sentinel ----
OW, OH = 33, 24
rs = OW * 3 + 13  # unaligned row starts
case("pad hwc u8 c3", S5, OW, OH, "hwc", "u8", 3, strides=(rs * OH + 11, 0, rs), guard=64)
case("pad hwc u8 c3 tensor", S5, OW, OH, "hwc", "u8", 3, strides=(rs * OH + 11, 0, rs), guard=64, tensor_out=True)
rs = OW + 5
ps = OH * rs + 7
case("pad chw f16 c3", S5, OW, OH, "chw", "f16", 3, strides=(3 * ps + 11, ps, rs), guard=64)
case("pad chw f16 c4 tensor", S5, OW, OH, "chw", "f16", 4, strides=(4 * ps + 11, ps, rs), guard=64, tensor_out=True)
case("pad mixed chw f32 c3", MIX, 16, 12, "chw", "f32", 3, strides=(3 * (12 * 21 + 7) + 11, 12 * 21 + 7, 21), guard=64)
# a base one element past its allocation
for layout, dtype, ch in (("chw", "u8", 3), ("chw", "f32", 3), ("hwc", "f16", 4), ("hwc", "u8", 4), ("hwc", "f32", 3)):
    case(f"offset-1 {layout} {dtype} c{ch}", S5, 32, OH, layout, dtype, ch, strides=packed_strides(32, OH, ch, layout),
         offset=1, guard=32, tensor_out=True)
case("offset-1 ptr chw f16 c3", S5, 32, OH, "chw", "f16", 3, strides=packed_strides(32, OH, 3, "chw"), offset=1, guard=32)

# ---- pipeline knobs (read per call) ----
for key, val in (("ZW_DEC_CHUNK", "2"), ("ZW_DEC_TOKENS", "device")):
    os.environ[key] = val
    case(f"{key}={val} mixed chw f16 c3", MIX + S5[2:], 16, 12, "chw", "f16", 3)
    case(f"{key}={val} mixed hwc u8 c3 padded", MIX + S5[2:], 16, 12, "hwc", "u8", 3, strides=(16 * 3 * 12 + 29, 0, 16 * 3 + 2),
         guard=16)
    del os.environ[key]

# ---- goldens ----
g1 = [open(os.path.join(GOLD, "gallery1_1.vp8"), "rb").read()]
case("gallery1_1 -> 224x224 chw f16 c3", g1, 224, 224, "chw", "f16", 3)
case("gallery1_1 -> 32x32 chw u8 c3", g1, 32, 32)
rl = [open(os.path.join(GOLD, f"random_lossy_{i}.vp8"), "rb").read() for i in (1, 2, 3, 4)]
case("random_lossy -> 32x32 chw u8 c3", rl, 32, 32)
case("random_lossy -> 32x32 hwc f32 c3", rl, 32, 32, "hwc", "f32", 3)
case("goldens mixed -> 32x32", g1 + rl, 32, 32, "chw", "f32", 3)

# ---- a bad filter value: code 3 before any launch (the sentinel-filled output stays untouched) ----
fs, ps0, rs0 = packed_strides(16, 12, 3, "chw")
cap = span(6, 16, 12, 3, "chw", fs, ps0, rs0)
buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
for bad in (2, -1, 255):
    try:
        zwebp.decode_batch_device_resized_ptr(MIX, buf.data_ptr(), cap, 16, 12, None, 3, "chw", "u8", BIL, None, None, fs,
                                              ps0, rs0, ctx=ctx, antialias=bad)
    except zwebp.ZwError as e:
        assert e.code == 3, (bad, e.code)
    else:
        raise AssertionError(f"filter {bad} accepted")
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), f"filter {bad}: output written"
print("case bad filter refused ok", flush=True)

# ---- antialias=False through the _ex entry is the existing entry's tensor (and the two-tap rule's) ----
L = zwebp.load_library()
arrs = [np.frombuffer(s, np.uint8) for s in MIX]
ptrs = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in arrs])
lens = (ctypes.c_size_t * 6)(*[a.size for a in arrs])
for layout, dtype, ch in FORMS:
    sc = SCALE[:ch] if dtype != "u8" else None
    bi = BIAS[:ch] if dtype != "u8" else None
    new = zwebp.decode_batch_device_resized(MIX, (12, 16), None, None, ch, layout, dtype, BIL, sc, bi, ctx=ctx,
                                            antialias=False)
    old = torch.full_like(new, SENT[dtype])
    lay = 0 if layout == "hwc" else 1
    f_s, p_s, r_s = packed_strides(16, 12, ch, layout)
    di = zwebp._DeviceImages(old.data_ptr(), old.numel(), lay, {"u8": 0, "f16": 1, "f32": 2}[dtype], ch, int(BIL), f_s, p_s,
                             r_s, (ctypes.c_float * 4)(*(list(sc or [1.0] * ch) + [1.0] * (4 - ch))),
                             (ctypes.c_float * 4)(*(list(bi or [0.0] * ch) + [0.0] * (4 - ch))))
    torch.cuda.synchronize()
    assert L.zw_vp8_decode_batch_device_resized(ctx.handle, 6, ptrs, lens, ctypes.byref(di), 16, 12, None, None, None) == 0
    want = reference(MIX, None, 16, 12, ch, BIL, dtype, rule=R)
    want = np.ascontiguousarray(want.transpose(0, 3, 1, 2) if layout == "chw" else want)
    assert same(new.cpu().numpy(), old.cpu().numpy()) and same(new.cpu().numpy(), want), (layout, dtype, ch)
print("case antialias=False equals the existing entry ok", flush=True)

# ---- containers ----
import struct


def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(*chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


files = [riff(chunk(b"VP8 ", s)) for s in MIX]
t = zwebp.decode_webp_batch_device_resized(files, (12, 16), channels=3, layout="chw", dtype="u8", ctx=ctx, antialias=True)
assert same(t.cpu().numpy(), np.ascontiguousarray(reference(MIX, None, 16, 12, 3, BIL, "u8").transpose(0, 3, 1, 2)))
print("case containers ok", flush=True)
print("cases", ncase)
print("antialiased resized decode ok")
"""


@pytest.mark.gpu
def test_gpu_decode_batch_device_resized_antialias():
    """Every antialiased crop-and-resize case in one child process (torch's HIP runtime must
    initialise before the library's): sizes on both sides of the column-block and row-band
    edges, one output pixel, spans taken in pieces, identity, windows, mixed-size batches, every
    layout x dtype x channels with both upsamplers, padded and misaligned outputs with
    sentinels, the pipeline knobs, the goldens, a bad filter value, and antialias=False against
    the existing entry."""
    r = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "antialiased resized decode ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
