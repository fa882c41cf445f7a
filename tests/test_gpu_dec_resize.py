"""Device-resident batch decode with crop and resize (zw_vp8_decode_batch_device_resized,
zwebp.decode_batch_device_resized / _ptr / decode_webp_batch_device_resized): VP8 key
frames of mixed sizes into one device tensor of one size.

Every expected value comes from the oracle's planes (O.decode), its full-frame u8
RGB(A) image (O.yuv_to_rgb_fancy / O.yuv_to_rgb_simple) and the numpy restatement of
the integer resampling rule (resize_ref.py; the float dtypes in float32: S * 2^-16,
times scale, plus bias, float16 = that rounded to nearest even).  Comparisons are exact
(array_equal over the whole output buffer, sentinel padding and guard included)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))

_CASES = r"""
import os
import struct
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp
import oracle_lib as O
import resize_ref as R
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


def reference(streams, windows, ow, oh, ch, up, dtype):
    # [N, oh, ow, ch] of `dtype`
    imgs = []
    for i, s in enumerate(streams):
        rgb = full_rgb(s, ch, up)
        win = windows[i] if windows is not None and windows[i] is not None else (0, 0, rgb.shape[1], rgb.shape[0])
        imgs.append(R.resize(rgb, win, oh, ow, dtype, SCALE, BIAS))
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
                                              ctx=ctx)
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
                                                  ctx=ctx)
            assert r is view, name
        else:
            torch.cuda.synchronize()
            dims = zwebp.decode_batch_device_resized_ptr(streams, buf.data_ptr() + offset * buf.element_size(), cap,
                                                         ow, oh, windows, ch, layout, dtype, up, scale, bias, fs, ps,
                                                         rs, ctx=ctx)
            assert dims == [zwebp.vp8_frame_dims(s) for s in streams], name
        got = buf.cpu().numpy()
        assert same(got, expected_buffer(total, offset, ref, layout, fs, ps, rs, dtype)), name
    assert zwebp.decode_rgb_kernel_ms(ctx=ctx) > 0, name
    assert zwebp.decode_stage_times(ctx=ctx)[1:] == (0, 0), name
    ncase += 1
    print("case", name, "ok", flush=True)


FORMS = (("hwc", "u8", 3), ("chw", "u8", 3), ("chw", "f16", 4), ("hwc", "f32", 3), ("hwc", "u8", 4), ("chw", "f32", 3))

# ---- sizes: one pixel, down on one axis and up on the other, identity, widths around 8 and around the
# 64 columns of a wave, heights that end inside a wave's 4 rows and a workgroup's 16, upscaling, one row ----
S1 = synth_streams(1, 1, 2, 0x5EED5000)
S9 = synth_streams(9, 3, 2, 0x5EED5100)
S17 = synth_streams(17, 9, 2, 0x5EED5200)
S8 = synth_streams(8, 1, 2, 0x5EED5300)
W, H = 161, 97
S5 = synth_streams(W, H, 5, 0x5EED2000)
S5_OUTS = ((32, 24), (7, 5), (8, 5), (9, 5), (63, 16), (64, 17), (65, 21), (200, 130))
for streams, (sw, sh), outs in ((S1, (1, 1), ((1, 1), (3, 2))), (S9, (9, 3), ((4, 5),)), (S17, (17, 9), ((17, 9),)),
                                (S5[:2], (W, H), S5_OUTS), (S8, (8, 1), ((16, 1),))):
    for (ow, oh) in outs:
        for layout, dtype, ch in FORMS:
            case(f"size {sw}x{sh} -> {ow}x{oh} {layout} {dtype} c{ch}", streams, ow, oh, layout, dtype, ch)

# identity: a window of the output's size is decode_batch_device's tensor
for streams, (sw, sh) in ((S17, (17, 9)), (S5, (W, H))):
    for layout, dtype, ch in FORMS:
        sc = SCALE[:ch] if dtype != "u8" else None
        bi = BIAS[:ch] if dtype != "u8" else None
        a = zwebp.decode_batch_device(streams, None, ch, layout, dtype, BIL, sc, bi, ctx=ctx).cpu().numpy()
        b = zwebp.decode_batch_device_resized(streams, (sh, sw), None, None, ch, layout, dtype, BIL, sc, bi,
                                              ctx=ctx).cpu().numpy()
        assert same(a, b), (sw, sh, layout, dtype, ch)
print("case identity equals decode_batch_device ok", flush=True)

# ---- windows ----
case("window 1x1 far corner", S5[:2], 3, 2, windows=[(W - 1, H - 1, 1, 1)] * 2)
case("window 1x1 far corner hwc f32", S5[:2], 9, 4, "hwc", "f32", 3, windows=[(W - 1, H - 1, 1, 1)] * 2)
case("window odd origin", S5[:2], 32, 24, windows=[(33, 21, 50, 40)] * 2)
case("window odd origin hwc u8 c4", S5[:2], 32, 24, "hwc", "u8", 4, windows=[(33, 21, 51, 41)] * 2)
case("window right and bottom edge", S5[:2], 20, 15, windows=[(W - 40, H - 30, 40, 30)] * 2)
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
case("mixed windows", MIX, 16, 12, windows=[(3, 5, 90, 70), (1, 1, 15, 7), None, (0, 0, 9, 3), (0, 0, 1, 1), (16, 8, 1, 1)])
torch.cuda.synchronize()
mb = torch.empty((6, 3, 12, 16), dtype=torch.uint8, device=dev)
assert zwebp.decode_batch_device_resized_ptr(MIX, mb.data_ptr(), mb.numel(), 16, 12, ctx=ctx) == MIXD

# ---- formats: every layout x dtype x channels, simple upsampling ----
for layout in ("hwc", "chw"):
    for dtype in ("u8", "f16", "f32"):
        for ch in (3, 4):
            case(f"161x97 -> 32x24 {layout} {dtype} c{ch}", S5[:2], 32, 24, layout, dtype, ch)
case("simple 161x97 -> 32x24 hwc u8 c3", S5[:2], 32, 24, "hwc", "u8", 3, SIMPLE)
case("simple 161x97 -> 32x24 chw f32 c3", S5[:2], 32, 24, "chw", "f32", 3, SIMPLE)
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
# a base one element past its allocation (misaligned for every vector store)
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
rl = [open(os.path.join(GOLD, f"random_lossy_{i}.vp8"), "rb").read() for i in (1, 2, 3, 4)]
case("random_lossy -> 32x32 chw u8 c3", rl, 32, 32)
case("random_lossy -> 32x32 hwc f32 c3", rl, 32, 32, "hwc", "f32", 3)
case("goldens mixed -> 32x32", g1 + rl, 32, 32, "chw", "f32", 3)

# ---- refusals: code 3 before any launch (the sentinel-filled output stays untouched) ----
fs, ps0, rs0 = packed_strides(16, 12, 3, "chw")
cap = span(6, 16, 12, 3, "chw", fs, ps0, rs0)
buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def refused(name, code=3, streams=MIX, ptr=None, capacity=cap, ow=16, oh=12, windows=None):
    try:
        zwebp.decode_batch_device_resized_ptr(streams, buf.data_ptr() if ptr is None else ptr, capacity, ow, oh,
                                              windows, 3, "chw", "u8", BIL, None, None, fs, ps0, rs0, ctx=ctx)
    except zwebp.ZwError as e:
        assert e.code == code, (name, e.code)
    else:
        raise AssertionError(name + ": accepted")
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), name + ": output written"
    print("case refused", name, "ok", flush=True)


whole = [(0, 0, w, h) for (w, h) in MIXD]
refused("window x + w one past the width", windows=whole[:3] + [(1, 0, 9, 3)] + whole[4:])
refused("window y + h one past the height", windows=whole[:1] + [(0, 1, 17, 9)] + whole[2:])
refused("window zero width", windows=whole[:5] + [(0, 0, 0, 9)])
refused("window zero height", windows=[(0, 0, W, 0)] + whole[1:])
refused("out_w 0", ow=0)
refused("out_h 0", oh=0)
refused("capacity one short", capacity=cap - 1)
pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
refused("pinned host memory", ptr=pinned.data_ptr())
refused("null data", ptr=0)

# ---- errors: a cut stream inside a mixed batch reports the decoder's code ----
cut = S5[1][:len(S5[1]) // 2]
try:
    zwebp.decode_rgb_batch([S5[0], cut], 3, BIL, ctx=ctx)
    raise AssertionError("cut stream decoded")
except zwebp.DecodingError as e:
    cut_code = e.code
assert cut_code != 0
try:
    zwebp.decode_batch_device_resized_ptr([S5[0], S17[0], cut, S9[0], S1[0], S17[1]], buf.data_ptr(), cap, 16, 12,
                                          ctx=ctx)
    raise AssertionError("cut stream accepted")
except zwebp.DecodingError as e:
    assert e.code == cut_code, (e.code, cut_code)
try:
    zwebp.decode_rgb_batch([S5[0][:5]], 3, BIL, ctx=ctx)
    raise AssertionError("short stream decoded")
except zwebp.DecodingError as e:
    short_code = e.code
try:  # a frame too short for dimensions is not refused with code 3: its decode reports its own code
    zwebp.decode_batch_device_resized_ptr([S17[0], S5[0][:5], S17[1]], buf.data_ptr(), cap, 16, 12, ctx=ctx)
    raise AssertionError("short stream accepted")
except zwebp.DecodingError as e:
    assert e.code == short_code, (e.code, short_code)
print("case cut stream ok", flush=True)

# ---- the tensor form's own checks ----
good = torch.empty((6, 3, 12, 16), dtype=torch.uint8, device=dev)
for name, bad in (("host tensor", torch.empty((6, 3, 12, 16), dtype=torch.uint8)),
                  ("dtype", torch.empty((6, 3, 12, 16), dtype=torch.int32, device=dev)),
                  ("channels", torch.empty((6, 2, 12, 16), dtype=torch.uint8, device=dev)),
                  ("batch", torch.empty((5, 3, 12, 16), dtype=torch.uint8, device=dev)),
                  ("column stride", torch.empty((6, 3, 12, 32), dtype=torch.uint8, device=dev)[..., ::2]),
                  ("permuted", torch.empty((6, 12, 16, 3), dtype=torch.uint8, device=dev).permute(0, 3, 1, 2))):
    try:
        zwebp.decode_batch_device_resized(MIX, None, bad, ctx=ctx)
    except ValueError:
        print("case ValueError", name, "ok", flush=True)
    else:
        raise AssertionError("tensor form accepted: " + name)
try:
    zwebp.decode_batch_device_resized(MIX, (12, 17), good, ctx=ctx)
    raise AssertionError("size mismatch accepted")
except ValueError:
    pass
try:
    zwebp.decode_batch_device_resized(MIX, None, None, ctx=ctx)
    raise AssertionError("neither size nor out accepted")
except ValueError:
    pass
assert zwebp.decode_batch_device_resized(MIX, None, good, ctx=ctx) is good
assert zwebp.decode_batch_device_resized(MIX, (12, 16), good, ctx=ctx) is good
assert same(good.cpu().numpy(), np.ascontiguousarray(reference(MIX, None, 16, 12, 3, BIL, "u8").transpose(0, 3, 1, 2)))

# ---- containers ----
def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(*chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


files = [riff(chunk(b"VP8 ", s)) for s in MIX]
t = zwebp.decode_webp_batch_device_resized(files, (12, 16), channels=3, layout="chw", dtype="u8", ctx=ctx)
assert same(t.cpu().numpy(), np.ascontiguousarray(reference(MIX, None, 16, 12, 3, BIL, "u8").transpose(0, 3, 1, 2)))
print("case containers ok", flush=True)
print("cases", ncase)
print("resized decode ok")
"""


@pytest.mark.gpu
def test_gpu_decode_batch_device_resized():
    """Every crop-and-resize case in one child process (torch's HIP runtime must initialise
    before the library's): sizes, windows, mixed-size batches, every layout x dtype x
    channels, simple upsampling, padded and misaligned outputs with sentinels, the pipeline
    knobs, the goldens, the refusals, decoder errors, the tensor form and the container entry."""
    r = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "resized decode ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
