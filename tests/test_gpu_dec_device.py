"""Device-resident batch decode (zw_vp8_decode_batch_device, zwebp.decode_batch_device
/ decode_batch_device_ptr / decode_webp_batch_device): VP8 key frames straight into a
device tensor, HWC or CHW, u8 / f16 / f32, 3 or 4 channels.

Every expected value comes from the oracle (O.decode, then O.yuv_to_rgb_fancy /
O.yuv_to_rgb_simple); the float dtypes are float32(v) * float32(scale) + float32(bias)
(two rounded float32 operations), float16 = that rounded to nearest even.  Comparisons
are exact (array_equal over the whole output buffer, padding and guard included)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))

_CASES = r"""
import os
import struct
import sys
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp
import oracle_lib as O
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


_planes = {}


def reference(streams, w, h, ch, up, dtype):
    # [N, H, W, C] of `dtype` from the oracle's planes (decoded once per stream)
    imgs = []
    for s in streams:
        if s not in _planes:
            rc, r = O.decode(s)
            assert rc == 0
            _planes[s] = (r["y"], r["u"], r["v"])
        y, u, v = _planes[s]
        fn = O.yuv_to_rgb_fancy if up == BIL else O.yuv_to_rgb_simple
        imgs.append(np.asarray(fn(y, u, v, w, h, ch)).reshape(h, w, ch))
    u8 = np.stack(imgs)
    if dtype == "u8":
        return u8
    f = np.empty(u8.shape, np.float32)
    for c in range(ch):
        f[..., c] = u8[..., c].astype(np.float32) * np.float32(SCALE[c]) + np.float32(BIAS[c])
    return f if dtype == "f32" else f.astype(np.float16)


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
    # exact, and bit-exact for the float dtypes (no value compares equal to another encoding)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def case(name, streams, w, h, layout, dtype, ch, up=BIL, strides=None, offset=0, guard=0, tensor_out=False):
    # strides None: out=None (the library allocates); else a sentinel-filled buffer with
    # `offset` elements before the images and `guard` after capacity, through the raw-pointer
    # form (capacity = exactly the last addressed element + 1) or, tensor_out, a strided tensor
    global ncase
    n = len(streams)
    ref = reference(streams, w, h, ch, up, dtype)
    scale = SCALE[:ch] if dtype != "u8" else None
    bias = BIAS[:ch] if dtype != "u8" else None
    if strides is None:
        t = zwebp.decode_batch_device(streams, None, ch, layout, dtype, up, scale, bias, ctx=ctx)
        want_shape = (n, ch, h, w) if layout == "chw" else (n, h, w, ch)
        assert tuple(t.shape) == want_shape and t.dtype == TDT[dtype] and t.is_contiguous(), name
        got = t.cpu().numpy()
        exp = ref.transpose(0, 3, 1, 2) if layout == "chw" else ref
        assert same(got, np.ascontiguousarray(exp)), name
    else:
        fs, ps, rs = strides
        cap = span(n, w, h, ch, layout, fs, ps, rs)
        total = offset + cap + guard
        buf = torch.full((total,), SENT[dtype], dtype=TDT[dtype], device=dev)
        if tensor_out:
            shape, st = ((n, ch, h, w), (fs, ps, rs, 1)) if layout == "chw" else ((n, h, w, ch), (fs, rs, ch, 1))
            view = torch.as_strided(buf, shape, st, offset)
            r = zwebp.decode_batch_device(streams, view, upsampling=up, scale=scale, bias=bias, ctx=ctx)
            assert r is view, name
        else:
            torch.cuda.synchronize()
            dims = zwebp.decode_batch_device_ptr(streams, buf.data_ptr() + offset * buf.element_size(), cap, w, h, ch,
                                                 layout, dtype, up, scale, bias, fs, ps, rs, ctx=ctx)
            assert dims == (w, h), name
        got = buf.cpu().numpy()
        assert same(got, expected_buffer(total, offset, ref, layout, fs, ps, rs, dtype)), name
    assert zwebp.decode_rgb_kernel_ms(ctx=ctx) > 0, name
    assert zwebp.decode_stage_times(ctx=ctx)[1] == 0, name
    ncase += 1
    print("case", name, "ok", flush=True)


# ---- sizes: partial right-edge runs, odd widths, one-row images, one-MB-column frames ----
for (w, h) in ((1, 1), (7, 2), (8, 1), (9, 3), (17, 9)):
    st = synth_streams(w, h, 2, 0x5EED1000 + w * 256 + h)
    for layout, dtype, ch in (("hwc", "u8", 3), ("chw", "u8", 3), ("chw", "f16", 4), ("hwc", "f32", 3),
                              ("hwc", "u8", 4), ("chw", "f32", 3)):
        case(f"size {w}x{h} {layout} {dtype} c{ch}", st, w, h, layout, dtype, ch)

# ---- 161x97, n = 5: every layout x dtype x channels, fancy ----
W, H = 161, 97
S5 = synth_streams(W, H, 5, 0x5EED2000)
for layout in ("hwc", "chw"):
    for dtype in ("u8", "f16", "f32"):
        for ch in (3, 4):
            case(f"161x97 {layout} {dtype} c{ch}", S5, W, H, layout, dtype, ch)

# ---- simple upsampling ----
for (w, h) in ((17, 9), (9, 3)):
    st = synth_streams(w, h, 2, 0x5EED3000 + w)
    case(f"simple {w}x{h} hwc u8 c3", st, w, h, "hwc", "u8", 3, SIMPLE)
    case(f"simple {w}x{h} chw f32 c3", st, w, h, "chw", "f32", 3, SIMPLE)

# ---- goldens ----
rl = [open(os.path.join(GOLD, f"random_lossy_{i}.vp8"), "rb").read() for i in (1, 2, 3, 4)]
case("random_lossy chw f32 c3", rl, 99, 87, "chw", "f32", 3)
case("random_lossy hwc u8 c4", rl, 99, 87, "hwc", "u8", 4)
g1 = [open(os.path.join(GOLD, "gallery1_1.vp8"), "rb").read()]
case("gallery1_1 chw u8 c3", g1, 550, 368, "chw", "u8", 3)
case("gallery1_1 hwc f16 c3", g1, 550, 368, "hwc", "f16", 3)
case("gallery1_1 chw f16 c3 simple", g1, 550, 368, "chw", "f16", 3, SIMPLE)

# ---- padding: gaps and the guard after capacity keep the sentinel ----
rs = W * 3 + 13  # unaligned row starts
case("pad hwc u8 c3", S5, W, H, "hwc", "u8", 3, strides=(rs * H + 11, 0, rs), guard=64)
case("pad hwc u8 c3 tensor", S5, W, H, "hwc", "u8", 3, strides=(rs * H + 11, 0, rs), guard=64, tensor_out=True)
rs = W + 5
ps = H * rs + 7
case("pad chw f16 c3", S5, W, H, "chw", "f16", 3, strides=(3 * ps + 11, ps, rs), guard=64)
case("pad chw f16 c4 tensor", S5, W, H, "chw", "f16", 4, strides=(4 * ps + 11, ps, rs), guard=64, tensor_out=True)
# a base one element past its allocation (misaligned for every vector store)
for layout, dtype, ch in (("chw", "u8", 3), ("chw", "f32", 3), ("hwc", "f16", 4), ("hwc", "u8", 4), ("hwc", "f32", 3)):
    case(f"offset-1 {layout} {dtype} c{ch}", S5, W, H, layout, dtype, ch, strides=packed_strides(W, H, ch, layout),
         offset=1, guard=32, tensor_out=True)
case("offset-1 ptr chw f16 c3", S5, W, H, "chw", "f16", 3, strides=packed_strides(W, H, 3, "chw"), offset=1, guard=32)

# ---- pipeline knobs (read per call) ----
for key, val in (("ZW_DEC_CHUNK", "2"), ("ZW_DEC_TOKENS", "device"), ("ZW_DEC_ROWS", "0"), ("ZW_DEC_ROWS", "1")):
    os.environ[key] = val
    case(f"{key}={val} chw f16 c3", S5, W, H, "chw", "f16", 3)
    case(f"{key}={val} hwc u8 c3", S5, W, H, "hwc", "u8", 3)
    case(f"{key}={val} chw f32 c4 padded", S5, W, H, "chw", "f32", 4, strides=(4 * ps + 11, ps, rs), guard=16)
    del os.environ[key]

# ---- equality across entries ----
for ch in (3, 4):
    t = zwebp.decode_batch_device(S5, None, ch, "hwc", "u8", ctx=ctx).cpu().numpy()
    host = zwebp.decode_rgb_batch(S5, ch, BIL, ctx=ctx)
    assert all(np.array_equal(t[i], host[i]) for i in range(5)), ch
    print("case entries equal c%d ok" % ch, flush=True)

# ---- errors: refused before any launch (the sentinel-filled output stays untouched) ----
fs, ps0, rs0 = packed_strides(W, H, 3, "hwc")
cap = span(5, W, H, 3, "hwc", fs, 0, rs0)
buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def refused(name, code, streams=S5, ptr=None, capacity=cap, ch=3, layout="hwc", dtype="u8", fs=fs, ps=0, rs=rs0):
    try:
        zwebp.decode_batch_device_ptr(streams, buf.data_ptr() if ptr is None else ptr, capacity, W, H, ch, layout,
                                      dtype, BIL, None, None, fs, ps, rs, ctx=ctx)
    except zwebp.ZwError as e:
        assert e.code == code, (name, e.code)
    else:
        raise AssertionError(name + ": accepted")
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), name + ": output written"
    print("case refused", name, "ok", flush=True)


refused("capacity one short", 3, capacity=cap - 1)
refused("row stride short", 3, rs=W * 3 - 1)
refused("frames overlap", 3, fs=fs - 1)
cps, crs = packed_strides(W, H, 3, "chw")[1:]
refused("chw plane stride short", 3, layout="chw", fs=fs, ps=cps - 1, rs=crs)
refused("chw row stride short", 3, layout="chw", fs=fs, ps=cps, rs=crs - 1)
refused("channels 2", 3, ch=2)
refused("bad layout", 3, layout=2)
refused("bad dtype", 3, dtype=3)
refused("null data", 3, ptr=0)
small = synth_streams(17, 9, 1, 0x5EED4000)
refused("mixed sizes", 3, streams=S5[:4] + small)
refused("mixed sizes first", 3, streams=S5[:1] + small + S5[1:4])
pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
refused("pinned host memory", 3, ptr=pinned.data_ptr())
try:
    zwebp.decode_rgb_batch([S5[0][:20]], 3, BIL, ctx=ctx)
    raise AssertionError("truncated stream decoded")
except zwebp.DecodingError as e:
    trunc_code = e.code
assert trunc_code != 0
refused("truncated first stream", trunc_code, streams=[S5[0][:20]] + S5[1:])
cut = S5[1][:len(S5[1]) // 2]
try:
    zwebp.decode_rgb_batch([S5[0], cut], 3, BIL, ctx=ctx)
    raise AssertionError("cut stream decoded")
except zwebp.DecodingError as e:
    cut_code = e.code
try:
    zwebp.decode_batch_device_ptr([S5[0], cut], buf.data_ptr(), cap, W, H, 3, "hwc", "u8", ctx=ctx)
    raise AssertionError("cut stream accepted")
except zwebp.DecodingError as e:
    assert e.code == cut_code, (e.code, cut_code)
print("case cut stream ok", flush=True)

# the tensor form's own checks
good = torch.empty((5, 3, H, W), dtype=torch.uint8, device=dev)
for name, bad in (("host tensor", torch.empty((5, 3, H, W), dtype=torch.uint8)),
                  ("dtype", torch.empty((5, 3, H, W), dtype=torch.int32, device=dev)),
                  ("shape", torch.empty((5, 3, H, W + 1), dtype=torch.uint8, device=dev)),
                  ("channels", torch.empty((5, 2, H, W), dtype=torch.uint8, device=dev)),
                  ("batch", torch.empty((4, 3, H, W), dtype=torch.uint8, device=dev)),
                  ("column stride", torch.empty((5, 3, H, 2 * W), dtype=torch.uint8, device=dev)[..., ::2]),
                  ("permuted", torch.empty((5, H, W, 3), dtype=torch.uint8, device=dev).permute(0, 3, 1, 2))):
    try:
        zwebp.decode_batch_device(S5, bad, ctx=ctx)
    except ValueError:
        print("case ValueError", name, "ok", flush=True)
    else:
        raise AssertionError("tensor form accepted: " + name)
assert zwebp.decode_batch_device(S5, good, ctx=ctx) is good

# ---- containers ----
def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(*chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


files = [riff(chunk(b"VP8 ", s)) for s in S5]
t = zwebp.decode_webp_batch_device(files, channels=3, layout="chw", dtype="u8", ctx=ctx)
assert same(t.cpu().numpy(), np.ascontiguousarray(reference(S5, W, H, 3, BIL, "u8").transpose(0, 3, 1, 2)))
vp8x = bytes([0x10, 0, 0, 0]) + (W - 1).to_bytes(3, "little") + (H - 1).to_bytes(3, "little")
alph = riff(chunk(b"VP8X", vp8x), chunk(b"ALPH", b"\0" * 9), chunk(b"VP8 ", S5[0]))
try:
    zwebp.decode_webp_batch_device(files[:2] + [alph], ctx=ctx)
    raise AssertionError("VP8X + ALPH decoded")
except zwebp.DecodingError as e:
    assert e.code == 5, e.code
print("case containers ok", flush=True)
print("cases", ncase)
print("device decode ok")
"""


@pytest.mark.gpu
def test_gpu_decode_batch_device():
    """Every device-tensor case in one child process (torch's HIP runtime must initialise
    before the library's): sizes, every layout x dtype x channels, simple upsampling, the
    goldens, padded and misaligned outputs with sentinels, the pipeline knobs, equality with
    decode_rgb_batch, the refusals and the container entry."""
    r = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "device decode ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_import_needs_no_torch():
    """`import zwebp` (and loading the library) must not import torch: the device entry
    imports it on first use."""
    code = "import sys, zwebp; zwebp.load_library(); assert 'torch' not in sys.modules; print('no torch')"
    r = subprocess.run([sys.executable, "-c", code], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "no torch" in r.stdout, r.stdout + r.stderr
    import zwebp
    assert callable(zwebp.decode_batch_device) and callable(zwebp.decode_batch_device_ptr)
    assert callable(zwebp.decode_webp_batch_device)
    assert "zw_vp8_decode_batch_device" in {n for n, _, _ in zwebp.SIGNATURES}
