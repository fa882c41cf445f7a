"""Device-resident batch encode (zw_encode_batch_device, zw_pipe_set_input_device;
zwebp.encode_batch_device / encode_batch_device_ptr / encode_webp_batch_device /
Pipeline.set_input): frames read straight from a device tensor, HWC or CHW, u8 / f16 /
f32, 3 or 4 channels.

Every expected bitstream is the oracle's (O.encode) of the u8 HWC image numpy makes by
the pixel rule: float32 multiply, float32 add, rint(clip(t, 0, 255)) with NaN -> 0.
Comparisons are exact equality of bitstreams.  Padding and guard elements hold NaN
(float dtypes) or 0xA5 (u8), so a kernel that reads them as pixels changes the stream;
the whole source buffer must be bit-identical after every call."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "image-webp_amd"), os.path.join(ROOT, "tests")]))

_CASES = r"""
import os
import numpy as np
import torch                      # torch's HIP runtime first, then the library (as bench.py does)
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import zwebp
import oracle_lib as O
from zwebp.synth import synth_rgba

NPDT = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [255.0 * s for s in STD]          # x = (v / 255 - mean) / std  ->  v = x * (255 std) + 255 mean
BIAS = [255.0 * m for m in MEAN]
RGB = zwebp.ColorType.Rgb8
ctx = zwebp.Context(0)
ncase = 0


def rule(x, scale=None, bias=None):
    # [..., C >= 3] elements -> [..., 3] u8 by the pixel rule
    x = np.asarray(x)[..., :3]
    if x.dtype == np.uint8:
        return np.ascontiguousarray(x)
    s = np.broadcast_to(np.asarray(1.0 if scale is None else scale, np.float64).reshape(-1)[:3], (3,)).astype(np.float32)
    b = np.broadcast_to(np.asarray(0.0 if bias is None else bias, np.float64).reshape(-1)[:3], (3,)).astype(np.float32)
    with np.errstate(all="ignore"):
        t = x.astype(np.float32) * s
        t = t + b
        r = np.rint(np.clip(t, np.float32(0), np.float32(255)))
    r[np.isnan(t)] = 0
    return r.astype(np.uint8)


_enc = {}


def expected(imgs, q=75, m=4, nparts=1):
    out = []
    for im in imgs:
        h, w = im.shape[:2]
        key = (im.tobytes(), w, h, q, m, nparts)
        if key not in _enc:
            rc, s, _ = O.encode(im, w, h, RGB, q, m, nparts=nparts)
            assert rc == 0
            _enc[key] = s
        out.append(_enc[key])
    return out


def frames_u8(n, w, h, seed, ch):
    # [n, h, w, ch] u8: synth colours, distinct per frame; channel 3 is noise
    f = np.stack([synth_rgba(w, h, seed + i) for i in range(n)])
    if ch == 4:
        f[..., 3] = np.stack([synth_rgba(w, h, seed + 77 + i, kind="noise")[..., 0] for i in range(n)])
    return np.ascontiguousarray(f[..., :ch])


def as_dtype(u8, dtype):
    # elements of `dtype` whose rule image is u8's colours, with (scale, bias)
    ch = u8.shape[-1]
    if dtype == "u8":
        return u8, None, None
    if dtype == "f16":      # v / 255 in f16, scale 255: the round trip is exact
        x = (u8.astype(np.float32) / np.float32(255)).astype(np.float16)
        return x, 255.0, None
    x = np.empty(u8.shape, np.float32)    # normalised: (v / 255 - mean) / std, undone by SCALE / BIAS
    for c in range(ch):
        mc, sc = (MEAN[c], STD[c]) if c < 3 else (0.5, 0.25)
        x[..., c] = (u8[..., c].astype(np.float32) / np.float32(255) - np.float32(mc)) / np.float32(sc)
    return x, SCALE, BIAS


def place(x, layout, rp=0, pp=0, fp=0, offset=0, guard=0):
    # x [n, h, w, ch] -> (host buffer, device buffer, strided device view of it); the gaps
    # (row + rp, plane + pp, frame + fp elements, `offset` before, `guard` after) hold NaN / 0xA5
    n, h, w, ch = x.shape
    if layout == "hwc":
        rs = w * ch + rp
        one = (h - 1) * rs + w * ch
        fs = one + fp if fp or n == 1 else rs * h
        fs = max(fs, one)
        shape, st = (n, h, w, ch), (fs, rs, ch, 1)
    else:
        rs = w + rp
        ps = (h - 1) * rs + w + pp if pp else rs * h
        one = (ch - 1) * ps + (h - 1) * rs + w
        fs = one + fp if fp else ps * ch
        shape, st = (n, ch, h, w), (fs, ps, rs, 1)
    total = offset + (n - 1) * fs + one + guard
    host = np.full(total, 0xA5 if x.dtype == np.uint8 else np.nan, x.dtype)
    es = host.itemsize
    v = np.lib.stride_tricks.as_strided(host[offset:], shape, tuple(s * es for s in st))
    v[...] = x if layout == "hwc" else x.transpose(0, 3, 1, 2)
    buf = torch.from_numpy(host.copy()).to(dev)
    return host, buf, torch.as_strided(buf, shape, st, offset)


def unchanged(host, buf):
    return np.array_equal(buf.cpu().numpy().view(np.uint8), host.view(np.uint8))


def case(name, x, layout, scale=None, bias=None, q=75, m=4, nparts=1, want=None, **pad):
    global ncase
    host, buf, view = place(x, layout, **pad)
    want = expected(rule(x, scale, bias), q, m, nparts) if want is None else want
    got = zwebp.encode_batch_device(view, q, m, layout, scale, bias, nparts, ctx=ctx)
    assert len(got) == len(want), name
    for i, (g, e) in enumerate(zip(got, want)):
        assert g == e, f"{name}: frame {i} differs ({len(g)} vs {len(e)} bytes)"
    assert unchanged(host, buf), name + ": the source tensor changed"
    ncase += 1
    print("case", name, "ok", flush=True)


# ---- non-vacuity: a channel or layout mix-up changes the expected streams ----
W, H = 40, 24
base = frames_u8(1, W, H, 0x5EED5000, 3)[0]
e0 = expected([base])[0]
assert expected([np.ascontiguousarray(base[..., ::-1])])[0] != e0
misread = np.ascontiguousarray(base.reshape(-1).reshape(3, H, W).transpose(1, 2, 0))   # HWC bytes read as CHW
assert expected([misread])[0] != e0
print("case non-vacuity ok", flush=True)

# ---- sizes ----
for (w, h) in ((1, 1), (16, 16), (37, 21), (40, 24), (72, 40)):
    u8 = frames_u8(2, w, h, 0x5EED5100 + w, 4)
    for layout, dtype, ch in (("chw", "u8", 3), ("hwc", "u8", 4), ("chw", "f16", 3), ("hwc", "f32", 3)):
        x, s, b = as_dtype(u8[..., :ch], dtype)
        case(f"size {w}x{h} {layout} {dtype} c{ch}", x, layout, s, b)

# ---- layouts x dtypes x channels, packed, odd and aligned sizes ----
for (w, h) in ((37, 21), (40, 24)):
    u8 = frames_u8(2, w, h, 0x5EED5200 + w, 4)
    want3 = expected(u8[..., :3])
    for layout in ("hwc", "chw"):
        for dtype in ("u8", "f16", "f32"):
            for ch in (3, 4):
                x, s, b = as_dtype(u8[..., :ch], dtype)
                if dtype != "f32":     # exact round trips: the u8 image's streams, 3 or 4 channels
                    assert np.array_equal(rule(x, s, b), u8[..., :3])
                    case(f"{w}x{h} {layout} {dtype} c{ch}", x, layout, s, b, want=want3)
                else:
                    case(f"{w}x{h} {layout} {dtype} c{ch}", x, layout, s, b)
    # 4 channels: the stream is the 3-channel one whatever channel 3 holds (NaN and inf too)
    x4, s, b = as_dtype(u8, "f32")
    x4[..., 3] = np.where(u8[..., 3] & 1, np.nan, np.inf)
    case(f"{w}x{h} hwc f32 c4 alpha NaN/inf", x4, "hwc", s, b, want=expected(rule(x4[..., :3], s, b)))
    case(f"{w}x{h} chw f32 c4 alpha NaN/inf", x4, "chw", s, b, want=expected(rule(x4[..., :3], s, b)))

# ---- strided tensors at 40x24: row / plane / frame padding, a misaligned base; one aligned padding ----
u8 = frames_u8(3, W, H, 0x5EED5300, 4)
for layout, dtype, ch in (("chw", "u8", 3), ("chw", "f32", 3), ("chw", "f16", 4), ("hwc", "u8", 3), ("hwc", "u8", 4),
                          ("hwc", "f16", 3), ("hwc", "f32", 4)):
    x, s, b = as_dtype(u8[..., :ch], dtype)
    tag = f"{layout} {dtype} c{ch}"
    case("row pad +3 " + tag, x, layout, s, b, rp=3, guard=8)
    if layout == "chw":
        case("plane pad +5 " + tag, x, layout, s, b, pp=5, guard=8)
    case("frame pad +7 " + tag, x, layout, s, b, fp=7, guard=8)
    case("offset 1 " + tag, x, layout, s, b, offset=1, guard=8)
    case("all pads " + tag, x, layout, s, b, rp=3, pp=5 if layout == "chw" else 0, fp=7, offset=1, guard=8)
    # every stride and the base stay multiples of 16 elements: the vector form, with gaps
    case("aligned pads " + tag, x, layout, s, b, rp=16, pp=32 if layout == "chw" else 0, fp=64, offset=16, guard=16)

# ---- float rule: every tie, the clamps, NaN and inf ----
ks = np.arange(256, dtype=np.float32)
vals = np.concatenate([ks + np.float32(0.5), ks - np.float32(0.5), ks + np.float32(0.49), ks - np.float32(0.49),
                       np.asarray([-1e9, -3.0, -0.75, -0.0, 255.75, 256.5, 300.0, 1e9, np.nan, np.inf, -np.inf,
                                   1e-45, 254.5, 255.5], np.float32)])
rng = np.random.default_rng(0x5EED54)
ties = rng.permutation(np.resize(vals, 2 * H * W * 3)).reshape(2, H, W, 3).astype(np.float32)
img = rule(ties)
assert img.min() == 0 and img.max() == 255 and len(np.unique(img)) == 256
for layout in ("hwc", "chw"):
    case(f"ties f32 {layout}", ties, layout)
    case(f"ties f32 {layout} unaligned", ties, layout, offset=1, guard=4)
    # the same values behind a scale and a bias: x = (t - bias) / scale lands near the ties again
    xs = ((ties - np.asarray(BIAS, np.float32)) / np.asarray(SCALE, np.float32)).astype(np.float32)
    case(f"ties f32 {layout} scale/bias", xs, layout, SCALE, BIAS)
h16 = ties.astype(np.float16)     # halves and quarters survive f16 up to 255.5 / 127.75
case("ties f16 chw", h16, "chw")
case("ties f16 hwc scale 0.5 bias 0.25", h16, "hwc", 0.5, 0.25)
u8 = frames_u8(2, W, H, 0x5EED5500, 3)
x16, s, b = as_dtype(u8, "f16")
case("f16 v/255 scale 255 == u8 streams", x16, "chw", s, b, want=expected(u8))

# ---- frame indexing: chunks and lanes start at the right frame ----
for (w, h) in ((16, 16), (37, 21)):
    for n, key, val in ((1, None, None), (3, None, None), (5, "ZW_PIPE_CHUNK", "2"), (16, "ZW_PIPE_LANES", "2")):
        u8 = frames_u8(n, w, h, 0x5EED5600 + 32 * w + n, 4)
        assert len(set(expected(u8[..., :3]))) == n      # every frame distinct
        if key:
            os.environ[key] = val
        for layout, dtype, ch in (("chw", "f16", 3), ("hwc", "u8", 4)):
            x, s, b = as_dtype(u8[..., :ch], dtype)
            case(f"n={n} {key}={val} {w}x{h} {layout} {dtype} c{ch}", x, layout, s, b)
        if key:
            p = zwebp.Pipeline(n, w, h, RGB, ctx=ctx)
            assert (p.lanes == 2) if key == "ZW_PIPE_LANES" else (p.launch_frames == 2), key
            p.close()
            del os.environ[key]

# ---- other options ----
u8 = frames_u8(2, 37, 21, 0x5EED5700, 3)
x, s, b = as_dtype(u8, "f32")
case("token_partitions=2", x, "chw", s, b, nparts=2)
assert expected(rule(x, s, b), nparts=2) != expected(rule(x, s, b))
for m in (2, 6):
    case(f"method {m}", x, "hwc", s, b, q=60, m=m)

# ---- Pipeline.set_input ----
n, w, h = 3, 37, 21
u8 = frames_u8(n, w, h, 0x5EED5800, 3)
x, s, b = as_dtype(u8, "f32")
img = rule(x, s, b)
want = expected(img)
host, buf, view = place(x, "chw", rp=3, guard=8)
p = zwebp.Pipeline(n, w, h, RGB, ctx=ctx)
p.set_input(view, "chw", s, b)
p.encode()
assert [p.output(i) for i in range(n)] == want
for i in range(n):
    py, pu, pv = p.planes(i, 0)
    ry, ru, rv = zwebp.rgb_to_yuv420(img[i], w, h, 3, ctx=ctx)
    assert np.array_equal(py, ry) and np.array_equal(pu, ru) and np.array_equal(pv, rv), i
    oy, ou, ov = O.rgb_to_yuv420(img[i], w, h, 3)
    assert np.array_equal(py, oy) and np.array_equal(pu, ou) and np.array_equal(pv, ov), i
p.encode_repeat(2)
assert [p.output(i) for i in range(n)] == want
p.run_pass1(False)
p.run_device()
try:
    p.encode_host([[img[i] for i in range(n)]])
    raise AssertionError("encode_host with a device input")
except zwebp.EncodingError as e:
    assert e.code == 3
other = frames_u8(n, w, h, 0x5EED5900, 3)
p.set_input(None)
for i in range(n):
    p.upload(i, other[i])
p.encode()
assert [p.output(i) for i in range(n)] == expected(other)
assert [p.output(i) for i in range(n)] == zwebp.encode_batch(list(other), w, h, RGB, ctx=ctx)
p.set_input(view, "chw", s, b)
p.encode()
assert [p.output(i) for i in range(n)] == want
p.close()
assert unchanged(host, buf)
for bad in (torch.zeros((n, 4, h, w), dtype=torch.uint8, device=dev),     # RGBA tensor, RGB pipe
            torch.zeros((n + 1, 3, h, w), dtype=torch.uint8, device=dev),
            torch.zeros((n, 3, h, w + 1), dtype=torch.uint8, device=dev)):
    p = zwebp.Pipeline(n, w, h, RGB, ctx=ctx)
    try:
        p.set_input(bad)
        raise AssertionError("set_input accepted " + str(tuple(bad.shape)))
    except (ValueError, zwebp.EncodingError) as e:
        assert isinstance(e, ValueError) or e.code == 3
    p.close()
print("case Pipeline.set_input ok", flush=True)

# ---- containers ----
host, buf, view = place(x, "hwc")
files = zwebp.encode_webp_batch_device(view, scale=s, bias=b, ctx=ctx)
assert files == zwebp.encode_webp_batch(list(img), w, h, RGB, ctx=ctx)
assert all(f[:4] == b"RIFF" and f[12:16] == b"VP8 " and f[20:20 + len(e)] == e for f, e in zip(files, want))
x4 = np.concatenate([x, x[..., :1]], axis=-1)
host4, buf4, view4 = place(x4, "hwc")
try:
    zwebp.encode_webp_batch_device(view4, scale=s, bias=b, ctx=ctx)
    raise AssertionError("container output from 4 channels")
except ValueError:
    pass
p = zwebp.Pipeline(n, w, h, zwebp.ColorType.Rgba8, ctx=ctx)
p.set_input(view4, "hwc", s, b)
try:
    p.set_container([np.zeros((h, w, 4), np.uint8)] * n)
    raise AssertionError("RGBA container with a device input")
except zwebp.EncodingError as e:
    assert e.code == 3
p.encode()       # (bare frames still work)
assert [p.output(i) for i in range(n)] == want
p.close()
print("case containers ok", flush=True)

# ---- rejections: refused before any launch ----
good = torch.zeros((2, 3, H, W), dtype=torch.uint8, device=dev)
for name, bad in (("host tensor", torch.zeros((2, 3, H, W), dtype=torch.uint8)),
                  ("int32", torch.zeros((2, 3, H, W), dtype=torch.int32, device=dev)),
                  ("transposed", torch.zeros((2, 3, W, H), dtype=torch.uint8, device=dev).transpose(2, 3)),
                  ("2 channels", torch.zeros((2, 2, H, W), dtype=torch.uint8, device=dev)),
                  ("column stride", torch.zeros((2, 3, H, 2 * W), dtype=torch.uint8, device=dev)[..., ::2]),
                  ("3-d", torch.zeros((3, H, W), dtype=torch.uint8, device=dev))):
    try:
        zwebp.encode_batch_device(bad, ctx=ctx)
    except ValueError:
        print("case ValueError", name, "ok", flush=True)
    else:
        raise AssertionError("tensor form accepted: " + name)
assert len(zwebp.encode_batch_device(good, ctx=ctx)) == 2

fs, rs = W * 3 * H, W * 3
cap = fs + (H - 1) * rs + W * 3
buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def refused(name, ptr=None, capacity=cap, n=2, ch=3, layout="hwc", dtype="u8", fs=fs, ps=None, rs=rs, up=0, w=W, h=H,
            code=3, nparts=1):
    try:
        zwebp.encode_batch_device_ptr(buf.data_ptr() if ptr is None else ptr, capacity, n, w, h, ch, layout, dtype,
                                      frame_stride=fs, plane_stride=ps, row_stride=rs, upsampling=up,
                                      token_partitions=nparts, ctx=ctx)
    except zwebp.EncodingError as e:
        assert e.code == code, (name, e.code)
    else:
        raise AssertionError(name + ": accepted")
    print("case refused", name, "ok", flush=True)


assert len(zwebp.encode_batch_device_ptr(buf.data_ptr(), cap, 2, W, H, 3, "hwc", "u8", ctx=ctx)) == 2
refused("capacity one short", capacity=cap - 1)
refused("frame stride below a frame", fs=(H - 1) * rs + W * 3 - 1)
refused("row stride short", rs=W * 3 - 1)
refused("chw plane stride short", layout="chw", ps=(H - 1) * W + W - 1, rs=W)
refused("upsampling 1", up=1)
refused("channels 2", ch=2)
refused("bad layout", layout=2)
refused("bad dtype", dtype=3)
refused("null data", ptr=0)
refused("misaligned f32", ptr=buf.data_ptr() + 2, dtype="f32", capacity=cap // 4 - 1, n=1, w=8, h=8, fs=192, rs=24)
refused("token partitions 3", nparts=3)
refused("zero width", w=0, code=1)
pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
refused("pinned host memory", ptr=pinned.data_ptr())
plain = np.zeros(cap, np.uint8)
refused("host memory", ptr=plain.ctypes.data)
assert bool((buf == 0xA5).all())
print("cases", ncase)
print("device encode ok")
"""


@pytest.mark.gpu
def test_gpu_encode_batch_device():
    """Every device-tensor encode case in one child process (torch's HIP runtime must
    initialise before the library's): sizes, every layout x dtype x channels, padded and
    misaligned tensors with NaN / 0xA5 in the gaps, the float rule's ties and specials,
    frame indexing across chunks and lanes, token partitions and methods,
    Pipeline.set_input, the container entry and the refusals."""
    r = subprocess.run([sys.executable, "-c", _CASES], env=ENV, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "device encode ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_encode_device_entry_points_bound():
    """The new entry points exist and are bound without importing torch."""
    code = ("import sys, zwebp; L = zwebp.load_library(); assert 'torch' not in sys.modules; "
            "assert L.zw_encode_batch_device and L.zw_pipe_set_input_device; print('bound')")
    r = subprocess.run([sys.executable, "-c", code], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bound" in r.stdout, r.stdout + r.stderr
    import zwebp
    assert callable(zwebp.encode_batch_device) and callable(zwebp.encode_batch_device_ptr)
    assert callable(zwebp.encode_webp_batch_device) and callable(zwebp.Pipeline.set_input)
    assert {"zw_encode_batch_device", "zw_pipe_set_input_device"} <= {n for n, _, _ in zwebp.SIGNATURES}
