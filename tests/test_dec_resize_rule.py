"""The resampling rule of zw_vp8_decode_batch_device_resized on the CPU: the taps the
library computes (zw_dbg_resize_taps runs csrc/zw_resize.h's function, the one
k_yuv2rgb_resize runs per output pixel) against the numpy restatement in
resize_ref.py, the rule's identity and 2:1 properties, and the Python surface
(names, signatures, vp8_frame_dims).  No device is touched."""
import ctypes
import os

import numpy as np

import resize_ref as R
import zwebp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = (1, 224, 1080, 16383)


def lib_taps(src, dst):
    """(i0, i1, f) arrays of dst entries from the library, one call per output index."""
    L = zwebp.load_library()
    out = (ctypes.c_int32 * 3)()
    got = np.empty((dst, 3), np.int64)
    for o in range(dst):
        assert L.zw_dbg_resize_taps(src, dst, o, out) == 0
        got[o] = out[0], out[1], out[2]
    return got[:, 0], got[:, 1], got[:, 2]


def check_pair(src, dst):
    i0, i1, f = lib_taps(src, dst)
    r0, r1, rf = R.taps(src, dst)
    assert np.array_equal(i0, r0) and np.array_equal(i1, r1) and np.array_equal(f, rf), (src, dst)
    # inside the window, monotone, a fraction of 256
    assert i0.min() >= 0 and i1.max() <= src - 1 and np.all(i1 >= i0) and np.all(i1 - i0 <= 1), (src, dst)
    assert np.all(np.diff(i0) >= 0) and np.all(np.diff(i1) >= 0), (src, dst)
    assert f.min() >= 0 and f.max() <= 255, (src, dst)


def test_taps_match_restatement_small():
    """Every src, dst in 1..40, every output index."""
    for src in range(1, 41):
        for dst in range(1, 41):
            check_pair(src, dst)


def test_taps_match_restatement_large():
    """Pairs from {1, 224, 1080, 16383}: the numerator passes 2^32 (6.9e10 at 16383)."""
    for src in BIG:
        for dst in BIG:
            check_pair(src, dst)
    assert (2 * 16382 + 1) * 16383 * 128 > 2 ** 32


def test_taps_beyond_32_bits():
    """The tap division runs in 32 bits where (2o + 1) * src and the remainder * 128 fit,
    else in 64: sampled output indices on both sides of each bound, against Python integers."""
    for src, dst in ((16383, (1 << 25) + 1), (16383, 1 << 25), (1 << 20, 4099), (1 << 23, (1 << 32) - 1), (3, 1 << 31),
                     (65535, 65536), (65537, 65535)):
        edge = min(dst - 1, (1 << 32) // (2 * src))  # (2o + 1) * src passes 2^32 about here
        for o in {0, 1, dst // 3, dst // 2, dst - 2, dst - 1, max(edge - 1, 0), edge, min(edge + 1, dst - 1)}:
            assert zwebp.dbg_resize_taps(src, dst, o) == R.tap(src, dst, o), (src, dst, o)


def test_restatement_scalar_and_array_agree():
    for src, dst in ((7, 3), (3, 7), (16383, 224), (224, 16383)):
        i0, i1, f = R.taps(src, dst)
        for o in (0, dst // 2, dst - 1):
            assert R.tap(src, dst, o) == (i0[o], i1[o], f[o])


def test_identity_and_two_to_one():
    """src == dst: f = 0 and i0 = o (a window of the output's size reproduces
    decode_batch_device's bytes); src == 2 * dst: i0 = 2 o, f = 128 (pixel pairs averaged)."""
    for n in list(range(1, 41)) + list(BIG):
        i0, i1, f = lib_taps(n, n)
        assert np.array_equal(i0, np.arange(n)) and not f.any(), n
    for n in list(range(1, 41)) + [112, 540]:
        i0, i1, f = lib_taps(2 * n, n)
        assert np.array_equal(i0, 2 * np.arange(n)) and np.array_equal(i1, i0 + 1) and np.all(f == 128), n


def test_identity_and_two_to_one_values():
    """The same through the value rule: an identity resize returns the image; 2:1
    rounds the mean of each 2 x 2 block half up."""
    rng = np.random.default_rng(0x5EED7000)
    img = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(img, (0, 0, 10, 12), 12, 10), img)
    assert np.array_equal(R.resize(img, (3, 5, 4, 6), 6, 4), img[5:11, 3:7])
    half = R.resize(img, (0, 0, 10, 12), 6, 5)
    blocks = img.astype(np.int64).reshape(6, 2, 5, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(half, ((blocks * 16384 + 32768) >> 16).astype(np.uint8))
    f = R.resize(img, (0, 0, 10, 12), 12, 10, "f32", (2.0, 0.5, 1.0), (1.0, 0.0, -3.0))
    assert np.array_equal(f[..., 0], img[..., 0].astype(np.float32) * 2 + 1)


def test_hook_refuses_bad_arguments():
    L = zwebp.load_library()
    out = (ctypes.c_int32 * 3)()
    assert L.zw_dbg_resize_taps(0, 4, 0, out) == 3
    assert L.zw_dbg_resize_taps(4, 0, 0, out) == 3
    assert L.zw_dbg_resize_taps(4, 4, 4, out) == 3
    assert L.zw_dbg_resize_taps(4, 4, 0, None) == 3
    assert zwebp.dbg_resize_taps(4, 2, 1) == R.tap(4, 2, 1)


def test_python_surface():
    names = {n for n, _, _ in zwebp.SIGNATURES}
    assert "zw_vp8_decode_batch_device_resized" in names and "zw_dbg_resize_taps" in names
    for name in ("decode_batch_device_resized", "decode_batch_device_resized_ptr", "decode_webp_batch_device_resized",
                 "vp8_frame_dims"):
        assert name in zwebp.__all__ and callable(getattr(zwebp, name)), name
    assert ctypes.sizeof(zwebp._Rect) == 16


def test_vp8_frame_dims():
    g = open(os.path.join(GOLD, "gallery1_1.vp8"), "rb").read()
    assert zwebp.vp8_frame_dims(g) == (550, 368)
    r = open(os.path.join(GOLD, "random_lossy_1.vp8"), "rb").read()
    assert zwebp.vp8_frame_dims(r) == (99, 87)
    assert zwebp.vp8_frame_dims(np.frombuffer(r, np.uint8)) == (99, 87)
    assert zwebp.vp8_frame_dims(b"\x00\x01\x02\x03\x04") == (0, 0)
    assert zwebp.vp8_frame_dims(b"") == (0, 0)
    assert zwebp.vp8_frame_dims(g[:9]) == (0, 0) and zwebp.vp8_frame_dims(g[:10]) == (550, 368)
