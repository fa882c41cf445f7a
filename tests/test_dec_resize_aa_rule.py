"""The antialiased resampling rule of zw_vp8_decode_batch_device_resized_ex
(ZW_RESIZE_TRIANGLE_AA) on the CPU: the taps and weights the library computes
(zw_dbg_resize_aa_taps runs csrc/zw_resize.h's functions, the ones the weight kernel
runs per output index) against the restatement in resize_aa_ref.py, the rule's stated
properties, the hook's refusals, the Python surface, and the restatement against
torch's interpolate(mode="bilinear", antialias=True) in float64.  No device is touched."""
import ctypes
import inspect

import numpy as np
import pytest

import resize_aa_ref as A
import zwebp

BIG = (1, 224, 1080, 16383)


def check_output(src, dst, o, prev_first):
    first, w = zwebp.dbg_resize_aa_taps(src, dst, o)
    assert (first, w) == A.tap(src, dst, o), (src, dst, o)
    m = max(src, dst)
    assert sum(w) == 4096 and min(w) >= 0, (src, dst, o)
    assert first >= 0 and first + len(w) <= src and 1 <= len(w) <= -(-2 * m // dst), (src, dst, o)
    assert first >= prev_first, (src, dst, o)
    return first


def test_taps_match_restatement_small():
    """Every src, dst in 1..40, every output index: the hook equals the restatement, the
    weights sum to 4096, none is negative, the taps lie in the window, there are at most
    ceil(2m / d) of them, and `first` does not decrease with o."""
    for src in range(1, 41):
        for dst in range(1, 41):
            prev = 0
            for o in range(dst):
                prev = check_output(src, dst, o, prev)


def test_taps_match_restatement_large():
    """Pairs from {1, 224, 1080, 16383} at o = 0, 1, the middle and the last two (U
    reaches 2 s^2 / d = 5.4e8 at 16383 -> 1, times 4096 past 2^32)."""
    for src in BIG:
        for dst in BIG:
            prev = 0
            for o in sorted({0, min(1, dst - 1), dst // 2, max(dst - 2, 0), dst - 1}):
                prev = check_output(src, dst, o, prev)
    first, w = zwebp.dbg_resize_aa_taps(16383, 1, 0)
    assert first == 0 and len(w) == 16383


def test_axis_tap_total_bound():
    """Over a whole axis there are at most 2m + d taps."""
    for src, dst in ((161, 32), (97, 24), (161, 1), (9, 4), (3, 5), (1080, 224), (40, 39), (39, 40)):
        total = sum(len(zwebp.dbg_resize_aa_taps(src, dst, o)[1]) for o in range(dst))
        assert total <= 2 * max(src, dst) + dst, (src, dst, total)


def test_identity_weights():
    """s == d: one tap of weight 4096 at i = o."""
    for n in list(range(1, 41)) + list(BIG):
        for o in sorted({0, n // 2, n - 1}) if n > 40 else range(n):
            assert zwebp.dbg_resize_aa_taps(n, n, o) == (o, [4096]), (n, o)


def test_two_to_one_weights():
    """s == 2d: 512, 1536, 1536, 512 on 2o - 1 .. 2o + 2, renormalised at the window's ends."""
    for d in list(range(3, 41)) + [112, 540]:
        for o in range(1, d - 1):
            assert zwebp.dbg_resize_aa_taps(2 * d, d, o) == (2 * o - 1, [512, 1536, 1536, 512]), (d, o)
        # the ends drop the tap outside the window: 3, 3, 1 of 7
        U = 7 * d
        W0, W1 = (3 * d * 4096 + U // 2) // U, (6 * d * 4096 + U // 2) // U
        end = [W0, W1 - W0, 4096 - W1]
        assert zwebp.dbg_resize_aa_taps(2 * d, d, 0) == (0, end), d
        assert zwebp.dbg_resize_aa_taps(2 * d, d, d - 1)[0] == 2 * d - 3, d
        assert sorted(zwebp.dbg_resize_aa_taps(2 * d, d, d - 1)[1]) == sorted(end), d
    assert zwebp.dbg_resize_aa_taps(2, 1, 0) == (0, [2048, 2048])


def test_upscale_is_bilinear():
    """s < d: at most two taps, the 12-bit rounding of the bilinear fraction."""
    for src, dst in ((3, 7), (8, 16), (97, 130), (1, 5), (39, 40)):
        for o in range(dst):
            first, w = zwebp.dbg_resize_aa_taps(src, dst, o)
            assert len(w) <= 2, (src, dst, o)
            # centre in source pixels: (2o + 1) s / (2d) - 1/2; the second tap's share is its fraction
            num = (2 * o + 1) * src - dst  # position * 2d
            if num <= 0:
                assert (first, w) == (0, [4096])
            elif num >= (src - 1) * 2 * dst:
                assert (first, w) == (src - 1, [4096])
            else:
                i0, r = divmod(num, 2 * dst)
                W0 = ((2 * dst - r) * 4096 + dst) // (2 * dst)
                want = [W0, 4096 - W0] if r else [4096]
                assert (first, w) == (i0, want), (src, dst, o)


def test_identity_and_flat_values():
    """An identity resize returns the image (and a window of the output's size the crop);
    a flat image of value 0 or 255 comes back exactly, at any ratio, in every dtype."""
    rng = np.random.default_rng(0x5EED7A00)
    img = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
    assert np.array_equal(A.resize(img, (0, 0, 10, 12), 12, 10), img)
    assert np.array_equal(A.resize(img, (3, 5, 4, 6), 6, 4), img[5:11, 3:7])
    f = A.resize(img, (0, 0, 10, 12), 12, 10, "f32", (2.0, 0.5, 1.0), (1.0, 0.0, -3.0))
    assert np.array_equal(f[..., 0], img[..., 0].astype(np.float32) * 2 + 1)
    for v in (0, 255):
        flat = np.full((23, 31, 3), v, np.uint8)
        for oh, ow in ((1, 1), (5, 7), (23, 31), (22, 30), (40, 50), (11, 62)):
            assert np.all(A.weighted_sum(flat, (0, 0, 31, 23), oh, ow) == v * 65536), (v, oh, ow)
            assert np.all(A.resize(flat, (0, 0, 31, 23), oh, ow) == v), (v, oh, ow)
            assert np.all(A.resize(flat, (0, 0, 31, 23), oh, ow, "f32") == np.float32(v)), (v, oh, ow)


def test_crop_then_resize_is_resize_of_crop():
    rng = np.random.default_rng(0x5EED7A01)
    img = rng.integers(0, 256, (30, 41, 3), dtype=np.uint8)
    win = (5, 3, 29, 20)
    crop = np.ascontiguousarray(img[3:23, 5:34])
    assert np.array_equal(A.weighted_sum(img, win, 7, 9), A.weighted_sum(crop, (0, 0, 29, 20), 7, 9))


def test_hook_refuses_bad_arguments():
    L = zwebp.load_library()
    first, count = ctypes.c_int32(-7), ctypes.c_int32(-7)
    w = (ctypes.c_uint16 * 64)()
    f, c = ctypes.byref(first), ctypes.byref(count)
    assert L.zw_dbg_resize_aa_taps(0, 4, 0, f, c, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps((1 << 23) + 1, 4, 0, f, c, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps(4, 0, 0, f, c, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps(4, 4, 4, f, c, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps(4, 4, 0, None, c, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps(4, 4, 0, f, None, w, 64) == 3
    assert L.zw_dbg_resize_aa_taps(4, 4, 0, f, c, None, 64) == 3
    assert L.zw_dbg_resize_aa_taps(8, 2, 0, f, c, w, 5) == 3  # six taps (of 8 possible)
    assert L.zw_dbg_resize_aa_taps(8, 2, 0, f, c, w, 6) == 0 and (first.value, count.value) == (0, 6)
    assert L.zw_dbg_resize_aa_taps(1 << 23, 4, 3, f, c, w, 0) == 3
    assert zwebp.dbg_resize_aa_taps(4, 2, 1) == A.tap(4, 2, 1)


def test_python_surface():
    names = {n for n, _, _ in zwebp.SIGNATURES}
    assert "zw_vp8_decode_batch_device_resized_ex" in names and "zw_dbg_resize_aa_taps" in names
    assert "zw_vp8_decode_batch_device_resized" in names
    for name in ("decode_batch_device_resized", "decode_batch_device_resized_ptr", "decode_webp_batch_device_resized"):
        p = inspect.signature(getattr(zwebp, name)).parameters
        assert "antialias" in p and p["antialias"].default is False, name
    assert callable(zwebp.dbg_resize_aa_taps)
    L = zwebp.load_library()
    assert L.zw_vp8_decode_batch_device_resized_ex and L.zw_dbg_resize_aa_taps


# ---- the rule against torch (CPU, float64): a sanity bound that catches a wrong filter ----
TORCH_SHAPES = (((161, 97), (32, 24)), ((161, 97), (7, 5)), ((161, 97), (160, 96)), ((161, 97), (200, 130)),
                ((480, 270), (56, 56)), ((17, 9), (1, 1)), ((400, 300), (399, 7)))


def _pattern(kind, w, h):
    if kind == "noise":
        return np.random.default_rng(0x5EED7B00 + w * 7 + h).integers(0, 256, (h, w, 1), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(127.5 + 80 * np.sin(x / 9.0) + 47 * np.cos(y / 5.0 + x / 31.0), 0, 255).astype(np.uint8)[..., None]


@pytest.mark.parametrize("kind", ("noise", "smooth"))
def test_restatement_agrees_with_torch(kind):
    """|S / 65536 - interpolate(antialias=True)| <= 0.5 of a level (the rule alone measured
    0.22 at worst, 400x300 -> 399x7 on noise); the u8 outputs differ by at most 1."""
    import torch
    worst = 0.0
    for (w, h), (ow, oh) in TORCH_SHAPES:
        img = _pattern(kind, w, h)
        S = A.weighted_sum(img, (0, 0, w, h), oh, ow)[..., 0]
        t = torch.from_numpy(img[..., 0].astype(np.float64))[None, None]
        ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bilinear", antialias=True,
                                              align_corners=False)[0, 0].numpy()
        err = float(np.abs(S / 65536.0 - ref).max())
        print(f"{kind} {w}x{h} -> {ow}x{oh}: max |S / 65536 - torch| = {err:.4f}")
        worst = max(worst, err)
        assert err <= 0.5, (kind, w, h, ow, oh, err)
        u8 = A.resize(img, (0, 0, w, h), oh, ow)[..., 0].astype(np.int64)
        assert np.abs(u8 - np.clip(np.floor(ref + 0.5), 0, 255).astype(np.int64)).max() <= 1
    print("worst", worst)
