"""numpy restatement of the resampling rule of zw_vp8_decode_batch_device_resized
(include/zwebp.h; the product's own definition is csrc/zw_resize.h).  Shared by
test_dec_resize_rule.py (the taps against zw_dbg_resize_taps) and
test_gpu_dec_resize.py (the expected tensors).  Integers throughout, Python /
int64 arithmetic: nothing here rounds."""
import numpy as np


def taps(src, dst):
    """(i0, i1, f) int64 arrays of dst entries: one axis, a window of `src`
    pixels to `dst` outputs (half-pixel centres, 1/256 pixel positions)."""
    assert src >= 1 and dst >= 1
    o = np.arange(dst, dtype=np.int64)
    pos = (2 * o + 1) * (np.int64(src) * 128) // np.int64(dst) - 128
    pos = np.clip(pos, 0, (src - 1) * 256)
    i0 = pos >> 8
    return i0, np.minimum(i0 + 1, src - 1), pos & 255


def tap(src, dst, o):
    """The same for one output index, in Python integers."""
    pos = (2 * o + 1) * src * 128 // dst - 128
    pos = min(max(pos, 0), (src - 1) * 256)
    i0 = pos >> 8
    return i0, min(i0 + 1, src - 1), pos & 255


def weighted_sum(rgb, window, out_h, out_w):
    """S [out_h, out_w, C] int64 (the output value times 65536) from the full
    frame's u8 image `rgb` [H, W, C] and window = (x, y, w, h) in frame pixels."""
    cx, cy, cw, ch = window
    H, W = rgb.shape[:2]
    assert cw >= 1 and ch >= 1 and cx + cw <= W and cy + ch <= H
    p = rgb[cy:cy + ch, cx:cx + cw].astype(np.int64)
    x0, x1, fx = taps(cw, out_w)
    y0, y1, fy = taps(ch, out_h)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    top = (256 - fx) * p[y0][:, x0] + fx * p[y0][:, x1]
    bot = (256 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]
    return (256 - fy) * top + fy * bot


def resize(rgb, window, out_h, out_w, dtype="u8", scale=None, bias=None):
    """The output image [out_h, out_w, C] as the entry stores it: u8 = (S +
    32768) >> 16; f32 = float32(S) * 2^-16 (exact), times float32(scale[c]),
    plus float32(bias[c]), each a rounded float32 operation; f16 = that rounded
    to nearest even."""
    S = weighted_sum(rgb, window, out_h, out_w)
    assert S.max() <= 255 * 65536
    if dtype == "u8":
        return ((S + 32768) >> 16).astype(np.uint8)
    v = S.astype(np.float32) * np.float32(2.0 ** -16)
    f = np.empty(v.shape, np.float32)
    for c in range(v.shape[2]):
        f[..., c] = v[..., c] * np.float32(1.0 if scale is None else scale[c]) + np.float32(0.0 if bias is None else bias[c])
    return f if dtype == "f32" else f.astype(np.float16)
