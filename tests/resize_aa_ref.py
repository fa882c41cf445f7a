"""numpy / Python-integer restatement of the antialiased resampling rule of
zw_vp8_decode_batch_device_resized_ex (ZW_RESIZE_TRIANGLE_AA; include/zwebp.h
gives it in full, the product's own definition is csrc/zw_resize.h).  Shared by
test_dec_resize_aa_rule.py (the taps against zw_dbg_resize_aa_taps, the rule
against torch) and test_gpu_dec_resize_aa.py (the expected tensors).  Integers
throughout, Python / int64 arithmetic: nothing here rounds.

One axis: a window of s source pixels to d outputs, output index o, m = max(s,
d); positions in units of 1/(2d) pixel.  Source sample i sits at (2i + 1) d, the
output centre at c = (2o + 1) s; u_i = max(0, 2m - |(2i + 1) d - c|); the taps
are the i in [0, s - 1] with u_i > 0; with the running sum C_k and the total U,
W_k = floor((C_k * 4096 + floor(U / 2)) / U) and w_k = W_k - W_(k-1)."""
import numpy as np

ONE = 4096


def tap(src, dst, o):
    """(first, [w_k]) for one output index, in Python integers."""
    assert src >= 1 and dst >= 1 and 0 <= o < dst
    m = max(src, dst)
    c = (2 * o + 1) * src
    # u_i > 0  <=>  c - 2m < (2i + 1) d < c + 2m: a window around c / (2d) - 1/2
    lo = max((c - 2 * m - dst) // (2 * dst), 0)
    hi = min((c + 2 * m - dst) // (2 * dst) + 1, src - 1)
    u = [(i, 2 * m - abs((2 * i + 1) * dst - c)) for i in range(lo, hi + 1)]
    u = [(i, v) for i, v in u if v > 0]
    assert u and [i for i, _ in u] == list(range(u[0][0], u[-1][0] + 1))
    U = sum(v for _, v in u)
    w, C, prev = [], 0, 0
    for _, v in u:
        C += v
        W = (C * ONE + U // 2) // U
        w.append(W - prev)
        prev = W
    return u[0][0], w


def matrix(src, dst):
    """The axis as a [dst, src] int64 matrix of weights (rows sum to 4096)."""
    M = np.zeros((dst, src), np.int64)
    for o in range(dst):
        first, w = tap(src, dst, o)
        M[o, first:first + len(w)] = w
    return M


def weighted_sum(rgb, window, out_h, out_w):
    """S [out_h, out_w, C] int64 (the output value times 65536) from the full
    frame's u8 image `rgb` [H, W, C] and window = (x, y, w, h) in frame pixels:
    T = sum_y wy * sum_x wx * p, S = (T + 128) >> 8."""
    cx, cy, cw, ch = window
    H, W = rgb.shape[:2]
    assert cw >= 1 and ch >= 1 and cx + cw <= W and cy + ch <= H
    p = rgb[cy:cy + ch, cx:cx + cw].astype(np.int64)
    Mx, My = matrix(cw, out_w), matrix(ch, out_h)
    T = np.einsum("oy,yxc->oxc", My, np.einsum("px,yxc->ypc", Mx, p))
    assert T.max() <= 255 * ONE * ONE
    return (T + 128) >> 8


def resize(rgb, window, out_h, out_w, dtype="u8", scale=None, bias=None):
    """The output image [out_h, out_w, C] as the entry stores it: S through
    resize_ref.resize's storage formulae (u8 = (S + 32768) >> 16; f32 =
    float32(S) * 2^-16 times scale plus bias, each a rounded float32 operation;
    f16 = that rounded to nearest even)."""
    S = weighted_sum(rgb, window, out_h, out_w)
    if dtype == "u8":
        return ((S + 32768) >> 16).astype(np.uint8)
    v = S.astype(np.float32) * np.float32(2.0 ** -16)
    f = np.empty(v.shape, np.float32)
    for c in range(v.shape[2]):
        f[..., c] = v[..., c] * np.float32(1.0 if scale is None else scale[c]) + np.float32(0.0 if bias is None else bias[c])
    return f if dtype == "f32" else f.astype(np.float16)

