// zw_resize.h -- the resampling rules of zw_vp8_decode_batch_device_resized[_ex],
// one definition each for the host (validation, zw_dbg_resize_taps,
// zw_dbg_resize_aa_taps), the device (k_yuv2rgb_resize; k_resize_aa_weights and
// k_yuv2rgb_resize_aa) and, restated in numpy, the tests (include/zwebp.h gives
// the rules in full).  First the two-tap rule: bilinear, half-pixel centres, no
// antialiasing; then the antialiased triangle rule.  Integers only, so every
// user computes the same bits.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZW_RSZ_HD __host__ __device__ __forceinline__
#else
#define ZW_RSZ_HD inline
#endif

// One axis: output index o of dst (>= 1) over a source window of src (>= 1)
// pixels reads the window's pixels i0 and i1 = min(i0 + 1, src - 1) with the
// weights 256 - f and f.  The position is in 1/256 pixel units; its numerator
// reaches 6.9e10 at 16383, hence 64 bits; it must stay below 2^63 (any o and
// dst up to 2^32 with src up to 2^23; a frame has at most 16383).
struct ZwTap {
    int32_t i0, i1, f;
};
ZW_RSZ_HD ZwTap zw_resize_tap(uint32_t src, uint32_t dst, uint32_t o)
{
    // q = floor((2o + 1) * src * 128 / dst).  With a = (2o + 1) * src = qa * dst + ra
    // it is qa * 128 + floor(ra * 128 / dst): two 32-bit divisions where a and
    // ra * 128 fit 32 bits (every size a VP8 frame can have), else one in 64 bits.
    const uint64_t a = (2 * (uint64_t)o + 1) * src;
    uint64_t q;
    if (a <= 0xffffffffu && dst <= (1u << 25)) {
        const uint32_t a32 = (uint32_t)a, qa = a32 / dst, ra = a32 - qa * dst;
        q = (uint64_t)qa * 128 + ra * 128u / dst;
    } else {
        q = a * 128 / dst;
    }
    int64_t pos = (int64_t)q - 128;
    const int64_t last = ((int64_t)src - 1) * 256;
    pos = pos < 0 ? 0 : (pos > last ? last : pos);
    ZwTap t;
    t.i0 = (int32_t)(pos >> 8);
    t.f = (int32_t)(pos & 255);
    t.i1 = t.i0 + 1 < (int32_t)src ? t.i0 + 1 : (int32_t)src - 1;
    return t;
}

// The weighted sum S of one channel's four source bytes (rows y0 / y1, columns
// x0 / x1), scaled by 65536: at most 255 * 65536 < 2^24, exact in a float.
ZW_RSZ_HD uint32_t zw_resize_sum(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx, uint32_t fy)
{
    return (256u - fy) * ((256u - fx) * p00 + fx * p01) + fy * ((256u - fx) * p10 + fx * p11);
}

// S as a u8 element: rounded to nearest, halves up.
ZW_RSZ_HD uint32_t zw_resize_u8(uint32_t S) { return (S + 32768u) >> 16; }
// S as the float the float dtypes scale and bias: both steps are exact.
ZW_RSZ_HD float zw_resize_f32(uint32_t S) { return (float)S * (1.0f / 65536.0f); }

// ---------------------------------------------------------------------------
// The antialiased rule (ZW_RESIZE_TRIANGLE_AA; include/zwebp.h gives it in
// full): a triangle filter whose support widens with the downscale factor,
// taps outside the window dropped and the rest renormalised to 12 bits.  One
// axis, a window of src pixels to dst outputs, output index o, m = max(src,
// dst); positions in 1/(2 dst) pixel, so everything is an integer.  Source
// sample i sits at (2i + 1) dst, the output centre at c = (2o + 1) src, and
// u_i = max(0, 2m - |(2i + 1) dst - c|).  The host hook (zw_dbg_resize_aa_taps)
// and the weight kernel (k_resize_aa_weights) both run the functions below.
// src <= 2^23 and dst <= 2^32 keep every product below 2^63.
// ---------------------------------------------------------------------------
#define ZW_AA_ONE 4096u  // the weights of one output index sum to this

// The unnormalised weight of window pixel i (may be <= 0 outside the support).
ZW_RSZ_HD int64_t zw_resize_aa_u(uint32_t src, uint32_t dst, uint32_t o, int64_t i)
{
    const int64_t m = src > dst ? src : dst;
    const int64_t t = (2 * i + 1) * (int64_t)dst - (2 * (int64_t)o + 1) * (int64_t)src;
    return 2 * m - (t < 0 ? -t : t);
}

// The taps of output index o: the contiguous run first .. first + count - 1 of
// the i in [0, src - 1] with u_i > 0 (never empty, at most ceil(2m / dst)
// indices), and total = their sum U.
struct ZwAaSpan {
    int32_t first, count;
    uint64_t total;
};
ZW_RSZ_HD ZwAaSpan zw_resize_aa_span(uint32_t src, uint32_t dst, uint32_t o)
{
    const int64_t m = src > dst ? src : dst, d2 = 2 * (int64_t)dst, c = (2 * (int64_t)o + 1) * (int64_t)src;
    // u_i > 0  <=>  c - 2m < (2i + 1) dst < c + 2m
    const int64_t lo = c - 2 * m - dst, hi = c + 2 * m - dst;  // lo < 2 dst i < hi; hi > 0
    int64_t a = lo >= 0 ? lo / d2 + 1 : 0;
    int64_t b = (hi + d2 - 1) / d2 - 1;
    if (b > (int64_t)src - 1) b = (int64_t)src - 1;
    ZwAaSpan s;
    s.first = (int32_t)a;
    s.count = (int32_t)(b - a + 1);
    uint64_t U = 0;
    for (int64_t i = a; i <= b; i++) U += (uint64_t)zw_resize_aa_u(src, dst, o, i);
    s.total = U;
    return s;
}

// The normalised weights w_0 .. w_(count-1) by cumulative rounding: W_k =
// floor((C_k * 4096 + floor(U / 2)) / U) over the running sum C_k, w_k = W_k -
// W_(k-1); they sum to exactly 4096 and none is negative.  put(k, w_k) is
// called for k = 0 .. count - 1 in order.  (U reaches 2 src^2 / dst: 64 bits.)
template <class Put>
ZW_RSZ_HD void zw_resize_aa_weights(uint32_t src, uint32_t dst, uint32_t o, const ZwAaSpan& s, Put&& put)
{
    uint64_t C = 0;
    uint32_t prev = 0;
    for (int32_t k = 0; k < s.count; k++) {
        C += (uint64_t)zw_resize_aa_u(src, dst, o, (int64_t)s.first + k);
        const uint32_t W = (uint32_t)((C * ZW_AA_ONE + s.total / 2) / s.total);
        put(k, W - prev);
        prev = W;
    }
}

// T = sum_y wy * sum_x wx * p (at most 255 * 2^24; any summation order is exact
// in u32) as the S the storage steps above take: S = (T + 128) >> 8.
ZW_RSZ_HD uint32_t zw_resize_aa_S(uint32_t T) { return (T + 128u) >> 8; }
