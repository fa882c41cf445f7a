// zw_resize.h -- the resampling rule of zw_vp8_decode_batch_device_resized, one
// definition for the host (validation, zw_dbg_resize_taps), the device
// (k_yuv2rgb_resize) and, restated in numpy, the tests (include/zwebp.h gives
// the rule in full).  Bilinear, half-pixel centres, no antialiasing; integers
// only, so every user computes the same bits.
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
