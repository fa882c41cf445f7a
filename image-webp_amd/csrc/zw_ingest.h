// zw_ingest.h -- device-tensor input of the encoder (zw_pipe_set_input_device,
// zw_encode_batch_device): the pixel rule, the argument check and the
// "every run is vectorisable" predicate.
//
// Plain C types only (no HIP types): k_rgb2yuv_dev in zw_ingest_kernels.hip
// reads it on the device, zw_host.cpp on the host, and tools/ingest_check.cpp
// walks all three parts on the CPU, where nothing can go out of range.
//
// PIXEL RULE.  Input element x of channel c gives the byte v the encoder sees:
//   u8    v = x (scale and bias are ignored);
//   f32   t = x * scale[c]   a rounded multiply,
//         t = t + bias[c]    a rounded add (the two are never fused),
//         v = 0 if t is NaN, else (uint8) rint(min(max(t, 0), 255)),
//         round-half-to-even; +-inf therefore clamps;
//   f16   x converted to f32 (exact), then the f32 rule.
// With 4 channels, channel 3 is never used (CHW: its plane is never read).
// Build host users with -ffp-contract=off; the device spells the two operations
// as __fmul_rn / __fadd_rn, which the compiler never contracts.
//
// ADDRESSING (zw_device_images, in elements from `data`):
//   HWC  i*frame_stride + y*row_stride + x*channels + c,  row_stride >= w*channels;
//   CHW  i*frame_stride + c*plane_stride + y*row_stride + x,
//        row_stride >= w, plane_stride >= (h-1)*row_stride + w.
//
// RUNS.  One thread owns 8x2 luma pixels: an 8-pixel run of two rows.  The
// vector form loads exactly the run's own elements, in pieces of
// ing_piece_bytes: per row 8*channels elements (HWC; channel 3 is loaded with
// its pixel and dropped) or 8 elements of each of the three planes (CHW).  A
// run is loaded that way only if it lies inside the row (x0 + 8 <= w) and the
// row inside the image; so no load leaves the row's own elements, hence none
// leaves [0, capacity).  Every piece is aligned iff the base address and every
// stride, in bytes, are multiples of the piece (a run starts 8*g pixels into
// its row: a multiple of the piece in every form): ing_vec_ok.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef ZW_HD
#ifdef __HIPCC__
#define ZW_HD __host__ __device__
#else
#define ZW_HD
#endif
#endif

// the values of ZW_LAYOUT_* / ZW_DTYPE_* (include/zwebp.h)
enum { ZW_ING_HWC = 0, ZW_ING_CHW = 1 };
enum { ZW_ING_U8 = 0, ZW_ING_F16 = 1, ZW_ING_F32 = 2 };

ZW_HD constexpr int ing_elsize(int dtype) { return dtype == ZW_ING_U8 ? 1 : (dtype == ZW_ING_F16 ? 2 : 4); }

// ---- pixel rule ----
ZW_HD inline uint8_t ing_byte_f32(float x, float scale, float bias)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fadd_rn(__fmul_rn(x, scale), bias);
    if (t != t) return 0;
    return (uint8_t)(int)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(t, 0.0f), 255.0f));
#else
    volatile float m = x * scale;  // (rounded to f32 before the add, whatever the build's contraction setting)
    const float t = m + bias;
    if (t != t) return 0;
    const float c = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (uint8_t)(int)__builtin_rintf(c);  // (the default rounding mode: to nearest, ties to even)
#endif
}

// binary16 bits -> f32, exact
ZW_HD inline float ing_f16_bits_to_f32(uint16_t hb)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, hb);
#else
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16;
    uint32_t e = (hb >> 10) & 31u, m = hb & 1023u, bits;
    if (e == 31u) {
        bits = sign | 0x7f800000u | (m << 13);  // inf / NaN
    } else if (e) {
        bits = sign | ((e + 112u) << 23) | (m << 13);
    } else if (m) {  // subnormal: m * 2^-24
        int sh = 0;
        while (!(m & 1024u)) {
            m <<= 1;
            sh++;
        }
        bits = sign | ((uint32_t)(113 - sh) << 23) | ((m & 1023u) << 13);
    } else {
        bits = sign;
    }
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
#endif
}

ZW_HD inline uint8_t ing_byte_f16(uint16_t hb, float scale, float bias)
{
    return ing_byte_f32(ing_f16_bits_to_f32(hb), scale, bias);
}

// ---- argument check ----
// a + b * c in size_t; false on overflow
inline bool ing_madd(size_t a, size_t b, size_t c, size_t* out)
{
    size_t t;
    return !__builtin_mul_overflow(b, c, &t) && !__builtin_add_overflow(a, t, out);
}

// The strides' bounds, frames that do not overlap, and the elements the batch
// needs at `data`: *need = the last addressed element + 1.  False: a stride
// below its bound, overlapping frames or an overflow.
inline bool ing_span(int layout, size_t n, size_t w, size_t h, size_t ch, size_t frame_stride, size_t plane_stride,
                     size_t row_stride, size_t* need)
{
    if (n == 0 || w == 0 || h == 0 || ch == 0) return false;
    size_t span = 0;  // the elements one frame spans
    if (layout == ZW_ING_CHW) {
        size_t plane = 0;
        if (row_stride < w || !ing_madd(w, h - 1, row_stride, &plane) || plane_stride < plane ||
            !ing_madd(plane, ch - 1, plane_stride, &span))
            return false;
    } else if (layout == ZW_ING_HWC) {
        size_t row = 0;
        if (!ing_madd(0, w, ch, &row) || row_stride < row || !ing_madd(row, h - 1, row_stride, &span)) return false;
    } else {
        return false;
    }
    if (n > 1 && frame_stride < span) return false;
    return ing_madd(span, n - 1, frame_stride, need);
}

// ---- vector form ----
// Bytes of one vector load: CHW u8 8 (a run of one plane), CHW f16 16, CHW f32
// 16 (two a run); HWC: the run's 8*channels elements in 16-byte pieces, 8-byte
// ones for u8 x 3 (24 bytes a run).
ZW_HD constexpr int ing_piece_bytes(int layout, int dtype, int ch)
{
    return layout == ZW_ING_CHW ? (dtype == ZW_ING_U8 ? 8 : 16) : (dtype == ZW_ING_U8 && ch == 3 ? 8 : 16);
}
// vector loads one row of a run takes from one plane (CHW) / from the row (HWC)
ZW_HD inline int ing_pieces(int layout, int dtype, int ch)
{
    const int elems = layout == ZW_ING_CHW ? 8 : 8 * ch;
    return elems * ing_elsize(dtype) / ing_piece_bytes(layout, dtype, ch);
}
// Run g of a row: its first element from the row's start (of each plane, CHW).
ZW_HD inline size_t ing_run_first(int layout, int ch, size_t g) { return layout == ZW_ING_CHW ? 8 * g : 8 * g * (size_t)ch; }
// A run takes the vector loads only inside the row; a row only inside the image.
ZW_HD inline bool ing_run_in_row(int x0, int w) { return x0 + 8 <= w; }

// Every piece of every run aligned: the base address and every stride the
// kernel adds, in bytes, are multiples of the piece.  plane_stride counts for CHW only.
inline bool ing_vec_ok(int layout, int dtype, int ch, uintptr_t base, size_t frame_stride, size_t plane_stride,
                       size_t row_stride)
{
    const size_t piece = (size_t)ing_piece_bytes(layout, dtype, ch), es = (size_t)ing_elsize(dtype);
    if (base % piece) return false;
    if (frame_stride % piece * es % piece || row_stride % piece * es % piece) return false;
    return layout != ZW_ING_CHW || plane_stride % piece * es % piece == 0;
}
