// zw_alpha_kernels.hip -- the alpha plane of a lossy file with an ALPH chunk,
// on the device (gfx950): undoing the ALPH filter and writing channel 3 of the
// caller's tensor.
//
// The host reads each frame's ALPH payload (zw_vp8l_dec.cpp) into a plane of
// w * h residual bytes; a chunk's planes lie `pstride` bytes apart (16-byte
// aligned, at least 16 bytes of slack after each, so an aligned word that
// holds a plane byte is always inside the allocation).  The filter is undone
// in place by get_alpha_predictor (decoder/extended.rs:151-211):
//     out(y, x) = predictor(y, x) + residual(y, x)   (mod 256)
//   horizontal  predictor = out(y, x-1); column 0: out(y-1, 0); (0, 0): 0.
//               k_alpha_col0 makes column 0 a running sum down the column, then
//               k_alpha_rows makes every row a running sum from its column 0.
//   vertical    predictor = out(y-1, x); row 0: out(0, x-1); (0, 0): 0.
//               k_alpha_rows over row 0 alone, then k_alpha_cols sums every
//               column downwards.
//   gradient    predictor = clamp(L + T - TL, 0, 255); row 0: L; column 0: T.
//               The clamp does not associate: k_alpha_gradient is a true
//               anti-diagonal wavefront, one wave per frame.
// The running sums are scans mod 256: a wave's scan plus a carry.  No kernel
// here waits for another wave or workgroup (the only barriers are those of the
// gradient kernel's single-wave workgroup around its LDS tile), so none can
// hang; a frame's filter kernels follow each other in stream order.  Each
// launch covers the frames of `list` (the chunk's frames that use the filter).
//
// k_alpha_store then writes the planes into channel 3 of the caller's tensor
// by k_yuv2rgb_dev's store rule (zw_dec_kernels.hip): u8 the byte; f32
// a * scale[3] + bias[3] as a rounded multiply and a rounded add; f16 that
// float rounded to nearest even; HWC or CHW with the caller's strides; the
// gaps are never written; frames without alpha keep the 255 k_yuv2rgb_dev wrote.
//
// Bounds: every kernel derives its addresses from w, h and pstride alone; a
// lane outside the plane neither loads nor stores, and word accesses are made
// only at aligned addresses below w * h rounded up to 4.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "zw_common.h"

namespace {

// inclusive scan of v over the wave's 64 lanes (mod 2^32; the callers keep 8 bits)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// four byte adds mod 256 in one word
__device__ __forceinline__ uint32_t add_bytes(uint32_t a, uint32_t b)
{
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}

}  // namespace

// Column 0 of each listed frame becomes its running sum down the column.  One
// wave per frame: 64 rows per step, a wave scan and a carry.
extern "C" __global__ __launch_bounds__(64) void k_alpha_col0(uint8_t* __restrict__ planes, size_t pstride, int w, int h,
                                                              const uint32_t* __restrict__ list)
{
    uint8_t* p = planes + (size_t)list[blockIdx.x] * pstride;
    const int lane = (int)threadIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < h; base += 64) {
        const int y = base + lane;
        uint32_t v = y < h ? p[(size_t)y * w] : 0u;
        v = wave_scan_add(v, lane) + carry;
        if (y < h) p[(size_t)y * w] = (uint8_t)v;
        carry = (uint32_t)__shfl((int)v, 63, 64) & 255u;
    }
}

// Rows [0, rows) of each listed frame become their running sums along x.  One
// wave per row; a lane takes one aligned word (4 bytes) per step of 256 bytes;
// the bytes of a word outside the row count as 0 and are not written (a word
// that straddles two rows is written byte by byte: its other bytes belong to
// another wave).
extern "C" __global__ __launch_bounds__(256) void k_alpha_rows(uint8_t* __restrict__ planes, size_t pstride, int w,
                                                               int rows, const uint32_t* __restrict__ list)
{
    const int lane = (int)threadIdx.x & 63;
    const int y = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (y >= rows) return;  // (the whole wave)
    uint8_t* p = planes + (size_t)list[blockIdx.y] * pstride;
    const size_t o = (size_t)y * w, end = o + (size_t)w;
    uint32_t carry = 0;
    for (size_t base = o & ~(size_t)3; base < end; base += 256) {
        const size_t wa = base + 4 * (size_t)lane;
        const bool live = wa < end;
        const uint32_t word = live ? *(const uint32_t*)(p + wa) : 0u;
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = (wa + k >= o && wa + k < end) ? (word >> (8 * k)) & 255u : 0u;
        b[1] += b[0];
        b[2] += b[1];
        b[3] += b[2];
        const uint32_t incl = wave_scan_add(b[3], lane);
        const uint32_t add = incl - b[3] + carry;
        carry = ((uint32_t)__shfl((int)incl, 63, 64) + carry) & 255u;
        if (live) {
            if (wa >= o && wa + 4 <= end) {
                *(uint32_t*)(p + wa) = ((b[0] + add) & 255u) | (((b[1] + add) & 255u) << 8) |
                                       (((b[2] + add) & 255u) << 16) | (((b[3] + add) & 255u) << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (wa + k >= o && wa + k < end) p[wa + k] = (uint8_t)(b[k] + add);
            }
        }
    }
}

// Every column of each listed frame becomes its running sum downwards (row 0
// is final already).  WORD (w % 4 == 0: every row starts on a word): a lane
// takes four adjacent columns as one word and adds bytes in the word; else a
// lane takes one column.  Four rows are loaded before the first is summed.
template <bool WORD>
__device__ __forceinline__ void alpha_cols_body(uint8_t* __restrict__ planes, size_t pstride, int w, int h,
                                                const uint32_t* __restrict__ list)
{
    typedef typename std::conditional<WORD, uint32_t, uint8_t>::type T;
    const size_t ncol = WORD ? (size_t)w / 4 : (size_t)w;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncol) return;
    T* q = (T*)(planes + (size_t)list[blockIdx.y] * pstride) + c;
    uint32_t acc = q[0];
    for (int y = 1; y < h; y += 4) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = y + k < h ? (uint32_t)q[(size_t)(y + k) * ncol] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (y + k < h) {
                acc = WORD ? add_bytes(acc, v[k]) : (acc + v[k]) & 255u;
                q[(size_t)(y + k) * ncol] = (T)acc;
            }
    }
}
extern "C" __global__ __launch_bounds__(256) void k_alpha_cols_word(uint8_t* __restrict__ planes, size_t pstride, int w,
                                                                    int h, const uint32_t* __restrict__ list)
{
    alpha_cols_body<true>(planes, pstride, w, h, list);
}
extern "C" __global__ __launch_bounds__(256) void k_alpha_cols_byte(uint8_t* __restrict__ planes, size_t pstride, int w,
                                                                    int h, const uint32_t* __restrict__ list)
{
    alpha_cols_body<false>(planes, pstride, w, h, list);
}

// The gradient filter.  One wave per listed frame walks the frame's bands of
// 64 rows in order; lane j owns row 64 b + j of band b.  A band is worked in
// tiles of up to ZW_AG_TW columns staged in LDS: the wave loads the tile's
// rows (and the row above the band) with aligned word loads, runs the
// wavefront over the tile out of LDS, and stores the rows back in aligned
// words (the partial words at a tile's ends byte by byte).  In the wavefront
// lane j works column t - j at step t: T is the value the lane above made one
// step earlier (a one-lane shift), TL the T of the step before, L the lane's
// own last value; all three carry over from tile to tile.  Lane 0 takes T from
// the row above the band (LDS row 0).  The next step's residual is read from
// LDS while this step computes.
//
// An LDS row keeps the byte phase of its global segment: byte x of the tile's
// row r is at r * ZW_AG_LROW + ((row start + c0) & 3) + (x - c0), so aligned
// global words map to aligned LDS words.
#define ZW_AG_TW 512
#define ZW_AG_LROW (ZW_AG_TW + 8)
extern "C" __global__ __launch_bounds__(64) void k_alpha_gradient(uint8_t* __restrict__ planes, size_t pstride, int w,
                                                                  int h, const uint32_t* __restrict__ list)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[65 * ZW_AG_LROW];
    uint32_t* ldsw = (uint32_t*)lds;
    uint8_t* p = planes + (size_t)list[blockIdx.x] * pstride;
    const int lane = (int)threadIdx.x;
    for (int y0 = 0; y0 < h; y0 += 64) {
        const int nl = min(64, h - y0);  // the band's rows
        const int y = y0 + lane;
        const size_t o = (size_t)y * w;  // (used by the lanes below nl only)
        uint32_t cur = 0, tl = 0;        // L and TL; the tiles of a band hand them on
        for (int c0 = 0; c0 < w; c0 += ZW_AG_TW) {
            const int tw = min(ZW_AG_TW, w - c0);
            // the tile in: LDS row r + 1 = band row r, LDS row 0 = the row above the band
            for (int r = (y0 > 0 ? -1 : 0); r < nl; r++) {
                const size_t g0 = (size_t)(y0 + r) * w + (size_t)c0, sa = g0 & ~(size_t)3;
                const int nw = (int)((g0 - sa) + (size_t)tw + 3) / 4;  // <= ZW_AG_LROW / 4
                for (int i = lane; i < nw; i += 64) ldsw[(r + 1) * (ZW_AG_LROW / 4) + i] = *(const uint32_t*)(p + sa + 4 * (size_t)i);
            }
            __syncthreads();
            const int ph = (int)((o + (size_t)c0) & 3);
            const int pha = y0 > 0 ? (int)(((size_t)(y0 - 1) * w + (size_t)c0) & 3) : 0;
            uint8_t* mine = lds + (lane + 1) * ZW_AG_LROW + ph;
            const uint8_t* above = lds + pha;
            const int steps = tw + nl - 1;
            // the residual (and lane 0's T) of step t, read a step ahead
            auto fetch = [&](int t, uint32_t* res, uint32_t* top) {
                const int xl = t - lane;
                const bool on = lane < nl && xl >= 0 && xl < tw;
                *res = on ? mine[xl] : 0u;
                *top = (on && lane == 0 && y0 > 0) ? above[xl] : 0u;
            };
            uint32_t rn, an;
            fetch(0, &rn, &an);
            for (int t = 0; t < steps; t++) {
                const uint32_t res = rn, top0 = an;
                if (t + 1 < steps) fetch(t + 1, &rn, &an);
                uint32_t T = (uint32_t)__shfl_up((int)cur, 1, 64);
                if (lane == 0) T = top0;
                const int xl = t - lane;
                if (lane < nl && xl >= 0 && xl < tw) {
                    const int x = c0 + xl;
                    uint32_t pred;
                    if (y == 0) pred = x == 0 ? 0u : cur;
                    else if (x == 0) pred = T;
                    else pred = (uint32_t)min(max((int)cur + (int)T - (int)tl, 0), 255);
                    cur = (pred + res) & 255u;
                    mine[xl] = (uint8_t)cur;
                    tl = T;
                }
            }
            __syncthreads();
            // the tile out
            for (int r = 0; r < nl; r++) {
                const size_t g0 = (size_t)(y0 + r) * w + (size_t)c0, g1 = g0 + (size_t)tw, sa = g0 & ~(size_t)3;
                const int nw = (int)((g0 - sa) + (size_t)tw + 3) / 4;
                for (int i = lane; i < nw; i += 64) {
                    const size_t ga = sa + 4 * (size_t)i;
                    const uint32_t v = ldsw[(r + 1) * (ZW_AG_LROW / 4) + i];
                    if (ga >= g0 && ga + 4 <= g1) {
                        *(uint32_t*)(p + ga) = v;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (ga + k >= g0 && ga + k < g1) p[ga + k] = (uint8_t)(v >> (8 * k));
                    }
                }
            }
            __syncthreads();
        }
        // the next band reads this band's last row back from memory
        __threadfence();
        __syncthreads();
    }
}

namespace {

template <class E>
__device__ __forceinline__ E alpha_elem(uint32_t byte, float scale, float bias)
{
    if constexpr (sizeof(E) == 1) return (E)byte;
    else return (E)__fadd_rn(__fmul_rn((float)byte, scale), bias);  // (float -> _Float16: round to nearest even)
}

// One thread per 4 pixels of a row: channel 3 of frame blockIdx.z, if the frame has alpha.
template <int LAYOUT, class E>
__device__ __forceinline__ void alpha_store_body(const uint8_t* __restrict__ planes, size_t pstride,
                                                 const ZwAlphaFrame* __restrict__ tab, int w, E* __restrict__ out,
                                                 const ZwY2rDev& P)
{
    const int f = (int)blockIdx.z, y = (int)blockIdx.y;
    const int x = (int)(blockIdx.x * 256u + threadIdx.x) * 4;
    if (x >= w || !tab[f].has_alpha) return;
    const uint8_t* a = planes + (size_t)tab[f].plane * pstride + (size_t)y * w + (size_t)x;
    const int n = min(4, w - x);
    uint32_t word = 0;
    if (((uintptr_t)a & 3) == 0) {
        word = *(const uint32_t*)a;  // (inside the plane's slack when n < 4)
    } else {
        for (int k = 0; k < n; k++) word |= (uint32_t)a[k] << (8 * k);
    }
    E* o = out + (size_t)f * P.frame_stride + (size_t)y * P.row_stride;
    if constexpr (LAYOUT == 0) {
        o += (size_t)x * 4 + 3;
        for (int k = 0; k < n; k++) o[4 * k] = alpha_elem<E>((word >> (8 * k)) & 255u, P.scale[3], P.bias[3]);
    } else {
        o += 3 * P.plane_stride + (size_t)x;
        for (int k = 0; k < n; k++) o[k] = alpha_elem<E>((word >> (8 * k)) & 255u, P.scale[3], P.bias[3]);
    }
}

}  // namespace

// One named kernel per (layout, dtype): X(name, LAYOUT, E, dtype index)
#define ZW_ALPHA_STORE_KERNELS(X)             \
    X(k_alpha_store_hwc_u8, 0, uint8_t, 0)    \
    X(k_alpha_store_hwc_f16, 0, _Float16, 1)  \
    X(k_alpha_store_hwc_f32, 0, float, 2)     \
    X(k_alpha_store_chw_u8, 1, uint8_t, 0)    \
    X(k_alpha_store_chw_f16, 1, _Float16, 1)  \
    X(k_alpha_store_chw_f32, 1, float, 2)
#define ZW_ALPHA_STORE_DEFINE(name, LAYOUT, E, DT)                                                                   \
    extern "C" __global__ __launch_bounds__(256) void name(const uint8_t* __restrict__ planes, size_t pstride,        \
                                                           const ZwAlphaFrame* __restrict__ tab, int w,                \
                                                           E* __restrict__ out, ZwY2rDev P)                            \
    {                                                                                                                  \
        alpha_store_body<LAYOUT, E>(planes, pstride, tab, w, out, P);                                                  \
    }
ZW_ALPHA_STORE_KERNELS(ZW_ALPHA_STORE_DEFINE)

// The bytes between two planes of a chunk for w x h frames.
extern "C" size_t zw_alpha_plane_stride(size_t w, size_t h) { return ((w * h + 15) & ~(size_t)15) + 16; }

// Undoes `filter` (1 horizontal, 2 vertical, 3 gradient) in the planes of the
// `count` frames list[0 .. count) (device memory; indices into planes).
extern "C" hipError_t zwk_alpha_unfilter(hipStream_t s, uint8_t* planes, size_t pstride, int w, int h, int filter,
                                         const uint32_t* list, int count)
{
    if (count <= 0 || filter == 0) return hipSuccess;
    if (w <= 0 || h <= 0 || filter < 0 || filter > 3 || pstride < zw_alpha_plane_stride((size_t)w, (size_t)h))
        return hipErrorInvalidValue;
    if (filter == 1) {
        hipLaunchKernelGGL(k_alpha_col0, dim3((unsigned)count), dim3(64), 0, s, planes, pstride, w, h, list);
        hipLaunchKernelGGL(k_alpha_rows, dim3(((unsigned)h + 3) / 4, (unsigned)count), dim3(256), 0, s, planes, pstride,
                           w, h, list);
    } else if (filter == 2) {
        hipLaunchKernelGGL(k_alpha_rows, dim3(1, (unsigned)count), dim3(256), 0, s, planes, pstride, w, 1, list);
        if (h > 1) {
            if (w % 4 == 0)
                hipLaunchKernelGGL(k_alpha_cols_word, dim3(((unsigned)w / 4 + 255) / 256, (unsigned)count), dim3(256), 0,
                                   s, planes, pstride, w, h, list);
            else
                hipLaunchKernelGGL(k_alpha_cols_byte, dim3(((unsigned)w + 255) / 256, (unsigned)count), dim3(256), 0, s,
                                   planes, pstride, w, h, list);
        }
    } else {
        hipLaunchKernelGGL(k_alpha_gradient, dim3((unsigned)count), dim3(64), 0, s, planes, pstride, w, h, list);
    }
    return hipGetLastError();
}

// Channel 3 of the chunk's nframes frames (out = the chunk's first frame), as
// zwk_yuv2rgb_dev addresses them; layout 0 HWC / 1 CHW, dtype 0 u8 / 1 f16 / 2 f32.
extern "C" hipError_t zwk_alpha_store(hipStream_t s, const uint8_t* planes, size_t pstride, const ZwAlphaFrame* tab,
                                      int w, int h, int layout, int dtype, void* out, const ZwY2rDev* P, int nframes)
{
    const void* fn = nullptr;
#define ZW_ALPHA_STORE_PICK(name, LAYOUT, E, DT) \
    if (layout == LAYOUT && dtype == DT) fn = (const void*)name;
    ZW_ALPHA_STORE_KERNELS(ZW_ALPHA_STORE_PICK)
    if (!fn || w <= 0 || h <= 0 || nframes <= 0) return hipErrorInvalidValue;
    ZwY2rDev p = *P;
    void* args[] = {&planes, &pstride, &tab, &w, &out, &p};
    const dim3 grid(((unsigned)w + 1023) / 1024, (unsigned)h, (unsigned)nframes);
    return hipLaunchKernel(fn, grid, dim3(256), args, 0, s);
}
