// zw_vp8l_kernels.hip -- the pixel half of a lossless (VP8L) decode on the
// device (gfx950): the four inverse transforms of decoder/lossless_transform.rs
// and the store into the caller's tensor.
//
// The host threads entropy-decode each file (zw_vp8l_dec.cpp, decode_coded) into
// a chunk: frame f's slot (ZwLlChunk, zw_common.h) holds its coded image, tw * h
// pixels of 4 bytes R, G, B, A (one little-endian word 0xAABBGGRR), and its
// transform data; one ZwLlFrame entry describes it.  The transforms are undone
// in reverse bitstream order: inverse step k of every frame runs before step
// k + 1, and for each (step, type) one launch covers the frames of `list` whose
// step k is of that type.  A frame works its coded buffer at width tw until its
// colour indexing inverse has expanded it into the frame's full-width buffer,
// and that one at the canvas width afterwards (ll_pixels).
//
//   predictor      k_ll_predictor: one wave per frame, a skewed wavefront (below).
//   cross-colour   k_ll_color, elementwise in place.
//   subtract-green k_ll_subgreen, elementwise in place.
//   indexing       k_ll_index, out of place: packed coded image -> full width.
//   store          k_ll_store_*: the final words into the tensor by
//                  k_yuv2rgb_dev's rule (u8 the byte; f32 v * scale[c] + bias[c]
//                  as a rounded multiply and a rounded add; f16 that float
//                  rounded to nearest even; HWC or CHW, the caller's strides,
//                  the gaps never written); channel 3 is the decoded alpha of a
//                  frame with has_alpha, 255 otherwise.
//
// No kernel here waits for another wave or workgroup and none has a barrier,
// so none can hang.  Bounds: every address follows from w, h, the frame's tw
// and the chunk's strides; a lane outside the image neither loads nor stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zw_common.h"

namespace {

// four byte adds mod 256 in one word
__device__ __forceinline__ uint32_t add_bytes(uint32_t a, uint32_t b)
{
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}
// four floor((a + b) / 2) in one word (average2, lossless_transform.rs:582-584)
__device__ __forceinline__ uint32_t avg_bytes(uint32_t a, uint32_t b)
{
    return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1);
}
// sum over the four bytes of |a - b|
__device__ __forceinline__ uint32_t sad_bytes(uint32_t a, uint32_t b)
{
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 255u) - (int)((b >> k) & 255u);
        s += (uint32_t)(d < 0 ? -d : d);
    }
    return s;
}
__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

// The prediction of a pixel below row 0 and right of column 0 from L, T, TL, TR
// (apply_predictor_transform_N, lossless_transform.rs:77-353).  Lanes of one
// wave may hold different modes: a plain switch.
__device__ __forceinline__ uint32_t ll_predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR)
{
    switch (mode) {
    case 0: return 0xff000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return avg_bytes(avg_bytes(L, TR), T);
    case 6: return avg_bytes(L, TL);
    case 7: return avg_bytes(L, T);
    case 8: return avg_bytes(TL, T);
    case 9: return avg_bytes(T, TR);
    case 10: return avg_bytes(avg_bytes(L, TL), avg_bytes(T, TR));
    case 11:  // select: |L + T - TL - L| = |T - TL| summed against |L - TL| summed
        return sad_bytes(T, TL) < sad_bytes(L, TL) ? L : T;
    case 12: {  // clamp(L + T - TL)
        uint32_t p = 0;
#pragma unroll
        for (int k = 0; k < 32; k += 8)
            p |= clamp255((int)((L >> k) & 255u) + (int)((T >> k) & 255u) - (int)((TL >> k) & 255u)) << k;
        return p;
    }
    case 13: {  // clamp(a + (a - TL) / 2), a = (L + T) / 2; the division truncates towards zero
        uint32_t p = 0;
#pragma unroll
        for (int k = 0; k < 32; k += 8) {
            const int a = ((int)((L >> k) & 255u) + (int)((T >> k) & 255u)) / 2;
            p |= clamp255(a + (a - (int)((TL >> k) & 255u)) / 2) << k;
        }
        return p;
    }
    default: return 0u;  // (modes 14 and up leave the residual)
    }
}

// Frame f's pixels before inverse step `step` (step == nsteps: the final image) and their width.
__device__ __forceinline__ uint32_t* ll_pixels(const ZwLlChunk& C, uint32_t f, const ZwLlFrame& F, uint32_t step, int* width)
{
    const bool expanded = F.index_step != ZW_LL_NO_INDEX && F.index_step < step;
    *width = expanded ? C.w : (int)F.tw;
    return (uint32_t*)(expanded ? C.full + (size_t)f * C.bstride : C.slots + (size_t)f * C.sstride);
}
__device__ __forceinline__ const uint32_t* ll_data(const ZwLlChunk& C, uint32_t f, const ZwLlFrame& F, uint32_t step)
{
    return (const uint32_t*)(C.slots + (size_t)f * C.sstride + C.doff + F.s[step].off);
}

}  // namespace

// The predictor inverse (inverse_predictor / predict_run of zw_vp8l_dec.cpp are
// the host statement).  One wave per listed frame walks the frame's bands of 64
// rows in order; lane j owns row 64 b + j of band b and works column t - 2 j at
// step t.  With that skew of two, TR is what the lane above made one step
// earlier (a one-lane shift of `cur`), T is the TR of the step before and TL the
// one before that: a three-deep history in registers, shifted every step whether
// the lane is inside the image or not.  Lane 0 takes its TR from the row above
// the band, which the same wave stored a band earlier (a fence between bands).
// The last column's TR is the row's own column 0 (the reference's flat
// indexing), which the lane keeps in `first`.
//
// Residuals come from and results go to global memory directly: a lane walks
// its own row, so consecutive steps share cache lines, and the loads of the
// next four steps are issued before this group's chain runs.  Nothing is staged
// in LDS: without a tile there is no barrier, no tile-edge case and no limit on
// the width, and the batch is bound by the host's entropy decode, which this
// kernel runs beside (DESIGN.md section 4 has the measurement).  The price is
// that a step's load and store each touch 64 cache lines, one per row; a wave
// spends 0.35-0.44 us a step on that, far more than its arithmetic needs, and
// skewed LDS tiles are the way to get it back should the host ever be faster.
extern "C" __global__ __launch_bounds__(64) void k_ll_predictor(ZwLlChunk C, uint32_t step,
                                                                const uint32_t* __restrict__ list)
{
    const uint32_t f = list[blockIdx.x];
    const ZwLlFrame F = C.tab[f];
    int w;
    uint32_t* px = ll_pixels(C, f, F, step, &w);
    const int h = C.h;
    const uint32_t bits = F.s[step].bits;
    const uint32_t* pimg = ll_data(C, f, F, step);
    const int bxs = (w + (1 << bits) - 1) >> bits, bmask = (1 << bits) - 1;
    const int lane = (int)threadIdx.x;
    for (int y0 = 0; y0 < h; y0 += 64) {
        const int nl = min(64, h - y0);
        const int y = y0 + lane;
        const bool live = lane < nl;
        uint32_t* row = px + (size_t)(live ? y : y0) * w;
        const uint32_t* above = px + (size_t)(y0 > 0 ? y0 - 1 : 0) * w;
        const uint32_t* prow = pimg + (size_t)((live ? y : y0) >> bits) * bxs;
        const bool top = lane == 0 && y0 > 0;  // the lane that reads the row above the band
        uint32_t cur = 0, first = 0, T = top ? above[0] : 0u, TL = 0, mode = 0;
        const int steps = w + 2 * (nl - 1);
        // the residuals (and lane 0's TR) of the four steps from t0
        uint32_t rn[4], an[4];
        auto fetch = [&](int t0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int x = t0 + k - 2 * lane;
                rn[k] = (live && x >= 0 && x < w) ? row[x] : 0u;
                an[k] = (top && t0 + k + 1 < w) ? above[t0 + k + 1] : 0u;
            }
        };
        fetch(0);
        for (int t0 = 0; t0 < steps; t0 += 4) {
            uint32_t res[4], top4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) res[k] = rn[k], top4[k] = an[k];
            if (t0 + 4 < steps) fetch(t0 + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t up = (uint32_t)__shfl_up((int)cur, 1, 64);
                if (lane == 0) up = top4[k];
                const int x = t0 + k - 2 * lane;
                if (live && x >= 0 && x < w) {
                    uint32_t pred;
                    if (y == 0) {
                        pred = x == 0 ? 0xff000000u : cur;
                    } else if (x == 0) {
                        pred = T;
                    } else {
                        if (x == 1 || (x & bmask) == 0) mode = (prow[x >> bits] >> 8) & 255u;
                        pred = ll_predict(mode, cur, T, TL, x == w - 1 ? first : up);
                    }
                    cur = add_bytes(res[k], pred);
                    row[x] = cur;
                    if (x == 0) first = cur;
                }
                TL = T;
                T = up;
            }
        }
        // the next band reads this band's last row back from memory
        __threadfence();
    }
}

// The cross-colour inverse (inverse_color): one thread per pixel of frame
// list[blockIdx.z], row blockIdx.y.  color_delta is (int8 * int8) >> 5, of which
// the low byte is kept; red is updated before blue reads it.
extern "C" __global__ __launch_bounds__(256) void k_ll_color(ZwLlChunk C, uint32_t step, const uint32_t* __restrict__ list)
{
    const uint32_t f = list[blockIdx.z];
    const ZwLlFrame F = C.tab[f];
    int w;
    uint32_t* px = ll_pixels(C, f, F, step, &w);
    const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y;
    if (x >= w) return;
    const uint32_t bits = F.s[step].bits;
    const int bxs = (w + (1 << bits) - 1) >> bits;
    const uint32_t t = ll_data(C, f, F, step)[(size_t)(y >> bits) * bxs + (x >> bits)];
    const int red_to_blue = (int8_t)(t & 255u), green_to_blue = (int8_t)((t >> 8) & 255u),
              green_to_red = (int8_t)((t >> 16) & 255u);
    const uint32_t p = px[(size_t)y * w + x];
    const int green = (int8_t)((p >> 8) & 255u);
    uint32_t red = p & 255u, blue = (p >> 16) & 255u;
    red = (red + ((uint32_t)(green_to_red * green) >> 5)) & 255u;
    blue += (uint32_t)(green_to_blue * green) >> 5;
    blue = (blue + ((uint32_t)(red_to_blue * (int)(int8_t)red) >> 5)) & 255u;
    px[(size_t)y * w + x] = (p & 0xff00ff00u) | red | (blue << 16);
}

// The subtract-green inverse: green is added to red and blue.
extern "C" __global__ __launch_bounds__(256) void k_ll_subgreen(ZwLlChunk C, uint32_t step,
                                                               const uint32_t* __restrict__ list)
{
    const uint32_t f = list[blockIdx.z];
    const ZwLlFrame F = C.tab[f];
    int w;
    uint32_t* px = ll_pixels(C, f, F, step, &w);
    const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y;
    if (x >= w) return;
    const uint32_t p = px[(size_t)y * w + x], g = (p >> 8) & 255u;
    px[(size_t)y * w + x] = add_bytes(p, g | (g << 16));
}

// The colour indexing inverse (inverse_color_indexing), out of place: the coded
// image's green bytes hold 8 / 4 / 2 / 1 table indices each, least significant
// bits first; one thread per pixel of the full-width image.  An index past the
// table is 0x00000000.
extern "C" __global__ __launch_bounds__(256) void k_ll_index(ZwLlChunk C, uint32_t step, const uint32_t* __restrict__ list)
{
    const uint32_t f = list[blockIdx.z];
    const ZwLlFrame F = C.tab[f];
    const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y;
    if (x >= C.w) return;
    const uint32_t table_size = F.s[step].bits;
    const uint32_t wbits = table_size <= 2 ? 3 : (table_size <= 4 ? 2 : (table_size <= 16 ? 1 : 0));
    const uint32_t per = 1u << wbits, bpe = 8u >> wbits, mask = (1u << bpe) - 1;
    const uint32_t* src = (const uint32_t*)(C.slots + (size_t)f * C.sstride);
    uint32_t* dst = (uint32_t*)(C.full + (size_t)f * C.bstride);
    const uint32_t packed = (src[(size_t)y * F.tw + ((uint32_t)x >> wbits)] >> 8) & 255u;
    const uint32_t k = (packed >> (((uint32_t)x & (per - 1)) * bpe)) & mask;
    dst[(size_t)y * C.w + x] = k < table_size ? ll_data(C, f, F, step)[k] : 0u;
}

namespace {

template <class E>
__device__ __forceinline__ E ll_elem(uint32_t byte, float scale, float bias)
{
    if constexpr (sizeof(E) == 1) return (E)byte;
    else return (E)__fadd_rn(__fmul_rn((float)byte, scale), bias);  // (float -> _Float16: round to nearest even)
}

// One thread per pixel of frame blockIdx.z, row blockIdx.y.
template <int LAYOUT, class E>
__device__ __forceinline__ void ll_store_body(const ZwLlChunk& C, int channels, E* __restrict__ out, const ZwY2rDev& P)
{
    const uint32_t f = blockIdx.z;
    const ZwLlFrame F = C.tab[f];
    const int x = (int)(blockIdx.x * 256u + threadIdx.x), y = (int)blockIdx.y;
    if (x >= C.w) return;
    int w;
    const uint32_t* px = ll_pixels(C, f, F, F.nsteps, &w);  // (w == C.w: tw is the canvas width without indexing)
    uint32_t p = px[(size_t)y * C.w + x];
    if (!F.has_alpha) p |= 0xff000000u;
    E* o = out + (size_t)f * P.frame_stride + (size_t)y * P.row_stride;
    if constexpr (LAYOUT == 0) {
        o += (size_t)x * channels;
        if (sizeof(E) == 1 && channels == 4 && ((uintptr_t)o & 3) == 0) {
            *(uint32_t*)o = p;
            return;
        }
        for (int c = 0; c < channels; c++) o[c] = ll_elem<E>((p >> (8 * c)) & 255u, P.scale[c], P.bias[c]);
    } else {
        o += (size_t)x;
        for (int c = 0; c < channels; c++)
            o[(size_t)c * P.plane_stride] = ll_elem<E>((p >> (8 * c)) & 255u, P.scale[c], P.bias[c]);
    }
}

}  // namespace

// One named kernel per (layout, dtype): X(name, LAYOUT, E, dtype index)
#define ZW_LL_STORE_KERNELS(X)             \
    X(k_ll_store_hwc_u8, 0, uint8_t, 0)    \
    X(k_ll_store_hwc_f16, 0, _Float16, 1)  \
    X(k_ll_store_hwc_f32, 0, float, 2)     \
    X(k_ll_store_chw_u8, 1, uint8_t, 0)    \
    X(k_ll_store_chw_f16, 1, _Float16, 1)  \
    X(k_ll_store_chw_f32, 1, float, 2)
#define ZW_LL_STORE_DEFINE(name, LAYOUT, E, DT)                                                                    \
    extern "C" __global__ __launch_bounds__(256) void name(ZwLlChunk C, int channels, E* __restrict__ out, ZwY2rDev P) \
    {                                                                                                                \
        ll_store_body<LAYOUT, E>(C, channels, out, P);                                                              \
    }
ZW_LL_STORE_KERNELS(ZW_LL_STORE_DEFINE)

// Inverse step `step` for the `count` frames list[0 .. count) whose step is of `type` (device memory).
extern "C" hipError_t zwk_ll_inverse(hipStream_t s, const ZwLlChunk* C, uint32_t step, uint32_t type,
                                     const uint32_t* list, int count)
{
    if (count <= 0) return hipSuccess;
    if (!C || C->w <= 0 || C->h <= 0 || C->w > 16384 || C->h > 16384 || step > 3 || type > 3) return hipErrorInvalidValue;
    const dim3 grid(((unsigned)C->w + 255) / 256, (unsigned)C->h, (unsigned)count);
    if (type == 0) hipLaunchKernelGGL(k_ll_predictor, dim3((unsigned)count), dim3(64), 0, s, *C, step, list);
    else if (type == 1) hipLaunchKernelGGL(k_ll_color, grid, dim3(256), 0, s, *C, step, list);
    else if (type == 2) hipLaunchKernelGGL(k_ll_subgreen, grid, dim3(256), 0, s, *C, step, list);
    else hipLaunchKernelGGL(k_ll_index, grid, dim3(256), 0, s, *C, step, list);
    return hipGetLastError();
}

// The chunk's nframes final images into the caller's tensor (out = the chunk's
// first frame), as zwk_yuv2rgb_dev addresses it; layout 0 HWC / 1 CHW, dtype 0
// u8 / 1 f16 / 2 f32, channels 3 | 4.
extern "C" hipError_t zwk_ll_store(hipStream_t s, const ZwLlChunk* C, int layout, int dtype, int channels, void* out,
                                   const ZwY2rDev* P, int nframes)
{
    const void* fn = nullptr;
#define ZW_LL_STORE_PICK(name, LAYOUT, E, DT) \
    if (layout == LAYOUT && dtype == DT) fn = (const void*)name;
    ZW_LL_STORE_KERNELS(ZW_LL_STORE_PICK)
    if (!fn || !C || C->w <= 0 || C->h <= 0 || nframes <= 0 || (channels != 3 && channels != 4))
        return hipErrorInvalidValue;
    ZwLlChunk c = *C;
    ZwY2rDev p = *P;
    void* args[] = {&c, &channels, &out, &p};
    const dim3 grid(((unsigned)C->w + 255) / 256, (unsigned)C->h, (unsigned)nframes);
    return hipLaunchKernel(fn, grid, dim3(256), args, 0, s);
}
