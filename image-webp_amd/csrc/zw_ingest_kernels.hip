// zw_ingest_kernels.hip -- RGB(A) frames of a device tensor -> the encoder's
// MB-padded Y/U/V planes (gfx950).
//
//   k_rgb2yuv_dev<layout, dtype, channels>   convert_image_yuv (decoder/yuv.rs:656)
//                 over the bytes the pixel rule (zw_ingest.h) makes of an HWC or
//                 CHW tensor of u8 / f16 / f32 elements, 3 or 4 channels.
//
// The planes equal k_rgb2yuv's of the packed u8 image the rule makes on the
// host; that image is never materialised.  Shaped like k_rgb2yuv_rows
// (zw_prepass_kernels.hip): one thread per 8x2 luma pixels (4 chroma samples), a
// wave reading 64 consecutive 8-pixel runs of two rows, 8-byte luma and 4-byte
// chroma stores.  Loads per row of a run (nontemporal: the tensor is read once):
//   CHW u8   one 8-byte load a plane        HWC u8 x 3   three 8-byte loads
//   CHW f16  one 16-byte load a plane       HWC u8 x 4   two 16-byte loads
//   CHW f32  two 16-byte loads a plane      HWC f16/f32  the run's 8*channels
//                                           elements in 16-byte loads
// exactly the run's own elements, so no load leaves the row.  Runs that reach
// the right edge and the padding rows below the image take the per-sample path
// (edge replication by clamped coordinates, one element a load), and so does
// every run when the launcher finds a base address or stride that would
// misalign a vector load (ing_vec_ok).  Plane 3 of a CHW tensor is never read;
// channel 3 of an HWC pixel comes in with its vector and is dropped.
#include "zw_dev.h"
#include "zw_ingest.h"

namespace {

struct IngestArgs {
    const uint8_t* data;                             // frame 0 of the launch
    size_t frame_stride, plane_stride, row_stride;   // in elements
    float scale[4], bias[4];
    int w, h, mbw, mbh;
    uint8_t *Y, *U, *V;
    size_t ysz, csz;
    int vec;  // every run's loads are aligned (ing_vec_ok and 8-byte aligned planes)
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// an element's bits -> the byte the encoder sees
template <int DTYPE>
DI uint32_t ing_cvt(uint32_t bits, float sc, float bi)
{
    if (DTYPE == ZW_ING_U8) return bits;
    if (DTYPE == ZW_ING_F16) return ing_byte_f16((uint16_t)bits, sc, bi);
    return ing_byte_f32(__uint_as_float(bits), sc, bi);
}

template <int DTYPE>
DI uint32_t ing_load(const uint8_t* fr, size_t e)
{
    if (DTYPE == ZW_ING_U8) return fr[e];
    if (DTYPE == ZW_ING_F16) return ((const uint16_t*)fr)[e];
    return ((const uint32_t*)fr)[e];
}

// pixel (x, y) of the frame at fr as 0x00BBGGRR, one element a load
template <int LAYOUT, int DTYPE, int CH>
DI uint32_t ing_pixel(const IngestArgs& A, const uint8_t* fr, int x, int y)
{
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t e = LAYOUT == ZW_ING_CHW ? (size_t)c * A.plane_stride + (size_t)y * A.row_stride + (size_t)x
                                              : (size_t)y * A.row_stride + (size_t)x * CH + c;
        px |= ing_cvt<DTYPE>(ing_load<DTYPE>(fr, e), A.scale[c], A.bias[c]) << (8 * c);
    }
    return px;
}

DI uint32_t ing_y(uint32_t p)
{
    return (16839u * (p & 255u) + 33059u * ((p >> 8) & 255u) + 6420u * ((p >> 16) & 255u) + (1u << 15) + (16u << 16)) >> 16;
}

// chroma sample (cx, cy) and its 2x2 luma pixels: rgb2yuv_sample over ing_pixel
template <int LAYOUT, int DTYPE, int CH>
DI void ing_sample(const IngestArgs& A, const uint8_t* fr, int cx, int cy, uint8_t* __restrict__ Yf,
                   uint8_t* __restrict__ Uf, uint8_t* __restrict__ Vf)
{
    const int w = A.w, h = A.h, cw = A.mbw * 8, lw = A.mbw * 16;
    const int acw = (w + 1) / 2, ach = (h + 1) / 2;
    uint32_t p[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            p[dy][dx] = ing_pixel<LAYOUT, DTYPE, CH>(A, fr, min(2 * cx + dx, w - 1), min(2 * cy + dy, h - 1));
            Yf[(size_t)(2 * cy + dy) * lw + 2 * cx + dx] = (uint8_t)ing_y(p[dy][dx]);
        }
    if (cx >= acw || cy >= ach) {  // padding: the chroma of the last real sample
        const int scx = min(cx, acw - 1), scy = min(cy, ach - 1);
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++)
                p[dy][dx] = ing_pixel<LAYOUT, DTYPE, CH>(A, fr, min(2 * scx + dx, w - 1), min(2 * scy + dy, h - 1));
    }
    const int su = pk_u(p[0][0]) + pk_u(p[0][1]) + pk_u(p[1][0]) + pk_u(p[1][1]) + (512 << 16);
    const int sv = pk_v(p[0][0]) + pk_v(p[0][1]) + pk_v(p[1][0]) + pk_v(p[1][1]) + (512 << 16);
    Uf[(size_t)cy * cw + cx] = (uint8_t)((su + (1 << 17)) >> 18);
    Vf[(size_t)cy * cw + cx] = (uint8_t)((sv + (1 << 17)) >> 18);
}

// NW words at p in PIECE-byte nontemporal loads (p aligned to PIECE)
template <int NW, int PIECE>
DI void ing_words(const uint8_t* __restrict__ p, uint32_t wd[NW])
{
    if (PIECE == 16) {
#pragma unroll
        for (int i = 0; i < NW / 4; i++) {
            const u32x4 v = __builtin_nontemporal_load((const u32x4*)(p + 16 * i));
            wd[4 * i] = v.x; wd[4 * i + 1] = v.y; wd[4 * i + 2] = v.z; wd[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW / 2; i++) {
            const u32x2 v = __builtin_nontemporal_load((const u32x2*)(p + 8 * i));
            wd[2 * i] = v.x; wd[2 * i + 1] = v.y;
        }
    }
}

// element e of the words of a run
template <int DTYPE>
DI uint32_t ing_elem(const uint32_t* wd, int e)
{
    if (DTYPE == ZW_ING_U8) return (wd[e >> 2] >> (8 * (e & 3))) & 255u;
    if (DTYPE == ZW_ING_F16) return (wd[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    return wd[e];
}

// The 8 pixels at (x0 .. x0 + 7, y) as 0x..BBGGRR words, by vector loads.
template <int LAYOUT, int DTYPE, int CH>
DI void ing_run8(const IngestArgs& A, const uint8_t* __restrict__ fr, int x0, int y, uint32_t px[8])
{
    constexpr int ES = ing_elsize(DTYPE), PIECE = ing_piece_bytes(LAYOUT, DTYPE, CH);  // (as ing_vec_ok counts them)
    if (LAYOUT == ZW_ING_HWC) {
        constexpr int NW = 8 * CH * ES / 4;
        uint32_t wd[NW];
        ing_words<NW, PIECE>(fr + ((size_t)y * A.row_stride + (size_t)x0 * CH) * ES, wd);
        if (DTYPE == ZW_ING_U8 && CH == 4) {
#pragma unroll
            for (int j = 0; j < 8; j++) px[j] = wd[j];
        } else if (DTYPE == ZW_ING_U8) {
#pragma unroll
            for (int q = 0; q < 2; q++) {  // 4 pixels in 3 words
                const uint32_t w0 = wd[3 * q], w1 = wd[3 * q + 1], w2 = wd[3 * q + 2];
                px[4 * q] = w0;
                px[4 * q + 1] = __builtin_amdgcn_alignbyte(w1, w0, 3);
                px[4 * q + 2] = __builtin_amdgcn_alignbyte(w2, w1, 2);
                px[4 * q + 3] = w2 >> 8;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                px[j] = 0;
#pragma unroll
                for (int c = 0; c < 3; c++)
                    px[j] |= ing_cvt<DTYPE>(ing_elem<DTYPE>(wd, j * CH + c), A.scale[c], A.bias[c]) << (8 * c);
            }
        }
    } else {
        constexpr int NW = 8 * ES / 4;
#pragma unroll
        for (int j = 0; j < 8; j++) px[j] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint32_t wd[NW];
            ing_words<NW, PIECE>(fr + ((size_t)c * A.plane_stride + (size_t)y * A.row_stride + (size_t)x0) * ES, wd);
#pragma unroll
            for (int j = 0; j < 8; j++)
                px[j] |= ing_cvt<DTYPE>(ing_elem<DTYPE>(wd, j), A.scale[c], A.bias[c]) << (8 * c);
        }
    }
}

static_assert(ZW_ING_HWC == 0 && ZW_ING_CHW == 1 && ZW_ING_U8 == 0 && ZW_ING_F16 == 1 && ZW_ING_F32 == 2, "ABI values");

template <int LAYOUT, int DTYPE, int CH>
__global__ __launch_bounds__(256) void k_rgb2yuv_dev(const IngestArgs A)
{
    constexpr int ES = ing_elsize(DTYPE);
    const int w = A.w, h = A.h;
    const int cw = A.mbw * 8, chh = A.mbh * 8, lw = A.mbw * 16, gpr = A.mbw * 2;  // 4-sample groups per chroma row
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= gpr * chh) return;
    const int g = idx % gpr, cy = idx / gpr;
    const int cx0 = 4 * g, px0 = 8 * g;
    const uint8_t* fr = A.data + (size_t)f * A.frame_stride * ES;
    uint8_t* Yf = A.Y + (size_t)f * A.ysz;
    uint8_t* Uf = A.U + (size_t)f * A.csz;
    uint8_t* Vf = A.V + (size_t)f * A.csz;
    if (A.vec && ing_run_in_row(px0, w) && cy < (h + 1) / 2) {
        const int r0 = 2 * cy, r1 = min(2 * cy + 1, h - 1);
        uint32_t a[8], b[8];
        ing_run8<LAYOUT, DTYPE, CH>(A, fr, px0, r0, a);
        ing_run8<LAYOUT, DTYPE, CH>(A, fr, px0, r1, b);
        const uint32_t ya[2] = {pk_y4(a[0], a[1], a[2], a[3]), pk_y4(a[4], a[5], a[6], a[7])};
        const uint32_t yb[2] = {pk_y4(b[0], b[1], b[2], b[3]), pk_y4(b[4], b[5], b[6], b[7])};
        uint32_t uw = 0, vw = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int su = pk_u(a[2 * j]) + pk_u(a[2 * j + 1]) + pk_u(b[2 * j]) + pk_u(b[2 * j + 1]) + (512 << 16);
            const int sv = pk_v(a[2 * j]) + pk_v(a[2 * j + 1]) + pk_v(b[2 * j]) + pk_v(b[2 * j + 1]) + (512 << 16);
            uw |= (uint32_t)((su + (1 << 17)) >> 18) << (8 * j);
            vw |= (uint32_t)((sv + (1 << 17)) >> 18) << (8 * j);
        }
        *(uint2*)(Yf + (size_t)(2 * cy) * lw + px0) = make_uint2(ya[0], ya[1]);
        *(uint2*)(Yf + (size_t)(2 * cy + 1) * lw + px0) = make_uint2(yb[0], yb[1]);
        *(uint32_t*)(Uf + (size_t)cy * cw + cx0) = uw;
        *(uint32_t*)(Vf + (size_t)cy * cw + cx0) = vw;
    } else {
#pragma unroll 1
        for (int j = 0; j < 4; j++) ing_sample<LAYOUT, DTYPE, CH>(A, fr, cx0 + j, cy, Yf, Uf, Vf);
    }
}

template <int LAYOUT, int DTYPE, int CH>
void launch(hipStream_t s, const IngestArgs& A, int nframes)
{
    const int ng = A.mbw * 2 * A.mbh * 8;
    hipLaunchKernelGGL((k_rgb2yuv_dev<LAYOUT, DTYPE, CH>), dim3((ng + 255) / 256, nframes), dim3(256), 0, s, A);
}
template <int LAYOUT, int DTYPE>
void launch_ch(hipStream_t s, const IngestArgs& A, int ch, int nframes)
{
    if (ch == 3) launch<LAYOUT, DTYPE, 3>(s, A, nframes);
    else launch<LAYOUT, DTYPE, 4>(s, A, nframes);
}
template <int LAYOUT>
void launch_dt(hipStream_t s, const IngestArgs& A, int dtype, int ch, int nframes)
{
    if (dtype == ZW_ING_U8) launch_ch<LAYOUT, ZW_ING_U8>(s, A, ch, nframes);
    else if (dtype == ZW_ING_F16) launch_ch<LAYOUT, ZW_ING_F16>(s, A, ch, nframes);
    else launch_ch<LAYOUT, ZW_ING_F32>(s, A, ch, nframes);
}

}  // namespace

// nframes frames from `data` (frame 0 of the launch; strides in elements, the
// caller has checked them with ing_span) into MB-padded planes.  The vector
// form needs every run's loads aligned (ing_vec_ok) and 8-byte aligned luma
// rows, as zwk_rgb2yuv chooses; anything else runs per sample.
extern "C" hipError_t zwk_rgb2yuv_dev(hipStream_t s, const void* data, int layout, int dtype, int channels,
                                      size_t frame_stride, size_t plane_stride, size_t row_stride, const float* scale,
                                      const float* bias, int w, int h, int mbw, int mbh, uint8_t* Y, uint8_t* U,
                                      uint8_t* V, size_t ysz, size_t csz, int nframes)
{
    if ((layout != ZW_ING_HWC && layout != ZW_ING_CHW) || dtype < ZW_ING_U8 || dtype > ZW_ING_F32 ||
        (channels != 3 && channels != 4) || !data || nframes <= 0)
        return hipErrorInvalidValue;
    IngestArgs A;
    A.data = (const uint8_t*)data;
    A.frame_stride = frame_stride;
    A.plane_stride = plane_stride;
    A.row_stride = row_stride;
    for (int c = 0; c < 4; c++) {
        A.scale[c] = scale[c];
        A.bias[c] = bias[c];
    }
    A.w = w; A.h = h; A.mbw = mbw; A.mbh = mbh;
    A.Y = Y; A.U = U; A.V = V;
    A.ysz = ysz; A.csz = csz;
    const bool planes_ok = ((uintptr_t)Y | (uintptr_t)U | (uintptr_t)V | ysz | csz) % 8 == 0;
    A.vec = planes_ok && ing_vec_ok(layout, dtype, channels, (uintptr_t)data, frame_stride, plane_stride, row_stride);
    if (layout == ZW_ING_HWC) launch_dt<ZW_ING_HWC>(s, A, dtype, channels, nframes);
    else launch_dt<ZW_ING_CHW>(s, A, dtype, channels, nframes);
    return hipGetLastError();
}
