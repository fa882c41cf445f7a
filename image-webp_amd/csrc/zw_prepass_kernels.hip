// zw_prepass_kernels.hip -- what runs on a frame before its encode passes (gfx950).
//
//   k_rgb2yuv     convert_image_yuv / convert_image_y      (decoder/yuv.rs:656, :806)
//   k_analysis4   analyze_image per-MB alpha + histogram    (encoder/analysis.rs:964)
//   k_segments    k-means, segment quant, matrices, lambdas (analysis.rs:1029, :1145;
//                 vp8.rs:2278-2388, types.rs:806)
#include "zw_dev.h"

// k_analysis4: 4-MB groups per wave (measured, analysis + segments per 256
// 1080p frames: 1 1.375, 2 1.47, 4 1.41 ms).
#ifndef ZW_AN4_GPW
#define ZW_AN4_GPW 1
#endif

// ---------------------------------------------------------------------------
// RGB(A)/L(A) -> padded YUV420.  One thread per chroma sample; it produces the
// 2x2 luma pixels and the U/V sample.  Padding (x >= w, y >= h) is produced by
// clamping the source coordinate, which equals the reference's edge
// replication (yuv.rs:765-803).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int rgb_y(const uint8_t* p)
{
    return (16839 * p[0] + 33059 * p[1] + 6420 * p[2] + (1 << 15) + (16 << 16)) >> 16;
}
__device__ __forceinline__ int rgb_u(const uint8_t* p) { return -9719 * p[0] - 19081 * p[1] + 28800 * p[2] + (128 << 16); }
__device__ __forceinline__ int rgb_v(const uint8_t* p) { return 28800 * p[0] - 24116 * p[1] - 4684 * p[2] + (128 << 16); }

// chroma sample (cx, cy) of one frame and its 2x2 luma pixels
__device__ __forceinline__ void rgb2yuv_sample(const uint8_t* __restrict__ im, int w, int h, int bpp, int mbw, int cx,
                                               int cy, uint8_t* __restrict__ Yf, uint8_t* __restrict__ Uf,
                                               uint8_t* __restrict__ Vf)
{
    const int cw = mbw * 8, lw = mbw * 16;
    const int acw = (w + 1) / 2, ach = (h + 1) / 2;
    const int scx = cx < acw ? cx : acw - 1, scy = cy < ach ? cy : ach - 1;
    int xs[2] = {min(2 * scx, w - 1), min(2 * scx + 1, w - 1)};
    int ys[2] = {min(2 * scy, h - 1), min(2 * scy + 1, h - 1)};
    // luma: the 2x2 pixels this thread owns in the padded plane
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            int px = min(2 * cx + dx, w - 1), py = min(2 * cy + dy, h - 1);
            const uint8_t* p = im + ((size_t)py * w + px) * bpp;
            Yf[(size_t)(2 * cy + dy) * lw + 2 * cx + dx] = (uint8_t)(bpp <= 2 ? p[0] : rgb_y(p));
        }
    uint8_t uo = 127, vo = 127;
    if (bpp > 2) {
        int su = 0, sv = 0;
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const uint8_t* p = im + ((size_t)ys[dy] * w + xs[dx]) * bpp;
                su += rgb_u(p);
                sv += rgb_v(p);
            }
        uo = (uint8_t)((su + (1 << 17)) >> 18);
        vo = (uint8_t)((sv + (1 << 17)) >> 18);
    }
    Uf[(size_t)cy * cw + cx] = uo;
    Vf[(size_t)cy * cw + cx] = vo;
}

extern "C" __global__ void k_rgb2yuv(const uint8_t* __restrict__ img, int w, int h, int bpp, int mbw, int mbh,
                                     uint8_t* __restrict__ Y, uint8_t* __restrict__ U, uint8_t* __restrict__ V,
                                     size_t img_stride, size_t ysz, size_t csz)
{
    const int cw = mbw * 8, chh = mbh * 8;
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cw * chh) return;
    rgb2yuv_sample(img + (size_t)f * img_stride, w, h, bpp, mbw, idx % cw, idx / cw, Y + (size_t)f * ysz,
                   U + (size_t)f * csz, V + (size_t)f * csz);
}

// Row-coalesced form for 3- and 4-byte pixels: one thread per 8x2 luma pixels
// (4 chroma samples), so a wave reads 64 consecutive 8-pixel runs of two rows
// with 16-byte (RGBA) or 8-byte (RGB) loads and writes 8-byte luma and 4-byte
// chroma words.  Runs that reach the right edge and the padding rows below the
// image take the per-sample path (edge replication).  The host launches it
// only when every run is aligned for those loads.
template <int BPP>
__device__ __forceinline__ void rgb_run8(const uint8_t* __restrict__ row, uint32_t px[8])  // 0x..BBGGRR
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    if (BPP == 4) {
        const u32x4 a = __builtin_nontemporal_load((const u32x4*)row);
        const u32x4 b = __builtin_nontemporal_load((const u32x4*)(row + 16));
        px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
        px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
    } else {
        const u32x2 a = __builtin_nontemporal_load((const u32x2*)row);
        const u32x2 b = __builtin_nontemporal_load((const u32x2*)(row + 8));
        const u32x2 c = __builtin_nontemporal_load((const u32x2*)(row + 16));
        const uint32_t wd[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
        for (int q = 0; q < 2; q++) {  // 4 pixels in 3 words
            const uint32_t w0 = wd[3 * q], w1 = wd[3 * q + 1], w2 = wd[3 * q + 2];
            px[4 * q] = w0;
            px[4 * q + 1] = __builtin_amdgcn_alignbyte(w1, w0, 3);
            px[4 * q + 2] = __builtin_amdgcn_alignbyte(w2, w1, 2);
            px[4 * q + 3] = w2 >> 8;
        }
    }
}

template <int BPP>
__global__ __launch_bounds__(256) void k_rgb2yuv_rows(const uint8_t* __restrict__ img, int w, int h, int mbw, int mbh,
                                                      uint8_t* __restrict__ Y, uint8_t* __restrict__ U,
                                                      uint8_t* __restrict__ V, size_t img_stride, size_t ysz,
                                                      size_t csz)
{
    const int cw = mbw * 8, chh = mbh * 8, lw = mbw * 16, gpr = mbw * 2;  // 4-sample groups per chroma row
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= gpr * chh) return;
    const int g = idx % gpr, cy = idx / gpr;
    const int cx0 = 4 * g, px0 = 8 * g;
    const uint8_t* im = img + (size_t)f * img_stride;
    uint8_t* Yf = Y + (size_t)f * ysz;
    uint8_t* Uf = U + (size_t)f * csz;
    uint8_t* Vf = V + (size_t)f * csz;
    if (px0 + 8 <= w && cy < (h + 1) / 2) {
        const int r0 = 2 * cy, r1 = min(2 * cy + 1, h - 1);
        uint32_t a[8], b[8];
        rgb_run8<BPP>(im + ((size_t)r0 * w + px0) * BPP, a);
        rgb_run8<BPP>(im + ((size_t)r1 * w + px0) * BPP, b);
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
#pragma unroll
        for (int j = 0; j < 4; j++) rgb2yuv_sample(im, w, h, BPP, mbw, cx0 + j, cy, Yf, Uf, Vf);
    }
}

// ---------------------------------------------------------------------------
// Analysis (analysis.rs:964), four MBs a wave: 16 lanes an MB, lane j working
// three of the MB's 48 (block, mode) items -- luma block j under DC and under
// TM, chroma block j & 7 (U 0-3, V 4-7) under mode j >> 3 -- so every lane has
// work and the four MBs' chains overlap.  Predictors use source pixels; on the
// MB-padded planes libwebp's import/replicate rules reduce to direct reads
// (analysis.rs:520-745).
// ---------------------------------------------------------------------------
// An MB and its edge pixels staged in LDS.
struct AnalysisTile {
    uint32_t y[16][4];     // luma rows, 4 packed pixels per word
    uint32_t c[2][8][2];   // U, V rows
    uint32_t ytop[4], ctop[2][2];
    uint8_t yleft[16], cleft[2][8];
    uint8_t corner[4];     // Y, U, V
};

// One item: its 16 coefficient bins (min(|c| >> 3, 31)), the count of bin 0 and the largest bin.
DI void an_item(const AnalysisTile* A, bool luma, int mode, int b, bool ht, bool hl, int bins[16], int& z, int& vmax)
{
    const int pl = b >> 2;  // chroma plane
    const int bb = luma ? b : (b & 3);
    const int bx = luma ? (bb & 3) : (bb & 1), by = luma ? (bb >> 2) : (bb >> 1);
    uint32_t st = 0, sl = 0;
    if (luma) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            st = __builtin_amdgcn_sad_u8(A->ytop[w], 0u, st);
            sl = __builtin_amdgcn_sad_u8(((const uint32_t*)A->yleft)[w], 0u, sl);
        }
    } else {
#pragma unroll
        for (int w = 0; w < 2; w++) {
            st = __builtin_amdgcn_sad_u8(A->ctop[pl][w], 0u, st);
            sl = __builtin_amdgcn_sad_u8(((const uint32_t*)A->cleft[pl])[w], 0u, sl);
        }
    }
    const uint32_t s2 = ht && hl ? st + sl : (ht ? 2 * st : 2 * sl);
    const int dcv = (ht || hl) ? (luma ? (int)((s2 + 16) >> 5) : (int)((s2 + 8) >> 4)) : 0x80;
    const int corner = A->corner[luma ? 0 : 1 + pl];
    int d[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = by * 4 + i;
        const uint32_t srow = luma ? A->y[r][bx] : A->c[pl][r][bx];
        const int L = luma ? A->yleft[r] : A->cleft[pl][r];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int cidx = bx * 4 + j;
            const uint32_t tw = luma ? A->ytop[cidx >> 2] : A->ctop[pl][cidx >> 2];
            const int T = (int)((tw >> (8 * (cidx & 3))) & 255u);
            const int tm = (ht && hl) ? clamp255(L + T - corner) : (hl ? L : (ht ? T : 129));
            const int p = mode == 0 ? dcv : tm;
            d[i * 4 + j] = (int)((srow >> (8 * j)) & 255u) - p;
        }
    }
    int o[16];
    fdct16_pk(d, o);
    z = 0;
    vmax = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        bins[k] = min(iabs(o[k]) >> 3, 31);
        z += bins[k] == 0;
        vmax = max(vmax, bins[k]);
    }
}
DI int max8(int v)  // max within aligned 8-lane groups
{
    v = max(v, DPP(v, 0xB1));
    v = max(v, DPP(v, 0x4E));
    return max(v, DPP(v, 0x141));
}
DI int an_red8(int v)  // sum within aligned 8-lane groups
{
    v += DPP(v, 0xB1);
    v += DPP(v, 0x4E);
    return v + DPP(v, 0x141);
}
DI int max16(int v)
{
    v = max8(v);
    return max(v, DPP(v, 0x140));
}
typedef unsigned an_v4u __attribute__((ext_vector_type(4)));
typedef unsigned an_v2u __attribute__((ext_vector_type(2)));
extern "C" __global__ __launch_bounds__(256) void k_analysis4(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ U,
                                                              const uint8_t* __restrict__ V, int mbw, int mbh,
                                                              size_t ysz, size_t csz, uint8_t* __restrict__ alpha,
                                                              uint32_t* __restrict__ histo)
{
    __shared__ AnalysisTile tile[4][4];   // [wave][MB]
    __shared__ uint32_t hist[4][4][4][32];  // [wave][MB][histogram][bin] (only when some bin 0 is short)
    __shared__ uint32_t ahist[256];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, mi = lane >> 4, j = lane & 15;
    const int f = blockIdx.y;
    const int nmb = mbw * mbh;
    ahist[threadIdx.x] = 0;
    __syncthreads();
    const int ys = mbw * 16, cs = mbw * 8;
    const uint8_t* Yf = Y + (size_t)f * ysz;
    const uint8_t* Uf = U + (size_t)f * csz;
    const uint8_t* Vf = V + (size_t)f * csz;
    AnalysisTile* A = &tile[wv][mi];
#pragma unroll 1
    for (int it = 0; it < ZW_AN4_GPW; it++) {
        const int mb = ((blockIdx.x * ZW_AN4_GPW + it) * 4 + wv) * 4 + mi;
        const bool in = mb < nmb;
        const int mbx = in ? mb % mbw : 0, mby = in ? mb / mbw : 0;
        const bool ht = mby > 0, hl = mbx > 0;
        // ---- stage the MB and its edges (lane j: luma row j, chroma row j & 7 of plane j >> 3)
        {
            const int pl = j >> 3, cr = j & 7;
            const uint8_t* Cf = pl ? Vf : Uf;
            an_v4u yr = {0u, 0u, 0u, 0u};
            an_v2u cw = {0u, 0u};
            uint32_t yl = 0, cl = 0;
            if (in) {
                const uint8_t* yp = Yf + (size_t)(mby * 16 + j) * ys + mbx * 16;
                const uint8_t* cp = Cf + (size_t)(mby * 8 + cr) * cs + mbx * 8;
                yr = *(const an_v4u*)yp;
                cw = *(const an_v2u*)cp;
                if (hl) {
                    yl = yp[-1];
                    cl = cp[-1];
                }
            }
            wsync();  // (the previous group's reads of the tile are done)
            *(an_v4u*)A->y[j] = yr;
            *(an_v2u*)A->c[pl][cr] = cw;
            A->yleft[j] = (uint8_t)yl;
            A->cleft[pl][cr] = (uint8_t)cl;
            if (j < 6) {
                uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
                if (in && ht) {
                    if (j == 0) {
                        const an_v4u t = *(const an_v4u*)(Yf + (size_t)(mby * 16 - 1) * ys + mbx * 16);
                        t0 = t.x; t1 = t.y; t2 = t.z; t3 = t.w;
                    } else if (j < 3) {
                        const an_v2u t = *(const an_v2u*)((j == 1 ? Uf : Vf) + (size_t)(mby * 8 - 1) * cs + mbx * 8);
                        t0 = t.x; t1 = t.y;
                    } else if (hl) {
                        const uint8_t* cp = j == 3 ? Yf + (size_t)(mby * 16 - 1) * ys + mbx * 16 - 1
                                                   : (j == 4 ? Uf : Vf) + (size_t)(mby * 8 - 1) * cs + mbx * 8 - 1;
                        t0 = *cp;
                    }
                }
                if (j == 0) {
                    A->ytop[0] = t0; A->ytop[1] = t1; A->ytop[2] = t2; A->ytop[3] = t3;
                } else if (j < 3) {
                    A->ctop[j - 1][0] = t0;
                    A->ctop[j - 1][1] = t1;
                } else {
                    A->corner[j - 3] = (uint8_t)t0;
                }
            }
            wsync();
        }
        // ---- the three items: luma block j under DC (A) and TM (B), chroma block j & 7 under mode j >> 3 (C)
        int bins[16], zA, vA, zB, vB, zC, vC;
        an_item(A, true, 0, j, ht, hl, bins, zA, vA);
        an_item(A, true, 1, j, ht, hl, bins, zB, vB);
        an_item(A, false, j >> 3, j & 7, ht, hl, bins, zC, vC);
        // per histogram (luma DC, luma TM, chroma DC in lanes j < 8, chroma TM in j >= 8):
        // the bin-0 count and the largest bin
        const int z0 = red16(zA), z1 = red16(zB), z23 = an_red8(zC);
        const int v0 = max16(vA), v1 = max16(vB), v23 = max8(vC);
        // fast path: bin 0 holding at least half of a histogram's
        // coefficients is its largest count, and the last non-empty bin is the largest bin
        const bool ok = 2 * z0 >= 256 && 2 * z1 >= 256 && 2 * z23 >= 128;
        int a0, a1, a23;
        if (__ballot(in && !ok) == 0ull) {
            a0 = z0 > 1 ? (int)(510u * (uint32_t)v0 / (uint32_t)z0) : 0;
            a1 = z1 > 1 ? (int)(510u * (uint32_t)v1 / (uint32_t)z1) : 0;
            a23 = z23 > 1 ? (int)(510u * (uint32_t)v23 / (uint32_t)z23) : 0;
        } else {
            // exact histograms: bin 0 counted in the lane, the other bins by LDS atomics
            uint32_t* H = &hist[wv][mi][0][0];
#pragma unroll
            for (int k = 0; k < 8; k++) (&hist[wv][0][0][0])[64 * k + lane] = 0;
            wsync();
#pragma unroll 1
            for (int t = 0; t < 3; t++) {
                int zz, vv;
                const int h = t < 2 ? t : 2 + (j >> 3);
                an_item(A, t < 2, t < 2 ? t : j >> 3, t < 2 ? j : j & 7, ht, hl, bins, zz, vv);
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (bins[k]) atomicAdd(&H[h * 32 + bins[k]], 1u);
                if (zz) atomicAdd(&H[h * 32], (uint32_t)zz);
            }
            wsync();
            int av[4];
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const uint32_t c0 = H[h * 32 + 2 * j], c1 = H[h * 32 + 2 * j + 1];
                const int mx = max16((int)max(c0, c1));
                const int lnz = max16(c1 ? 2 * j + 1 : (c0 ? 2 * j : -1));
                av[h] = mx > 1 ? (int)(510u * (uint32_t)max(lnz, 0) / (uint32_t)mx) : 0;
            }
            a0 = av[0];
            a1 = av[1];
            a23 = j < 8 ? av[2] : av[3];
        }
        const int a3 = __shfl(a23, (lane & ~15) | 8);  // chroma TM's, from lane 8 of the MB
        if (j == 0 && in) {
            const int best = max(-1, max(a0, a1));
            const int buv = max(-1, max(a23, a3));
            int al = (3 * best + buv + 2) >> 2;
            al = 255 - al;
            al = al < 0 ? 0 : (al > 255 ? 255 : al);
            alpha[(size_t)f * nmb + mb] = (uint8_t)al;
            atomicAdd(&ahist[al], 1u);
        }
    }
    __syncthreads();
    const uint32_t c = ahist[threadIdx.x];
    if (c) atomicAdd(&histo[(size_t)f * 256 + threadIdx.x], c);
}

// ---------------------------------------------------------------------------
// Segments: one thread per frame.  k-means over the alpha histogram
// (assign_segments_kmeans analysis.rs:1029), per-segment quant via the
// reference's f64 fast_math pow (compute_segment_quant :1145; this file is
// built with -ffp-contract=off), matrices/lambdas (Segment::init_matrices
// types.rs:806), segment tree probabilities (vp8.rs:2340-2368).
// ---------------------------------------------------------------------------
__device__ double fm_log2(double x)
{
    unsigned long long bits = __double_as_longlong(x);
    long long e = (long long)((bits >> 52) & 0x7FF) - 1023;
    unsigned long long mb = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double m = __longlong_as_double((long long)mb);
    double y = (m - 1.0) / (m + 1.0);
    double y2 = y * y;
    const double C0 = 2.8853900817779268, C1 = 0.9617966939259756, C2 = 0.5770780163555854,
                 C3 = 0.4121985831111324, C4 = 0.3205988987531030;
    double poly = C0 + y2 * (C1 + y2 * (C2 + y2 * (C3 + y2 * C4)));
    return (double)e + y * poly;
}
__device__ double fm_exp2(double x)
{
    if (x < -1022.0) x = -1022.0;
    if (x > 1023.0) x = 1023.0;
    long long xi = x >= 0.0 ? (long long)x : (long long)x - 1;
    double xf = x - (double)xi;
    const double LN2 = 0.6931471805599453;
    const double C1 = LN2, C2 = LN2 * LN2 / 2.0, C3 = LN2 * LN2 * LN2 / 6.0, C4 = LN2 * LN2 * LN2 * LN2 / 24.0,
                 C5 = LN2 * LN2 * LN2 * LN2 * LN2 / 120.0;
    double poly = 1.0 + xf * (C1 + xf * (C2 + xf * (C3 + xf * (C4 + xf * C5))));
    double scale = __longlong_as_double((long long)((unsigned long long)(xi + 1023) << 52));
    return poly * scale;
}
__device__ double fm_pow(double x, double n)
{
    if (x <= 0.0) return 0.0;
    if (x == 1.0 || n == 0.0) return 1.0;
    if (n == 1.0) return x;
    return fm_exp2(n * fm_log2(x));
}
__device__ int segment_quant(int base, int alpha, int sns)
{
    double amp = 0.9 * (double)sns / 100.0 / 128.0;
    double expn = 1.0 - amp * (double)alpha;
    if (expn <= 0.0) return base;
    double cb = 1.0 - ((double)base / 127.0);
    double c = fm_pow(cb, expn);
    int q = (int)(127.0 * (1.0 - c));
    return q < 0 ? 0 : (q > 127 ? 127 : q);
}

__device__ void matrix_init(ZwMatrix& m, int qdc, int qac, int bdc, int bac)
{
    m.q[0] = (uint32_t)qdc;
    m.q[1] = (uint32_t)qac;
    for (int i = 0; i < 2; i++) {
        uint32_t b = i ? bac : bdc;
        m.iq[i] = (1u << 17) / m.q[i];
        m.bias[i] = ((b << 17) + 128) >> 8;
        m.zthresh[i] = ((1u << 17) - 1 - m.bias[i]) / m.iq[i];
    }
}

__device__ void segment_init(ZwSegment& s, int qi, int delta)
{
    int ydc = d_DC_QUANT[qi], yac = d_AC_QUANT[qi];
    int y2dc = d_DC_QUANT[qi] * 2;
    int y2ac = (int)d_AC_QUANT[qi] * 155 / 100;
    if (y2ac < 8) y2ac = 8;
    int uvdc = d_DC_QUANT[qi], uvac = d_AC_QUANT[qi];
    matrix_init(s.y1, ydc, yac, 96, 110);
    matrix_init(s.y2, y2dc, y2ac, 96, 108);
    matrix_init(s.uv, uvdc, uvac, 110, 115);
    for (int i = 0; i < 16; i++) {
        uint32_t q = i == 0 ? (uint32_t)ydc : (uint32_t)yac;
        s.sharpen[i] = (uint16_t)(((uint32_t)d_VP8_FREQ_SHARPENING[i] * q) >> 11);
    }
    uint32_t qi4 = ((uint32_t)ydc + 15u * (uint32_t)yac + 8) >> 4;
    uint32_t qi16 = ((uint32_t)y2dc + 15u * (uint32_t)y2ac + 8) >> 4;
    uint32_t quv = ((uint32_t)uvdc + 15u * (uint32_t)uvac + 8) >> 4;
#define MAX1(v) ((v) ? (v) : 1u)
    s.lt_i4 = MAX1((7 * qi4 * qi4) >> 3);
    s.lt_i16 = MAX1((qi16 * qi16) >> 2);
    s.lt_uv = MAX1((quv * quv) << 1);
    s.l_i4 = MAX1((3 * qi4 * qi4) >> 7);
    s.l_i16 = MAX1(3 * qi16 * qi16);
    s.l_uv = MAX1((3 * quv * quv) >> 6);
    s.l_mode = MAX1((qi4 * qi4) >> 7);
#undef MAX1
    s.tlambda = (50 * qi4) >> 5;
    s.quant_index = qi;
    s.quantizer_level = delta;
}

// Consumes the frame's alpha histogram and clears it for the next launch of
// k_analysis4 (zeroed once at pipeline creation; no per-launch memset blit).
extern "C" __global__ void k_segments(uint32_t* __restrict__ histo, const ZwFrameParams* __restrict__ tmpl,
                                      ZwFrameParams* __restrict__ params, int nframes)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    ZwFrameParams P = *tmpl;
    const int base = P.base_qi;
    const int nmb = P.mbw * P.mbh;
    for (int i = 0; i < 4; i++) segment_init(P.seg[i], base, 0);
    for (int i = 0; i < 256; i++) P.seg_map_lut[i] = 0;
    P.seg_probs[0] = P.seg_probs[1] = P.seg_probs[2] = 255;
    P.seg_enabled = 0;
    P.seg_update_map = 0;
    if (nmb >= 256) {
        const uint32_t* H = histo + (size_t)f * 256;
        uint8_t centers[4] = {0, 0, 0, 0};
        uint8_t* map = P.seg_map_lut;
        int min_a = 0, max_a = 255;
        for (int n = 0; n < 256; n++)
            if (H[n] > 0) { min_a = n; break; }
        for (int n = 255; n >= min_a; n--)
            if (H[n] > 0) { max_a = n; break; }
        int range = max_a > min_a ? max_a - min_a : 0;
        for (int k = 0; k < 4; k++) centers[k] = (uint8_t)(min_a + ((1 + 2 * k) * range) / 8);
        uint32_t accum[4], dacc[4];
        int wa = 0;
        uint32_t tw = 0;
        for (int it = 0; it < 6; it++) {
            for (int i = 0; i < 4; i++) accum[i] = dacc[i] = 0;
            int cc = 0;
            for (int a = min_a; a <= max_a; a++) {
                if (H[a] > 0) {
                    while (cc + 1 < 4) {
                        int dc = iabs(a - centers[cc]), dn = iabs(a - centers[cc + 1]);
                        if (dn < dc) cc++;
                        else break;
                    }
                    map[a] = (uint8_t)cc;
                    dacc[cc] += (uint32_t)a * H[a];
                    accum[cc] += H[a];
                }
            }
            int displaced = 0;
            wa = 0;
            tw = 0;
            for (int n = 0; n < 4; n++) {
                if (accum[n] > 0) {
                    uint8_t nc = (uint8_t)((dacc[n] + accum[n] / 2) / accum[n]);
                    displaced += iabs(centers[n] - nc);
                    centers[n] = nc;
                    wa += (int)nc * (int)accum[n];
                    tw += accum[n];
                }
            }
            if (displaced < 5) break;
        }
        int mid = tw > 0 ? (wa + (int)tw / 2) / (int)tw : 128;
        int minc = centers[0], maxc = centers[0];
        for (int i = 1; i < 4; i++) {
            minc = min(minc, (int)centers[i]);
            maxc = max(maxc, (int)centers[i]);
        }
        int rng = maxc == minc ? 1 : maxc - minc;
        for (int s = 0; s < 4; s++) {
            int ta = 255 * ((int)centers[s] - mid) / rng;
            ta = ta < -127 ? -127 : (ta > 127 ? 127 : ta);
            int sq = segment_quant(base, ta, 50);
            int delta = (int)(int8_t)((int8_t)sq - (int8_t)base);
            segment_init(P.seg[s], sq, delta);
        }
        uint32_t cnt[4] = {0, 0, 0, 0};
        for (int a = 0; a < 256; a++) cnt[map[a]] += H[a];
        uint32_t t01 = cnt[0] + cnt[1], t23 = cnt[2] + cnt[3];
#define GETP(a, b) ((a) + (b) == 0 ? 255 : (uint8_t)((255 * (a) + ((a) + (b)) / 2) / ((a) + (b))))
        P.seg_probs[0] = GETP(t01, t23);
        P.seg_probs[1] = GETP(cnt[0], cnt[1]);
        P.seg_probs[2] = GETP(cnt[2], cnt[3]);
#undef GETP
        P.seg_update_map = P.seg_probs[0] != 255 || P.seg_probs[1] != 255 || P.seg_probs[2] != 255;
        P.seg_enabled = 1;
    }
    params[f] = P;
    uint4* Hz = (uint4*)(histo + (size_t)f * 256);
    for (int i = 0; i < 64; i++) Hz[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------------------
// Host-side launch wrappers (called from zw_host.cpp).
// ---------------------------------------------------------------------------
extern "C" hipError_t zwk_rgb2yuv(hipStream_t s, const uint8_t* img, int w, int h, int bpp, int mbw, int mbh,
                                  uint8_t* Y, uint8_t* U, uint8_t* V, size_t img_stride, size_t ysz, size_t csz,
                                  int nframes)
{
    // the row-coalesced kernel needs every 8-pixel run aligned for its loads
    // (16 B for RGBA, 8 B for RGB) and 8-byte aligned luma rows
    const uintptr_t base = (uintptr_t)img;
    const bool planes_ok = ((uintptr_t)Y | (uintptr_t)U | (uintptr_t)V | ysz | csz) % 8 == 0;
    const int ng = mbw * 2 * mbh * 8;
    if (planes_ok && bpp == 4 && base % 16 == 0 && img_stride % 16 == 0 && w % 4 == 0) {
        hipLaunchKernelGGL(k_rgb2yuv_rows<4>, dim3((ng + 255) / 256, nframes), dim3(256), 0, s, img, w, h, mbw, mbh,
                           Y, U, V, img_stride, ysz, csz);
    } else if (planes_ok && bpp == 3 && base % 8 == 0 && img_stride % 8 == 0 && w % 8 == 0) {
        hipLaunchKernelGGL(k_rgb2yuv_rows<3>, dim3((ng + 255) / 256, nframes), dim3(256), 0, s, img, w, h, mbw, mbh,
                           Y, U, V, img_stride, ysz, csz);
    } else {
        const int n = mbw * 8 * mbh * 8;
        hipLaunchKernelGGL(k_rgb2yuv, dim3((n + 255) / 256, nframes), dim3(256), 0, s, img, w, h, bpp, mbw, mbh, Y, U,
                           V, img_stride, ysz, csz);
    }
    return hipGetLastError();
}

extern "C" hipError_t zwk_analysis(hipStream_t s, const uint8_t* Y, const uint8_t* U, const uint8_t* V, int mbw,
                                   int mbh, size_t ysz, size_t csz, uint8_t* alpha, uint32_t* histo, int nframes)
{
    const int nmb = mbw * mbh;
    hipLaunchKernelGGL(k_analysis4, dim3((nmb + 16 * ZW_AN4_GPW - 1) / (16 * ZW_AN4_GPW), nframes), dim3(256), 0, s, Y, U,
                       V, mbw, mbh, ysz, csz, alpha, histo);
    return hipGetLastError();
}

extern "C" hipError_t zwk_segments(hipStream_t s, uint32_t* histo, const ZwFrameParams* tmpl,
                                   ZwFrameParams* params, int nframes)
{
    hipLaunchKernelGGL(k_segments, dim3((nframes + 63) / 64), dim3(64), 0, s, histo, tmpl, params, nframes);
    return hipGetLastError();
}
