// zw_enc_kernels.hip -- the encode pass of the lossy encoder (gfx950).
//
//   k_encode_*    one encode pass over a batch of frames:   (vp8.rs:1281-1488)
//                 RD mode search (pick_best_intra16/intra4/uv), final transform,
//                 quantization (simple or trellis), recon, error diffusion, skip.
//
// (The conversion, analysis and segment kernels that run before it are in
// zw_prepass_kernels.hip, the block quantiser kernels in zw_quant_kernels.hip.)
//
// Parallel structure: one workgroup per frame, NW waves.  Macroblock rows are
// dealt to waves round-robin and advance as an x+2y wavefront (a row may work
// on MB x once the row above has finished MB x+1), synchronised through LDS
// progress counters.  Within a macroblock the 64 lanes work block-parallel.
// Pass 1's chroma is a raster chain (left_derr is not reset per row, quirk A5)
// and runs on wave 0 while waves 1..NW-1 do the luma wavefront.
#include "zw_dev.h"

#include <type_traits>

#include "zw_enc_rows.h"
#include "zw_enc_pairfinal.h"
#include "zw_enc_i4pair.h"

// Phase counters of the profiling build (tools/phase_prof.py names them).
#define ZW_PH_N 28

// ---------------------------------------------------------------------------
// Compile-time knobs (make exp EXPDEFS="-DZW_...=..."), each with the
// measurement that set its default.  The row schedule's (ZW_P1_ORDER,
// ZW_P1_SLOWSKIP, ZW_P1_SLOW_NUM / _DEN; in frame pairs ZW_P1P_SLOW_NUM / _DEN,
// ZW_P1P_JOIN_NUM / _DEN / _MIN) are in zw_enc_rows.h.
// ---------------------------------------------------------------------------
// Waves per workgroup of each encode pass.  Both kernels stay within 168
// VGPRs, so three waves share each SIMD (12 per CU); ZW_NW sets both.
#ifdef ZW_NW
#define ZW_NW1 ZW_NW
#define ZW_NW2 ZW_NW
#endif
#ifndef ZW_NW1
#define ZW_NW1 12
#endif
#ifndef ZW_NW2
#define ZW_NW2 12
#endif
#define NW_MAX (ZW_NW1 > ZW_NW2 ? ZW_NW1 : ZW_NW2)
// Issue priority of a luma wave from its slack to the row above
// (luma_issue_prio): slack (MBs) per priority level, 0: off; pass 1's level
// width and cap.
#ifndef ZW_DYN_PRIO
#define ZW_DYN_PRIO 1
#endif
#ifndef ZW_DYN_PRIO1
#define ZW_DYN_PRIO1 2  // (1: 28.86, 2: 28.74 ms per 256 1080p frames, one-frame kernel)
#endif
#ifndef ZW_P1_LUMA_MAX
#define ZW_P1_LUMA_MAX 3  // (2 kept the luma waves below the chroma chain: 0.7 % slower)
#endif                    // (frame pairs with the chain waves joining, 512 1080p frames: 3 46.13-46.26, 2 46.23-46.30 ms)
// The chroma chain is pass 1's critical path: it takes issue priority over the
// luma waves sharing its SIMD (measured: 47.6 -> 44.3 ms per 256 1080p frames
// against luma-first priority at 12 waves).  Pass 1's luma waves start below
// it: the chain sets the pass's length once 11 waves share the luma wavefront.
// (Frame pairs, where the chain waves take luma rows after their chains, 512
// 1080p frames, join at 5/8 and slow share 2/1: priority 3 46.13-46.26, 2
// 46.14-46.25 ms: no difference.)
#ifndef ZW_CHAIN_PRIO
#define ZW_CHAIN_PRIO 3
#endif
#ifndef ZW_LUMA_PRIO
#define ZW_LUMA_PRIO 0
#endif

template <int PASS> struct PassShape {
    static constexpr int NW = PASS == 1 ? ZW_NW1 : ZW_NW2;
    static constexpr int WG = NW * 64;
};

// ---------------------------------------------------------------------------
// The encode pass.
// ---------------------------------------------------------------------------
struct EncArgs {
    const uint8_t *Y, *U, *V;
    const uint8_t* alpha;       // per MB (segment lookup)
    const ZwFrameParams* params;
    const ZwLevelCosts* lcost;  // per frame; null in pass 1 (all-zero tables, quirk A2)
    int8_t* derr;               // [nframes][mbw][4] top_derr: pass 1 writes, pass 2 reads
    ZwMbOut* out;
    uint8_t *ry, *ru, *rv;      // reconstruction (pass 2), may be null
    size_t ysz, csz;
    int mbw, mbh, pass;
    int* dbg;                   // optional pass-2 I4 dump (16*34 ints per MB), may be null
    uint8_t* rows;              // row-parallel kernels: zero-filled ZW_ROWS_HDR + nframes * RowsLayout::frame
    uint32_t* sizes;            // pass 2, may be null: per MB its packed record size (zw_pack_kernels.hip)
    int nframes;                // frames of the launch (the frame-pair kernel's last workgroup may hold one)
};

// Per-MB LDS state: what lives from an MB's first search to its stores (the
// staged source, the luma work buffer with the I4 search's reconstruction, the
// levels and sub-modes) and the MB row's left contexts.  A wave working two
// rows at once (the paired kernels) keeps one per row.
struct MbLds {
    uint8_t sy[256], su[64], sv[64];  // source MB (staged per MB)
    uint8_t ws[17 * ZW_BPS];      // luma work buffer (create_border_luma layout)
    uint8_t left_y[20], left_u[12], left_v[12], left_c[12];
    int8_t left_derr[4];
    uint8_t modes[16];
    int16_t lev[25][16];
};

// per-wave LDS scratch
struct WaveLds {
    MbLds mb;                     // the wave's (first) row
    uint8_t cu[9 * ZW_BPS], cv[9 * ZW_BPS];
    uint32_t uvc[64][8];          // pick_uv -> final_chroma, per lane: its coefficients (i16 pairs) + rows' pred
    int dc[64];
    int y2d[64];
    int y2cost[4];
    int V[2][40];                 // I4 value vectors of the (up to) two sub-blocks of a search step
    int nzt[4], nzl[4];
    int misc[16];
    uint32_t pst[2][4];           // paired kernels: per MB {lm | need << 4 | seg << 8, i16 score lo, hi, i4 nz | win << 16};
                                  // after the searches [1] = final chroma's result | cm << 9, [2] = final luma's result
    // row-parallel kernels: this MB's slice of the row above's state (top_y of
    // the MB and of the MB above-right, top_u/v, top_c, top_derr), pulled from
    // and pushed to global memory around each MB
    uint8_t win_y[32], win_u[8], win_v[8], win_c[12];
    int8_t win_d[4];
#ifdef ZW_PHASE_PROF
    unsigned long long ph[ZW_PH_N];
#endif
};


struct Ctx {
    const EncArgs* a;
    const ZwFrameParams* P;
    int method;           // EncoderParams method (wave-uniform, read once)
    const ZwSegment* S;   // the MB's segment, in LDS
    const ZwSegment* Sl;  // the frame's 4 segments, in LDS
    const LdsTables* T;
    WaveLds* W;
    MbLds* M;             // the MB's per-row state (&W->mb, or the paired row's)
    uint8_t *top_y, *top_u, *top_v, *top_c;
    int8_t* top_derr;
    const uint8_t *srcY, *srcU, *srcV;  // MB origin (HBM)
    const uint8_t *sY, *sU, *sV;        // the same MB staged in LDS (strides 16 / 8)
    int ys, cs;
    int mbx, mby, lane, seg;
    int f;                  // frame of the launch
    int oy, oc, ocx, od;    // offsets of this MB in top_y / top_u,v / top_c / top_derr
                            // (mbx*16, *8, *12, *4; 0 in the row-parallel kernels, whose
                            // top_* point at the wave's per-MB window)
};

// create_border_luma (prediction.rs:15) into C.M->ws
// part 0: corner, top and left (everything the I16 search reads: available once
// the MB above is done); part 1: the top-right pixels (row 0 columns 17..31 and
// their copies at rows 4, 8, 12; the I4 search needs the MB above-right);
// part 2: both.
__device__ void build_luma_border(const Ctx& C, int part = 2)
{
    uint8_t* ws = C.M->ws;
    const int l = C.lane;
    const int mbw = C.a->mbw;
    const bool want = part == 2 || (part == 0 ? (l < 17 || l >= 32) : (l >= 17 && l < 32));
    // row 0 entries 0..31
    if (!want) {
    } else if (l < 32) {
        int v;
        if (l == 0) v = C.mby == 0 ? 127 : (C.mbx == 0 ? 129 : C.M->left_y[0]);
        else if (C.mby == 0) v = 127;
        else if (l <= 16) v = C.top_y[C.oy + l - 1];
        else if (C.mbx == mbw - 1) v = C.top_y[C.oy + 15];
        else v = C.top_y[C.oy + l - 1];
        ws[l] = (uint8_t)v;
        if (l >= 17 && l < 21) {
            ws[4 * ZW_BPS + l] = (uint8_t)v;
            ws[8 * ZW_BPS + l] = (uint8_t)v;
            ws[12 * ZW_BPS + l] = (uint8_t)v;
        }
    } else if (l < 48) {
        int i = l - 32;
        ws[(i + 1) * ZW_BPS] = C.mbx == 0 ? 129 : C.M->left_y[1 + i];
    }
    wsync();
}

// create_border_chroma (prediction.rs:85) into cu / cv
__device__ void build_chroma_border(const Ctx& C)
{
    const int l = C.lane;
    if (l < 34) {  // per plane: corner, 8 top, 8 left
        const int pl = l >= 17;
        const int i = pl ? l - 17 : l;
        uint8_t* w = pl ? C.W->cv : C.W->cu;
        const uint8_t* top = pl ? C.top_v : C.top_u;
        const uint8_t* left = pl ? C.M->left_v : C.M->left_u;
        if (i == 0) w[0] = C.mby == 0 ? 127 : (C.mbx == 0 ? 129 : left[0]);
        else if (i <= 8) w[i] = C.mby == 0 ? 127 : top[C.oc + i - 1];
        else w[(i - 8) * ZW_BPS] = C.mbx == 0 ? 129 : left[i - 8];
    }
    wsync();
}

// pick_best_intra16 (vp8.rs:1504-1687).  lane = mode*16 + block.
template <int PASS>
__device__ void pick_i16(const Ctx& C, int& best_mode, unsigned long long& best_score)
{
    const int lane = C.lane, m = lane >> 4, b = lane & 15, bx = b & 3, by = b >> 2;
    const uint8_t* ws = C.M->ws;
    const ZwSegment& S = *C.S;
    const LdsTables* T = C.T;
    const int above = C.mby != 0, left = C.mbx != 0;
    int dcv;
    {  // DC predictor: lanes 0..15 top row, 16..31 left column
        const int top = lane < 16;
        const int v = (int)ws[csel(top, 1 + b, (b + 1) * ZW_BPS)] & -(int)(lane < 32 && (top ? above : left));
        const int sum = red16(v);
        const int s = __builtin_amdgcn_readlane(sum, 0) + __builtin_amdgcn_readlane(sum, 16);
        const int shf = 3 + above + left;
        dcv = (!above && !left) ? 128 : ((s + (1 << (shf - 1))) >> shf);
    }
    int src[16], pr[16], r[16], c[16];
    {
        const int P0 = ws[0];
        int L[4], Tp[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            L[i] = ws[(by * 4 + i + 1) * ZW_BPS];
            Tp[i] = ws[1 + bx * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t srow = *(const uint32_t*)(C.sY + (by * 4 + i) * 16 + bx * 4);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int p = sel4(m, dcv, Tp[j], L[i], clamp255(L[i] + Tp[j] - P0));
                const int sv = (int)((srow >> (8 * j)) & 255u);
                src[i * 4 + j] = sv;
                pr[i * 4 + j] = p;
                r[i * 4 + j] = sv - p;
            }
        }
    }
    fdct16_pk(r, c);
    int aq[16], dq[16];
    aq[0] = 0;
    int nzac = 0;
#pragma unroll
    for (int k = 1; k < 16; k++) {
        aq[k] = (int)((__umul24((uint32_t)iabs(c[k]), S.y1.iq[1]) + S.y1.bias[1]) >> 17);
        nzac |= aq[k];
        dq[k] = m24(c[k] < 0 ? -aq[k] : aq[k], (int)S.y1.q[1]);
    }
    nzac = nzac != 0;
    int cost = (int)rcost_bf<1, PASS == 2>(aq, 0, 0, T);
    // Y2 in group form: lane (m, b) holds block b's DC under mode m
    int y2cost;
    {
        const int d = wht_g(c[0], b);
        const int t = b > 0;
        const int ay = (int)((__umul24((uint32_t)iabs(d), S.y2.iq[t]) + S.y2.bias[t]) >> 17);
        const int qy = d < 0 ? -ay : ay;
        y2cost = (int)rcost_g<0, PASS == 2>(qy, b, 0, 1, T);  // uniform within the mode's group
        dq[0] = iwht_g(m24(qy, (int)S.y2.q[t]), b);
    }
    idct16(dq);
    int rec[16], sse = 0, flat = 1;
    const int s00 = C.sY[0];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        rec[k] = clamp255(pr[k] + dq[k]);
        const int d = src[k] - rec[k];
        sse += m24(d, d);
        flat &= src[k] == s00;
    }
    int td = iabs(ttransform_diff_pk(rec, src)) >> 5;
    sse = red16(sse);
    td = red16(td);
    cost = red16(cost);
    nzac = red16(nzac);
    flat = red16(flat);
    // per mode (uniform within the 16-lane group), decided on the scalar unit
    const int srcflat = __builtin_amdgcn_readlane(flat, 0) == 16;  // mode-0 group covers all 256 pixels
    cost += y2cost;
    int sd = S.tlambda > 0 ? ((int)S.tlambda * td + 128) >> 8 : 0;
    int dfin = sse;
    if (srcflat && nzac == 0) {
        dfin = sse * 2;
        sd = sd * 2;
    }
    const int mcost = sel4(m, d_FIXED_COSTS_I16[0], d_FIXED_COSTS_I16[1], d_FIXED_COSTS_I16[2], d_FIXED_COSTS_I16[3]) + cost;
    const int dist = dfin + sd;
    long long brd = 0x7fffffffffffffffLL, bfin = 0;
    int bm = 0;
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        const long long mc = __builtin_amdgcn_readlane(mcost, mm * 16);
        const long long dd = 256LL * __builtin_amdgcn_readlane(dist, mm * 16);
        const long long r_m = mc * (long long)S.l_i16 + dd;
        const long long f_m = mc * (long long)S.l_mode + dd;
        const int avail = mm == 0 || (mm == 1 && above) || (mm == 2 && left) || (mm == 3 && above && left);
        if (avail && r_m < brd) {
            brd = r_m;
            bfin = f_m;
            bm = mm;
        }
    }
    best_mode = bm;
    best_score = bfin < 0 ? 0ull : (unsigned long long)bfin;
}

#ifdef ZW_PHASE_PROF
// Per-phase cycle counters (profiling builds only): [pass-1][phase].
__device__ unsigned long long zw_phase_cycles_dev[2][ZW_PH_N];
__device__ unsigned long long zw_wave_cycles_dev[2][16][ZW_PH_N];  // the same per wave index
#define PH_START() long long ph_t_ = clock64()
#define PH_RESET() (ph_t_ = clock64())
#define PH_MARK(k) PH_MARK_L(k, lane, PASS)
// accumulate in the wave's LDS slot; flushed once per kernel (ph_flush)
#define PH_MARK_L(k, ln, ps)                                                        \
    do {                                                                            \
        const long long n_ = clock64();                                             \
        if ((ln) == 0) C.W->ph[k] += (unsigned long long)(n_ - ph_t_);               \
        ph_t_ = n_;                                                                 \
    } while (0)
extern "C" int zw_wave_cycles(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zw_wave_cycles_dev), sizeof(zw_wave_cycles_dev)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long z[2][16][ZW_PH_N];
        if (hipMemcpyToSymbol(HIP_SYMBOL(zw_wave_cycles_dev), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
extern "C" int zw_phase_cycles(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zw_phase_cycles_dev), sizeof(zw_phase_cycles_dev)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long z[2][ZW_PH_N];
        if (hipMemcpyToSymbol(HIP_SYMBOL(zw_phase_cycles_dev), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define PH_COUNT(k) \
    do {                \
        if (C.lane == 0) C.W->ph[k] += 1; \
    } while (0)
#else
#define PH_COUNT(k) (void)0
#define PH_START() (void)0
#define PH_RESET() (void)0
#define PH_MARK(k) (void)0
#define PH_MARK_L(k, ln, ps) (void)0
#endif

// Fill the I4 value vectors V[h] for the NB sub-blocks (x0[h], y0[h]) of
// C.M->ws (branch-free: every lane reads up to three edge pixels and forms an
// avg2/avg3/copy; the lane -> (edge indices, weights) map is block invariant).
//   V[0..12]  E = [L3 L2 L1 L0 P A0..A7]      V[13..23] avg3(E[k], E[k+1], E[k+2])
//   V[24..35] avg2(E[k], E[k+1])              V[36] avg3(A6,A7,A7)  V[37] avg3(L2,L3,L3)
//   V[38] DC = (4 + L0..L3 + A0..A3) >> 3
template <int NB>
__device__ __forceinline__ void i4_values_n(const Ctx& C, const int* x0, const int* y0)
{
    WaveLds* W = C.W;
    const uint8_t* ws = C.M->ws;
    const int l = C.lane;
    // lane -> (ka, kb, kc) and weights; t: 0 copy, 1 avg3, 2 avg2, 3/4 special avg3
    // (arithmetic only: lane-dependent selects must not become branches)
    const int t = (int)(l >= 13) + (int)(l >= 24) + (int)(l >= 36) + (int)(l >= 37);
    const int k = min(l - 13 * (int)(l >= 13) - 11 * (int)(l >= 24), 12);
    const int t3 = (int)(t == 3), t4 = (int)(t >= 4), t12 = (int)(t == 1 || t == 2);
    const int ka = k + t3 * (11 - k) + t4 * (1 - k);
    const int kb = k + t12 + t3 * (12 - k) - t4 * k;
    const int kc = min(k + 2 * (int)(t == 1), 12);
    // v = (ea + wb*eb + wc*ec + rnd) >> sh
    const int wb = 2 * (int)(t == 1) + (int)(t == 2) + 3 * (t3 + t4);
    const int wc = (int)(t == 1);
    const int sh = (int)(t != 0) + (int)(t != 0 && t != 2);
    const int oa = csel(ka < 4, -ka * ZW_BPS, ka - 4 - 4 * ZW_BPS);  // offsets from rowL = (y0+3)*BPS + x0-1
    const int ob = csel(kb < 4, -kb * ZW_BPS, kb - 4 - 4 * ZW_BPS);
    const int oc = csel(kc < 4, -kc * ZW_BPS, kc - 4 - 4 * ZW_BPS);
    const bool dcl = l < 4 || (l >= 5 && l < 9);
    int v[NB], ea[NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        const int rowL = (y0[h] + 3) * ZW_BPS + x0[h] - 1;
        ea[h] = ws[rowL + oa];
        const int eb = ws[rowL + ob], ec = ws[rowL + oc];
        v[h] = (ea[h] + wb * eb + wc * ec + ((1 << sh) >> 1)) >> sh;
    }
#pragma unroll
    for (int h = 0; h < NB; h++) {
        const int dsum = red16(dcl ? ea[h] : 0);
        if (l < 38) W->V[h][l] = v[h];
        if (l == 0) W->V[h][38] = (dsum + 4) >> 3;
    }
    wsync();
}
__device__ __forceinline__ void i4_values(const Ctx& C, int x0, int y0) { i4_values_n<1>(C, &x0, &y0); }

__device__ __forceinline__ int bperm(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }

// V index of pixel p under I4 mode `mode`, with bit 8 set for TrueMotion
// (pred = clamp(V[ia] + V[5 + col] - V[4])).  Sub-block independent.
__device__ __forceinline__ int i4_src_index(const LdsTables* T, int mode, int p)
{
    // (TrueMotion is mode 1, the only row of d_I4_IDX that holds 254; i4qa is 4 x the index)
    return (T->i4qa[mode][p] >> 2) + csel(mode == 1, 256, 0);
}
__device__ __forceinline__ int i4_pred_at(const int* V, int sidx, int vbc)
{
    const int va = V[sidx & 255];
    return csel(sidx >= 256, clamp255(va + vbc), va);
}

__device__ __forceinline__ unsigned long long rdscore(uint32_t sse, uint32_t rate, uint32_t lambda)
{
    return (unsigned long long)sse * 256ull + (unsigned long long)(uint16_t)rate * lambda;
}

// Running state of the I4 search (pick_best_intra4, vp8.rs:1790-2040).
struct I4State {
    unsigned long long running;  // sum of the chosen blocks' rd scores (+ 211 * lambda_mode)
    uint32_t total_mc;           // header-bit cap accumulator (vp8.rs:1839)
    unsigned long long mpack;    // chosen sub-modes, 4 bits each (raster index)
    uint32_t tnz, lnz;           // nonzero flags of the chosen blocks: bit sbx / bit sby
    uint32_t nzm;                // nonzero flags of the chosen blocks: bit = raster index
};

// Unsigned minimum within aligned 16-lane rows (DPP row rotations), in every lane.
DI uint32_t min16u(uint32_t v)
{
    v = min(v, (uint32_t)DPP((int)v, 0x128));
    v = min(v, (uint32_t)DPP((int)v, 0x124));
    v = min(v, (uint32_t)DPP((int)v, 0x122));
    v = min(v, (uint32_t)DPP((int)v, 0x121));
    return v;
}

// ---------------------------------------------------------------------------
// Chroma in lane-pair form.  A 4x4 chroma block is worked by two lanes, l and
// l ^ 32 (half h = l >> 5): the pixel rows 2h, 2h+1 for prediction, residual,
// the fDCT row pass, the iDCT row pass and the reconstruction, the coefficient
// columns 2h, 2h+1 for the fDCT column pass, quantisation, rate and the iDCT
// column pass.  The halves trade intermediate values with v_permlane32_swap
// (four swaps per transform), so each lane does half of a block's arithmetic
// and the search over 4 modes x 8 blocks fills all 64 lanes.  Pixel rows are
// held as i16 pairs (x0, x1), (x3, x2) (the fdct16_pk layout).
// ---------------------------------------------------------------------------
// Both halves' copies of v: r[0] holds the lower half's value in every lane of
// the upper half, r[1] the upper half's in every lane of the lower half.
__device__ __forceinline__ int hx_partner(int v)
{
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (__lane_id() < 32) ? (int)r[1] : (int)r[0];
}
__device__ __forceinline__ int hx_sum(int v)  // v(l) + v(l ^ 32), in both lanes
{
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (int)r[0] + (int)r[1];
}
DI int lo16(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
DI int hi16(uint32_t v) { return (int)(int16_t)(v >> 16); }

// The lane's two pixel rows of chroma block (bx, by) under 8x8 mode m (0 DC,
// 1 V, 2 H, 3 TM; predict_dcpred / vpred / hpred / tmpred): pred(i, j) =
// clamp(rowv(i) + colv(j)) with (rowv, colv) = (dc, 0) / (0, T[j]) / (L[i], 0)
// / (L[i] - P, T[j]); source and prediction as i16 pairs.
DI void uv_rows_pk(const uint8_t* w, const uint8_t* sblk, int bx, int by, int h, int m, int dc, uint32_t s01[2],
                   uint32_t s32[2], uint32_t p01[2], uint32_t p32[2])
{
    const int cm = -(int)(m & 1), rm = -(int)(m >= 2);
    const int P = w[0];
    const int ro = csel(m == 0, dc, csel(m == 3, -P, 0));
    const uint8_t* tp = w + 1 + bx * 4;
    const uint32_t c01 = pack_lo(tp[0] & cm, tp[1] & cm), c32 = pack_lo(tp[3] & cm, tp[2] & cm);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int y = 2 * h + r;
        const int rv = (w[(by * 4 + y + 1) * ZW_BPS] & rm) + ro;
        const uint32_t rvv = pack_lo(rv, rv);
        p01[r] = clamp_pk(add_pk(c01, rvv));
        p32[r] = clamp_pk(add_pk(c32, rvv));
        const uint32_t sw = *(const uint32_t*)(sblk + y * 8);
        s01[r] = __builtin_amdgcn_perm(0u, sw, 0x0c010c00u);
        s32[r] = __builtin_amdgcn_perm(0u, sw, 0x0c020c03u);
    }
}

// dct4x4 (transform.rs:176) of the pair's block: this lane's coefficients of
// columns 2h, 2h+1, cf[col][row] = coefficient (row, 2h + col).
DI void fdct_pair(const uint32_t s01[2], const uint32_t s32[2], const uint32_t p01[2], const uint32_t p32[2], int h,
                  int cf[2][4])
{
    // row pass (fdct16_pk first stage), outputs of this lane's columns (own*)
    // and of the partner's columns (oth*)
    const zs2 k8p = {8, 8}, k8m = {8, -8}, k1a = {10704, 4434}, k1b = {4434, -10704};
    const uint32_t kA0 = h ? as_zu(k8m) : as_zu(k8p), kA1 = h ? as_zu(k8p) : as_zu(k8m);
    const uint32_t kD0 = h ? as_zu(k1b) : as_zu(k1a), kD1 = h ? as_zu(k1a) : as_zu(k1b);
    const int rD0 = h ? 1875 : 3625, rD1 = h ? 3625 : 1875;
    int own0[2], own1[2], oth0[2], oth1[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t R01 = sub_pk(s01[r], p01[r]), R32 = sub_pk(s32[r], p32[r]);
        const uint32_t A = add_pk(R01, R32), D = sub_pk(R01, R32);
        own0[r] = dot2v(A, kA0, 0);
        oth0[r] = dot2v(A, kA1, 0);
        own1[r] = dot2v(D, kD0, rD0) >> 10;
        oth1[r] = dot2v(D, kD1, rD1) >> 10;
    }
    // the partner's rows of this lane's columns
    const uint32_t g0 = (uint32_t)hx_partner((int)pack_lo(oth0[0], oth0[1]));
    const uint32_t g1 = (uint32_t)hx_partner((int)pack_lo(oth1[0], oth1[1]));
    const zs2 k1p = {1, 1}, k1m = {1, -1}, k2a = {5352, 2217}, k2b = {2217, -5352};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int* ow = c ? own1 : own0;
        const uint32_t g = c ? g1 : g0;
        // column = rows (0, 1) and (3, 2): own rows are 2h, 2h+1, the partner's the others
        const uint32_t fwd = pack_lo(ow[0], ow[1]), rev = pack_lo(ow[1], ow[0]);
        const uint32_t grev = __builtin_amdgcn_alignbit(g, g, 16);
        const uint32_t X01 = h ? g : fwd, X32 = h ? rev : grev;
        const zs2 A = as_zs2(X01) + as_zs2(X32), D = as_zs2(X01) - as_zs2(X32);
        cf[c][0] = dot2(A, k1p, 7) >> 4;
        cf[c][2] = dot2(A, k1m, 7) >> 4;
        cf[c][1] = (dot2(D, k2a, 12000) >> 16) + ((as_zu(D) & 0xffffu) != 0u ? 1 : 0);
        cf[c][3] = dot2(D, k2b, 51000) >> 16;
    }
}

// idct4x4 (transform.rs:19, i32 form of idct16) of the pair's dequantised
// coefficients dq[col][row] (columns 2h, 2h+1), then the reconstruction
// clamp(pred + residual) of this lane's two rows as i16 pairs (x0,x1),(x3,x2).
DI void idct_recon_pair(const int dq[2][4], const uint32_t p01[2], const uint32_t p32[2], int h, uint32_t r01[2],
                        uint32_t r32[2])
{
    uint32_t lo[2], hi[2];  // vertical pass of this lane's columns: rows (0,1), (2,3)
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int x0 = dq[c][0], x1 = dq[c][1], x2 = dq[c][2], x3 = dq[c][3];
        const int a1 = x0 + x2, b1 = x0 - x2;
        const int c1 = (m24(x1, 35468) >> 16) - (x3 + (m24(x3, 20091) >> 16));
        const int d1 = (x1 + (m24(x1, 20091) >> 16)) + (m24(x3, 35468) >> 16);
        lo[c] = pack_lo(a1 + d1, b1 + c1);
        hi[c] = pack_lo(b1 - c1, a1 - d1);
    }
    // the partner needs these columns at its rows, this lane the partner's columns at its own
    const uint32_t g0 = (uint32_t)hx_partner((int)(h ? lo[0] : hi[0]));
    const uint32_t g1 = (uint32_t)hx_partner((int)(h ? lo[1] : hi[1]));
    const uint32_t m0 = h ? hi[0] : lo[0], m1 = h ? hi[1] : lo[1];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        // values of row 2h + r at columns 0..3
        const int e0 = r ? hi16(m0) : lo16(m0), e1 = r ? hi16(m1) : lo16(m1);
        const int f0 = r ? hi16(g0) : lo16(g0), f1 = r ? hi16(g1) : lo16(g1);
        const int y0 = h ? f0 : e0, y1 = h ? f1 : e1, y2 = h ? e0 : f0, y3 = h ? e1 : f1;
        const int a1 = y0 + y2, b1 = y0 - y2;
        const int c1 = (m24(y1, 35468) >> 16) - (y3 + (m24(y3, 20091) >> 16));
        const int d1 = (y1 + (m24(y1, 20091) >> 16)) + (m24(y3, 35468) >> 16);
        const int o0 = (a1 + d1 + 4) >> 3, o1 = (b1 + c1 + 4) >> 3, o2 = (b1 - c1 + 4) >> 3, o3 = (a1 - d1 + 4) >> 3;
        r01[r] = clamp_pk(add_pk(pack_lo(o0, o1), p01[r]));
        r32[r] = clamp_pk(add_pk(pack_lo(o3, o2), p32[r]));
    }
}

// get_residual_cost (cost.rs:1670, quirk A1: positions are natural indices) of
// a lane pair's block, first position 0: av[col][row] = |level| at natural
// index n = 4 row + 2h + col.  Returns the block's rate in 1/256 bits, uniform
// in the pair.  LC = false: the LevelCosts tables are zero (pass 1, quirk A2)
// and lfc[0] == 0, so positions past the last nonzero level add nothing.
template <bool LC>
DI int rcost_pair(const int av[2][4], int h, int ctx0, int ctype, const LdsTables* T, int& last_o)
{
    unsigned nzbits = 0, big = 0;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int n = 4 * r + 2 * h + c;
            nzbits |= (unsigned)min(av[c][r], 1) << n;
            big |= (unsigned)(av[c][r] >= 2) << n;
        }
    nzbits |= (unsigned)hx_partner((int)nzbits);
    big |= (unsigned)hx_partner((int)big);
    const int last = 31 - __clz((int)nzbits);
    last_o = last;
    int part = 0;
    if (LC) {
        // predecessor contexts from the partner's second column (2(1-h)+1), 2 bits per row
        unsigned sc = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) sc |= (unsigned)min(av[1][r], 2) << (2 * r);
        const unsigned rc = (unsigned)hx_partner((int)sc);
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = 4 * r + 2 * h + c;
                int ctx;
                if (c == 1) ctx = min(av[0][r], 2);
                else if (r == 0) ctx = h ? (int)(rc & 3u) : ctx0;  // n = 2: column 1 of row 0; n = 0: ctx0
                else ctx = h ? (int)((rc >> (2 * r)) & 3u) : (int)((rc >> (2 * r - 2)) & 3u);
                const int a = av[c][r];
                const int tl = T->lfc[min(a, 2047)] + T->lc[ctype][band_of(n)][ctx][min(a, 67)];
                part += tl & -(int)(n <= last);
            }
    } else {
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) part += T->lfc[min(av[c][r], 2047)];
    }
    const int sum = hx_sum(part);
    const int ctx_t = ((big >> max(last, 0)) & 1u) ? 2 : 1;
    const int tail = (int)T->beob[ctype][band_of(min(last + 1, 15))][ctx_t] & -(int)(last < 15);
    const int head = (int)T->binit[ctype][0][ctx0] & -(int)(ctx0 == 0);
    return csel(last < 0, (int)T->beob[ctype][0][ctx0], head + sum + tail);  // (no divergent branch)
}

// Chroma DC predictors of both planes (uniform values): lanes 0..15 sum U,
// 16..31 V; lane i < 8 reads left pixel i, i >= 8 top pixel i - 8.
__device__ __forceinline__ void uv_dc_preds(const Ctx& C, int& dcU, int& dcV)
{
    const int l = C.lane, pl = (l >> 4) & 1, i = l & 15;
    const uint8_t* w = pl ? C.W->cv : C.W->cu;
    const int above = C.mby != 0, left = C.mbx != 0;
    const int v = (int)w[csel(i < 8, (i + 1) * ZW_BPS, i - 7)] & -(int)(i < 8 ? left : above);
    const int sum = red16(v);
    const int su = __builtin_amdgcn_readlane(sum, 0), sv = __builtin_amdgcn_readlane(sum, 16);
    const int shf = 2 + left + above;
    dcU = (above | left) ? (su + (1 << (shf - 1))) >> shf : 128;
    dcV = (above | left) ? (sv + (1 << (shf - 1))) >> shf : 128;
}

// pick_best_uv (vp8.rs:2050-2200): lane pair (l, l ^ 32) = mode * 8 + block
// (U blocks 0..3, V 4..7).  Each lane leaves its coefficients (i16 pairs) and
// its rows' prediction in W->uvc[lane], so final_chroma starts from the chosen
// mode's transform instead of recomputing it.
template <int PASS>
__device__ int pick_uv(const Ctx& C)
{
    const ZwSegment& S = *C.S;
    const LdsTables* T = C.T;
    WaveLds* W = C.W;
    const int l = C.lane;
    const int above = C.mby != 0, left = C.mbx != 0;
    int dcU, dcV;
    uv_dc_preds(C, dcU, dcV);
    const int h = l >> 5, q = l & 31, m = q >> 3, b = q & 7;
    const int pl = b >> 2, bx = b & 1, by = (b >> 1) & 1;
    uint32_t s01[2], s32[2], p01[2], p32[2];
    uv_rows_pk(pl ? W->cv : W->cu, (pl ? C.sV : C.sU) + by * 32 + bx * 4, bx, by, h, m, pl ? dcV : dcU, s01, s32, p01,
               p32);
    int cf[2][4];
    fdct_pair(s01, s32, p01, p32, h, cf);
    {
        uint32_t* e = W->uvc[l];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            e[2 * c] = pack_lo(cf[c][0], cf[c][1]);
            e[2 * c + 1] = pack_lo(cf[c][2], cf[c][3]);
        }
        e[4] = p01[0];
        e[5] = p32[0];
        e[6] = p01[1];
        e[7] = p32[1];
    }
    // quantize_coeff (no sharpening, cost.rs:457); natural index n = 4 row + 2h + col
    int dq[2][4], av[2][4];
    int nzac = 0;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool dcs = c == 0 && r == 0;  // natural index 2h: the DC when h == 0
            const int t = dcs ? (int)(h != 0) : 1;
            const uint32_t iq = dcs ? (h ? S.uv.iq[1] : S.uv.iq[0]) : S.uv.iq[1];
            const uint32_t bias = dcs ? (h ? S.uv.bias[1] : S.uv.bias[0]) : S.uv.bias[1];
            const int q_ = dcs ? (int)(h ? S.uv.q[1] : S.uv.q[0]) : (int)S.uv.q[1];
            const int v = cf[c][r];
            const int a = (int)((__umul24((uint32_t)iabs(v), iq) + bias) >> 17);
            av[c][r] = a;
            dq[c][r] = m24(v < 0 ? -a : a, q_);
            nzac += t ? min(a, 1) : 0;
        }
    // get_residual_cost (cost.rs:1670), ctype 2, first 0, ctx0 0
    int last_;
    int cost = rcost_pair<PASS == 2>(av, h, 0, 2, T, last_);
    // reconstruction and SSE of this lane's rows
    uint32_t r01[2], r32[2];
    idct_recon_pair(dq, p01, p32, h, r01, r32);
    int sse = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t d01 = sub_pk(s01[r], r01[r]), d32 = sub_pk(s32[r], r32[r]);
        sse = dot2v(d01, d01, sse);
        sse = dot2v(d32, d32, sse);
    }
    sse = red8(hx_sum(sse));
    cost = red8(cost);
    nzac = red8(hx_sum(nzac));
    const int fixed = sel4(m, d_FIXED_COSTS_UV[0], d_FIXED_COSTS_UV[1], d_FIXED_COSTS_UV[2], d_FIXED_COSTS_UV[3]);
    const int pen = (m > 0 && nzac <= 2) ? 140 * 8 : 0;
    const int csum = fixed + cost + pen;
    // per-mode RD on the scalar unit: rd = (fixed + cost + pen) * lambda_uv + 256 * sse
    long long brd = 0x7fffffffffffffffLL;
    int bm = 0;
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        const long long r_m = (long long)__builtin_amdgcn_readlane(csum, mm * 8) * (long long)S.l_uv +
                              256LL * (long long)__builtin_amdgcn_readlane(sse, mm * 8);
        const int avail = mm == 0 || (mm == 1 && above) || (mm == 2 && left) || (mm == 3 && above && left);
        if (avail && r_m < brd) {
            brd = r_m;
            bm = mm;
        }
    }
    return bm;
}

// ---------------------------------------------------------------------------
// I4 search (pick_best_intra4, vp8.rs:1790-2040) in lane-pair form.
// Sub-blocks are visited along x+2y anti-diagonals (10 steps, 6 of them with
// two independent blocks).  One step evaluates ALL ten modes of both blocks at
// once: lane l = 32 hf + 16 slot + mode (modes 10..15 idle), the pair (l,
// l ^ 32) working one (block, mode) in the chroma pair layout (rows 2hf,
// 2hf+1 / columns 2hf, 2hf+1).  The reference's candidate set -- the K modes
// of smallest prediction SSE, in that order (K = 3 / 4 / 10 by method) -- is
// applied afterwards as an eligibility mask: the chosen mode is the eligible
// one of smallest RD score, ties to the smaller (sse, mode) key, which is the
// reference's first strict minimum in candidate order.  The full RD of the
// non-candidates costs nothing extra (the lanes would idle) and the ranking no
// longer sits in front of the transforms.
// ---------------------------------------------------------------------------
// Per-lane constants of the search (fixed for an MB).
struct I4Lane {
    uint32_t ia, ib;  // bperm byte addresses (4 x V index) of the lane's pixels in rows 2hf, 2hf+1, one per byte
    uint32_t psel;    // v_perm selector taking the lane's slot half of two gathered words
    int tm;           // mode is TrueMotion
};

// Value vectors of the step's (up to) two sub-blocks, slot 0 in the low and
// slot 1 in the high 16 bits: lane v < 39 holds V[v] (see i4_values_n).
template <int NB>
__device__ __forceinline__ uint32_t i4_values_pk(const Ctx& C, const int* x0, const int* y0)
{
    const uint8_t* ws = C.M->ws;
    const int l = C.lane;
    const int t = (int)(l >= 13) + (int)(l >= 24) + (int)(l >= 36) + (int)(l >= 37);
    const int k = min(l - 13 * (int)(l >= 13) - 11 * (int)(l >= 24), 12);
    const int t3 = (int)(t == 3), t4 = (int)(t >= 4), t12 = (int)(t == 1 || t == 2);
    const int ka = k + t3 * (11 - k) + t4 * (1 - k);
    const int kb = k + t12 + t3 * (12 - k) - t4 * k;
    const int kc = min(k + 2 * (int)(t == 1), 12);
    const int wb = 2 * (int)(t == 1) + (int)(t == 2) + 3 * (t3 + t4);
    const int wc = (int)(t == 1);
    const int sh = (int)(t != 0) + (int)(t != 0 && t != 2);
    const int oa = csel(ka < 4, -ka * ZW_BPS, ka - 4 - 4 * ZW_BPS);
    const int ob = csel(kb < 4, -kb * ZW_BPS, kb - 4 - 4 * ZW_BPS);
    const int oc = csel(kc < 4, -kc * ZW_BPS, kc - 4 - 4 * ZW_BPS);
    const bool dcl = l < 4 || (l >= 5 && l < 9);
    uint32_t v = 0, ea = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int hh = NB == 2 ? h : 0;
        const int rowL = (y0[hh] + 3) * ZW_BPS + x0[hh] - 1;
        const int a = ws[rowL + oa], eb = ws[rowL + ob], ec = ws[rowL + oc];
        v |= (uint32_t)((a + wb * eb + wc * ec + ((1 << sh) >> 1)) >> sh) << (16 * h);
        ea |= (uint32_t)a << (16 * h);
    }
    // DC = (4 + L0..L3 + A0..A3) >> 3 of both slots at once (sums < 2^16)
    const uint32_t ds = (uint32_t)__builtin_amdgcn_readfirstlane(red16((int)(dcl ? ea : 0u)));
    const uint32_t dcv = (((ds & 0xffffu) + 4) >> 3) | ((((ds >> 16) + 4) >> 3) << 16);
    return l == 38 ? dcv : v;
}

DI void i4_lane_init(const Ctx& C, I4Lane& L)
{
    const int l = C.lane, hf = l >> 5, m = l & 15, mv = m < 10 ? m : 0;
    L.ia = L.ib = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int sa = i4_src_index(C.T, mv, 8 * hf + j) & 255, sb = i4_src_index(C.T, mv, 8 * hf + 4 + j) & 255;
        L.ia |= (uint32_t)(4 * sa) << (8 * j);
        L.ib |= (uint32_t)(4 * sb) << (8 * j);
    }
    L.psel = (l & 16) ? 0x0c060c02u : 0x0c040c00u;
    L.tm = mv == 1;
}

DI int quad_or(int v)
{
    v |= DPP(v, 0xB1);
    return v | DPP(v, 0x4E);
}
DI int quad_sum(int v)
{
    v += DPP(v, 0xB1);
    return v + DPP(v, 0x4E);
}

// get_residual_cost (cost.rs:1670, quirk A1) of a quad's block, first position
// 0: lane q holds column q, av[r] = |level| at natural index n = 4 r + q.
// Uniform in the quad.  LC = false: pass 1 (zero LevelCosts, quirk A2).
template <bool LC>
DI int rcost_quad(const int av[4], int q, int ctx0, int ctype, const LdsTables* T, int& last_o, int head_none[2])
{
    unsigned nz = 0, big = 0, sc = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int n = 4 * r + q;
        nz |= (unsigned)min(av[r], 1) << n;
        big |= (unsigned)(av[r] >= 2) << n;
        sc |= (unsigned)min(av[r], 2) << (2 * r);
    }
    // every table read of the block issued before any is used (one LDS round
    // trip): the level costs, then the end-of-block cost at last + 1
    int tl[4];
    if (LC) {
        // the context of position n is min(|level[n - 1]|, 2): lane q - 1 of the
        // same row, for q = 0 lane 3 of the row above (ctx0 at n = 0)
        const unsigned pv = (unsigned)DPP((int)sc, 0x93);  // quad_perm [3, 0, 1, 2]
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int n = 4 * r + q;
            const int c_same = (int)((pv >> (2 * r)) & 3u);
            const int c_q0 = r == 0 ? ctx0 : (int)((pv >> (2 * r - 2)) & 3u);
            const int ctx = csel(q == 0, c_q0, c_same);
            const int a = av[r];
            tl[r] = T->lfc[min(a, 2047)] + T->lc[ctype][band_of(n)][ctx][min(a, 67)];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) tl[r] = T->lfc[min(av[r], 2047)];
    }
    nz = (unsigned)quad_or((int)nz);
    big = (unsigned)quad_or((int)big);
    const int last = 31 - __clz((int)nz);
    last_o = last;
    const int ctx_t = ((big >> max(last, 0)) & 1u) ? 2 : 1;
    const int tail = (int)T->beob[ctype][band_of(min(last + 1, 15))][ctx_t] & -(int)(last < 15);
    int part = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) part += LC ? tl[r] & -(int)(4 * r + q <= last) : tl[r];
    const int sum = quad_sum(part);
    return csel(last < 0, head_none[1], head_none[0] + sum + tail);  // (no divergent branch)
}

// rank = #{lanes of the 16-lane row with a smaller key}: per rotation the
// borrow of a DPP subtraction (keys are in [0, 2^31), so the borrow is
// rot(key) < key) into VCC, then an add-with-carry
DI int rank16(int key)
{
    int rank = 0, scratch_;
#define ZW_RANK_STEP(R) "v_sub_co_u32_dpp %1, vcc, %2, %2 row_ror:" #R " row_mask:0xf bank_mask:0xf\n" \
                        "v_addc_co_u32_e32 %0, vcc, 0, %0, vcc\n"
    asm volatile("s_nop 1\n" ZW_RANK_STEP(1) ZW_RANK_STEP(2) ZW_RANK_STEP(3) ZW_RANK_STEP(4) ZW_RANK_STEP(5)
                     ZW_RANK_STEP(6) ZW_RANK_STEP(7) ZW_RANK_STEP(8) ZW_RANK_STEP(9) ZW_RANK_STEP(10)
                         ZW_RANK_STEP(11) ZW_RANK_STEP(12) ZW_RANK_STEP(13) ZW_RANK_STEP(14) ZW_RANK_STEP(15)
                 : "+v"(rank), "=&v"(scratch_)
                 : "v"(key)
                 : "vcc");
#undef ZW_RANK_STEP
    return rank;
}

// Candidate evaluation of an I4 step in quad form (K <= 4: methods 0-4).  The
// step's candidate set -- the K modes of smallest prediction SSE per block,
// `rank` from the pair layout -- is evaluated with four lanes per (block,
// candidate): lane = 16 slot + 4 k + q, q = pixel row / coefficient column,
// k = the candidate's rank.  A lane does a quarter of a block's arithmetic
// (the quad transforms of the chroma chain), and only the K candidates are
// transformed instead of all ten modes.  The winner is the smallest (score,
// rank) of each slot's row: the reference's first strict minimum over its
// candidates in SSE order.
template <int PASS, int NB>
DI void i4_cand_quad(const Ctx& C, const int* sbx, const int* sby, const int* x0, const int* y0, const int* tctx,
                     const int* lctx, const int* nzc, int K, int rank, uint32_t vp, uint32_t ap01, uint32_t ap32,
                     I4State& st, bool keep)
{
    PH_START();
    const ZwSegment& S = *C.S;
    const LdsTables* T = C.T;
    const int l = C.lane, m = l & 15, hf = l >> 5;
    // candidate modes: k-th of each slot from the pair layout's ranks (lane
    // 16 slot + mode of the lower half), four bits each, slot 1 at bit 16
    uint32_t modes = 0;
    for (int k = 0; k < K; k++) {
        const unsigned long long b = __ballot(hf == 0 && m < 10 && rank == k);
        const uint32_t lo = (uint32_t)b & 0xffffu, hi = ((uint32_t)b >> 16) & 0xffffu;
        modes |= (uint32_t)__builtin_ctz(lo | 0x10000u) << (4 * k);
        if (NB == 2) modes |= (uint32_t)__builtin_ctz(hi | 0x10000u) << (16 + 4 * k);
    }
    const int slot = NB == 2 ? (l >> 4) & 1 : 0, k = (l >> 2) & 3, q = l & 3;
    const int mq = (int)((modes >> (16 * slot + 4 * k)) & 15u);
    const int mv = k < K ? mq : 0;  // (k >= K: a valid mode, never eligible)
    const int sl = NB == 2 ? 1 : 0;
    const int bx = csel(slot, sbx[sl], sbx[0]), by = csel(slot, sby[sl], sby[0]);
    const int ctx0 = csel(slot, nzc[sl], nzc[0]);
    const int mcost = T->fci4[csel(slot, tctx[sl], tctx[0])][csel(slot, lctx[sl], lctx[0])][mv];
    // read up front, off the transform's chain: the quantiser of this lane's
    // coefficients and the block's costs that depend only on ctx0 (the first
    // coefficient's "more tokens" bit, and the empty block's end of block)
    const uint32_t iq0 = q ? S.y1.iq[1] : S.y1.iq[0], bs0 = q ? S.y1.bias[1] : S.y1.bias[0];
    const uint32_t iq1 = S.y1.iq[1], bs1 = S.y1.bias[1];
    const int q0 = q ? (int)S.y1.q[1] : (int)S.y1.q[0], qa = (int)S.y1.q[1];
    int hn[2];
    hn[0] = (int)T->binit[3][0][ctx0] & -(int)(ctx0 == 0);
    hn[1] = (int)T->beob[3][0][ctx0];
    // prediction of row q: V indices of its four pixels (254: TrueMotion,
    // V[3 - q] + the top offsets; 255: the DC entry V[38])
    uint32_t p01, p32;
    {
        // bpermute byte addresses of the row's four pixels (T->i4qa: 4 x V index)
        const uint32_t iw = *(const uint32_t*)&T->i4qa[mv][4 * q];
        const uint32_t psel = (l & 16) ? 0x0c060c02u : 0x0c040c00u;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[j] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((iw >> (8 * j)) & 255u), (int)vp);
        const uint32_t q01 = __builtin_amdgcn_perm(v[1], v[0], psel), q32 = __builtin_amdgcn_perm(v[2], v[3], psel);
        const bool tm = mv == 1;
        p01 = tm ? clamp_pk(add_pk(q01, ap01)) : q01;
        p32 = tm ? clamp_pk(add_pk(q32, ap32)) : q32;
    }
    uint32_t s01, s32;
    {
        const uint32_t sw = *(const uint32_t*)(C.sY + (by * 4 + q) * 16 + bx * 4);
        s01 = __builtin_amdgcn_perm(0u, sw, 0x0c010c00u);
        s32 = __builtin_amdgcn_perm(0u, sw, 0x0c020c03u);
    }
    PH_MARK_L(22, l, 0);
    const uint32_t R01 = sub_pk(s01, p01), R32 = sub_pk(s32, p32);
    int cf[4];
    uvq_fdct(add_pk(R01, R32), sub_pk(R01, R32), q, cf);
    int av[4], dq[4], lv[4];
    {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool dcs = r == 0;  // (0, q): the DC for q = 0
            const int v = cf[r];
            const int a = (int)((__umul24((uint32_t)iabs(v), dcs ? iq0 : iq1) + (dcs ? bs0 : bs1)) >> 17);
            av[r] = a;
            lv[r] = v < 0 ? -a : a;
            dq[r] = m24(lv[r], dcs ? q0 : qa);
        }
    }
    int last;
    const int cost = rcost_quad<PASS == 2>(av, q, ctx0, 3, T, last, hn);  // get_cost_luma4 (ctype 3, first 0)
    PH_MARK_L(23, l, 0);
    uint32_t r01, r32;
    uvq_idct_recon(dq, p01, p32, q, r01, r32);
    int sse = 0;
    {
        const uint32_t d01 = sub_pk(s01, r01), d32 = sub_pk(s32, r32);
        sse = dot2v(d01, d01, sse);
        sse = dot2v(d32, d32, sse);
    }
    sse = quad_sum(sse);
    const uint32_t rate = (uint32_t)(mcost + cost);
    // rd_score (cost.rs): sse * 256 + u16(rate) * lambda_i4 < 2^29
    const uint32_t score = (uint32_t)sse * 256u + (rate & 0xffffu) * S.l_i4;
    const uint32_t key2 = k < K ? (score << 2) | (uint32_t)k : 0xffffffffu;
    const uint32_t kmin = min16u(key2);
    const unsigned long long win = __ballot(key2 == kmin);
    PH_MARK_L(12, l, 0);
    int bk[NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        bk[h] = __builtin_ctz((uint32_t)(win >> (16 * h)) & 0xffffu) >> 2;
        const int bmode = (int)((modes >> (16 * h + 4 * bk[h])) & 15u);
        const int wl = 16 * h + 4 * bk[h];
        const uint32_t bsse = (uint32_t)__builtin_amdgcn_readlane(sse, wl);
        const uint32_t brate = (uint32_t)__builtin_amdgcn_readlane((int)rate, wl);
        const int bnz = __builtin_amdgcn_readlane((int)(last >= 0), wl);
        const int i = sby[h] * 4 + sbx[h];
        st.tnz = (st.tnz & ~(1u << sbx[h])) | ((uint32_t)bnz << sbx[h]);
        st.lnz = (st.lnz & ~(1u << sby[h])) | ((uint32_t)bnz << sby[h]);
        st.nzm |= (uint32_t)bnz << i;
        // the winner's mode cost is its lane's mcost (= fci4[tctx][lctx][bmode]): no LDS round trip on the step chain
        st.total_mc += (uint32_t)__builtin_amdgcn_readlane(mcost, wl);
        st.running += rdscore(bsse, brate, S.l_mode);
        st.mpack |= (unsigned long long)bmode << (4 * i);
        if (l == h) C.M->modes[i] = (uint8_t)bmode;
    }
    // the winners' quads write their rows of the reconstruction (and, when the
    // final pass reuses them, their columns of levels in zigzag order)
    const int bks = csel(slot, bk[sl], bk[0]);
    if (k == bks && l < 16 * NB) {
        const int xo = csel(slot, x0[sl], x0[0]), yo = csel(slot, y0[sl], y0[0]);
        const uint32_t wd = __builtin_amdgcn_perm(r32, r01, 0x04060200u);
        uint8_t* p = C.M->ws + (yo + q) * ZW_BPS + xo;
#pragma unroll
        for (int j = 0; j < 4; j++) p[j] = (uint8_t)(wd >> (8 * j));
        if (keep) {
            int16_t* lvp = C.M->lev[by * 4 + bx];
#pragma unroll
            for (int r = 0; r < 4; r++) lvp[izz_of(4 * r + q)] = (int16_t)lv[r];
        }
    }
    wsync();
    PH_MARK_L(13, l, 0);
}

template <int PASS, int NB>
__device__ __forceinline__ void i4_step(const Ctx& C, const int* sbx, const int* sby, int K, const I4Lane& LC,
                                        I4State& st, bool keep)
{
    const ZwSegment& S = *C.S;
    const LdsTables* T = C.T;
    const int l = C.lane, hf = l >> 5, m = l & 15;
    const int slot = NB == 2 ? (l >> 4) & 1 : 0;
    int x0[NB], y0[NB], tctx[NB], lctx[NB], nzc[NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        const int i = sby[h] * 4 + sbx[h];
        x0[h] = sbx[h] * 4 + 1;
        y0[h] = sby[h] * 4 + 1;
        tctx[h] = sby[h] == 0 ? 0 : (int)((st.mpack >> (4 * (i - 4))) & 15);
        lctx[h] = sbx[h] == 0 ? 0 : (int)((st.mpack >> (4 * (i - 1))) & 15);
        nzc[h] = (sby[h] == 0 ? 0 : (int)((st.tnz >> sbx[h]) & 1)) + (sbx[h] == 0 ? 0 : (int)((st.lnz >> sby[h]) & 1));
    }
    const int sl = NB == 2 ? 1 : 0;
    const int bx = csel(slot, sbx[sl], sbx[0]), by = csel(slot, sby[sl], sby[0]);
    const int ctx0 = csel(slot, nzc[sl], nzc[0]);
    const int mcost = T->fci4[csel(slot, tctx[sl], tctx[0])][csel(slot, lctx[sl], lctx[0])][m < 10 ? m : 0];
    PH_START();
    const uint32_t vp = i4_values_pk<NB>(C, x0, y0);
    PH_MARK_L(10, l, 0);
    // TrueMotion offsets V[5 + j] - V[4] of both slots, as (x0, x1), (x3, x2) pairs
    uint32_t ap01, ap32;
    {
        const uint32_t P = (uint32_t)__builtin_amdgcn_readlane((int)vp, 4);
        uint32_t a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) a[j] = (uint32_t)__builtin_amdgcn_readlane((int)vp, 5 + j);
        const int sh = 16 * slot;
        const int p_ = (int)((P >> sh) & 255u);
        const int d0 = (int)((a[0] >> sh) & 255u) - p_, d1 = (int)((a[1] >> sh) & 255u) - p_;
        const int d2 = (int)((a[2] >> sh) & 255u) - p_, d3 = (int)((a[3] >> sh) & 255u) - p_;
        ap01 = pack_lo(d0, d1);
        ap32 = pack_lo(d3, d2);
    }
    // this lane's predictions (rows 2hf, 2hf+1) gathered from the value vectors
    uint32_t p01[2], p32[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t ix = r ? LC.ib : LC.ia;
        const uint32_t v0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ix & 255u), (int)vp);
        const uint32_t v1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ix >> 8) & 255u), (int)vp);
        const uint32_t v2 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ix >> 16) & 255u), (int)vp);
        const uint32_t v3 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ix >> 24), (int)vp);
        const uint32_t q01 = __builtin_amdgcn_perm(v1, v0, LC.psel), q32 = __builtin_amdgcn_perm(v2, v3, LC.psel);
        p01[r] = LC.tm ? clamp_pk(add_pk(q01, ap01)) : q01;
        p32[r] = LC.tm ? clamp_pk(add_pk(q32, ap32)) : q32;
    }
    // source rows
    uint32_t s01[2], s32[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t sw = *(const uint32_t*)(C.sY + (by * 4 + 2 * hf + r) * 16 + bx * 4);
        s01[r] = __builtin_amdgcn_perm(0u, sw, 0x0c010c00u);
        s32[r] = __builtin_amdgcn_perm(0u, sw, 0x0c020c03u);
    }
    // prediction SSE and the candidate set: rank of key = sse * 16 + mode among
    // the slot's ten modes (the reference's stable ascending sort, quirk A12)
    int pse = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t d01 = sub_pk(s01[r], p01[r]), d32 = sub_pk(s32[r], p32[r]);
        pse = dot2v(d01, d01, pse);
        pse = dot2v(d32, d32, pse);
    }
    pse = hx_sum(pse);
    const int key = m < 10 ? (pse << 4) | m : 0x7fffffff;
    const int rank = rank16(key);
    PH_MARK_L(11, l, 0);
    if (K <= 4) {
        i4_cand_quad<PASS, NB>(C, sbx, sby, x0, y0, tctx, lctx, nzc, K, rank, vp, ap01, ap32, st, keep);
        return;
    }
    // transform, quantiser, rate, reconstruction and distortion of every
    // (block, mode): natural coefficient index n = 4 row + 2 hf + col, the DC
    // (n = 0) in the lower half's column 0
    int cf[2][4];
    fdct_pair(s01, s32, p01, p32, hf, cf);
    int av[2][4], dq[2][4];
    unsigned sgn = 0;
    {
        const uint32_t iq0 = hf ? S.y1.iq[1] : S.y1.iq[0], bs0 = hf ? S.y1.bias[1] : S.y1.bias[0];
        const int q0 = hf ? (int)S.y1.q[1] : (int)S.y1.q[0];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool dcs = c == 0 && r == 0;
                const int v = cf[c][r];
                const int a = (int)((__umul24((uint32_t)iabs(v), dcs ? iq0 : S.y1.iq[1]) + (dcs ? bs0 : S.y1.bias[1])) >> 17);
                av[c][r] = a;
                dq[c][r] = m24(v < 0 ? -a : a, dcs ? q0 : (int)S.y1.q[1]);
                sgn |= (unsigned)(v < 0) << (4 * c + r);
            }
    }
    int last;
    const int cost = rcost_pair<PASS == 2>(av, hf, ctx0, 3, T, last);  // get_cost_luma4 (ctype 3, first 0)
    uint32_t r01[2], r32[2];
    idct_recon_pair(dq, p01, p32, hf, r01, r32);
    int sse = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t d01 = sub_pk(s01[r], r01[r]), d32 = sub_pk(s32[r], r32[r]);
        sse = dot2v(d01, d01, sse);
        sse = dot2v(d32, d32, sse);
    }
    sse = hx_sum(sse);
    const uint32_t rate = (uint32_t)(mcost + cost);
    // rd_score (cost.rs): sse * 256 + u16(rate) * lambda_i4 < 2^29 (see above)
    const uint32_t score = (uint32_t)sse * 256u + (rate & 0xffffu) * S.l_i4;
    const bool elig = m < 10 && rank < K;
    // the eligible lane of smallest (score, rank) in each slot's row: the
    // reference's first strict minimum over its candidates in SSE order
    // (DPP reads other lanes: every min16u runs with the whole wave active)
    const uint32_t sk = elig ? score : 0xffffffffu;
    const uint32_t smin = min16u(sk);
    const uint32_t rk = sk == smin ? (uint32_t)rank : 0xffffffffu;
    const uint32_t rmin = min16u(rk);
    const unsigned long long win = __ballot(rk == rmin && sk == smin);
    PH_MARK_L(12, l, 0);
    int bmode[NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        bmode[h] = __builtin_ctz((uint32_t)(win >> (16 * h)) & 0xffffu);
        const int wl = 16 * h + bmode[h];
        const uint32_t bsse = (uint32_t)__builtin_amdgcn_readlane(sse, wl);
        const uint32_t brate = (uint32_t)__builtin_amdgcn_readlane((int)rate, wl);
        const int bnz = __builtin_amdgcn_readlane((int)(last >= 0), wl);
        const int i = sby[h] * 4 + sbx[h];
        st.tnz = (st.tnz & ~(1u << sbx[h])) | ((uint32_t)bnz << sbx[h]);
        st.lnz = (st.lnz & ~(1u << sby[h])) | ((uint32_t)bnz << sby[h]);
        st.nzm |= (uint32_t)bnz << i;
        st.total_mc += (uint32_t)__builtin_amdgcn_readlane(mcost, wl);  // (lane wl's mode is bmode[h])
        st.running += rdscore(bsse, brate, S.l_mode);
        st.mpack |= (unsigned long long)bmode[h] << (4 * i);
        if (l == h) C.M->modes[i] = (uint8_t)bmode[h];
    }
    // the winners' two lanes write their rows of the reconstruction (and, when
    // the final pass reuses them, the levels in zigzag order)
    const int bms = csel(slot, bmode[sl], bmode[0]);
    if (m == bms && (NB == 2 || slot == 0)) {
        const int xo = csel(slot, x0[sl], x0[0]), yo = csel(slot, y0[sl], y0[0]);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t wd = __builtin_amdgcn_perm(r32[r], r01[r], 0x04060200u);
            uint8_t* p = C.M->ws + (yo + 2 * hf + r) * ZW_BPS + xo;
#pragma unroll
            for (int j = 0; j < 4; j++) p[j] = (uint8_t)(wd >> (8 * j));
        }
        if (keep) {
            int16_t* lv = C.M->lev[by * 4 + bx];
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int a = av[c][r];
                    lv[izz_of(4 * r + 2 * hf + c)] = (int16_t)(((sgn >> (4 * c + r)) & 1u) ? -a : a);
                }
        }
    }
    wsync();
    PH_MARK_L(13, l, 0);
}

// pick_best_intra4 (vp8.rs:1790-2040).  Returns true when I4 wins; modes in C.M->modes.
// Each block's choice depends only on its left / top / top-right neighbours,
// which every earlier anti-diagonal holds, so every choice equals the
// raster-order one.  The reference's early exits (running score >= the I16
// score, vp8.rs:2018; mode cost cap, :1839) test sums of non-negative terms,
// which grow with every block: "some raster prefix crossed the bound" is "the
// sum over every block crossed it", so testing the sum of the blocks searched
// so far after each step decides exactly as the reference does.
template <int PASS>
__device__ bool pick_i4(const Ctx& C, unsigned long long i16_score, bool keep, uint32_t& nzm)
{
    const ZwSegment& S = *C.S;
    const int K = C.method <= 3 ? 3 : (C.method == 4 ? 4 : 10);
    I4State st;
    st.running = 211ull * S.l_mode;
    st.total_mc = 0;
    st.mpack = 0;
    st.tnz = st.lnz = st.nzm = 0;
    I4Lane LC;
    i4_lane_init(C, LC);
    PH_COUNT(20);
    for (int s = 0; s < 10; s++) {
        PH_COUNT(19);
        // anti-diagonal s: A = (sbx, sby) with the smallest sby, B = (sbx - 2, sby + 1)
        const int sbyA = s < 4 ? 0 : (s - 2) >> 1;
        const int sbxA = s - 2 * sbyA;
        if (s >= 2 && s <= 7) {
            const int bx[2] = {sbxA, sbxA - 2}, by[2] = {sbyA, sbyA + 1};
            i4_step<PASS, 2>(C, bx, by, K, LC, st, keep);
        } else {
            i4_step<PASS, 1>(C, &sbxA, &sbyA, K, LC, st, keep);
        }
        if (st.running >= i16_score) return false;
        if (st.total_mc > 256u * 16u * 16u / 4u) return false;
    }
    nzm = st.nzm;
    return true;
}

// ---------------------------------------------------------------------------
// Paired I4 search: one wave searches the MBs of two rows at once.  The paired
// kernels give a wave two MB rows, y and y + 1, the second two columns behind
// (the x + 2y wavefront's lag), so MB A = (x, y) and MB B = (x - 2, y + 1) reach
// their I4 searches together; both visit the same anti-diagonal steps.  Lanes
// 0..31 work A and lanes 32..63 work B (hm = lane >> 5): the candidate phase
// keeps the quad form (lane = 32 hm + 16 slot + 4 k + q), the ranking works
// all four rows of a (slot, mode) in one lane (lane = 32 hm + 16 slot + mode).
// The value vectors of the four (MB, slot) blocks are packed one byte each
// (byte 2 hm + slot) in lanes 0..54: every prediction of every mode is a plain
// read of an entry, TrueMotion's sixteen clamped sums included (lanes 39..54),
// and the ranking orders the modes by byte dot products of the packed rows
// (zw_enc_i4pair.h).  Every per-MB decision (winners, early
// exits, running scores) is the single search's, per MB: a search that ends
// early leaves its lanes computing on, with their stores masked.
// A step stays in the lanes from its values to the next step's contexts
// (zw_enc_i4pair.h): the candidate modes come from a forward permute of the
// ranks' inverse, every lane of an MB holds its MB's running state and takes
// the step's winners into it, and only the two early exits are tested on the
// scalar side, once per step.
// ---------------------------------------------------------------------------
struct I4PLane {
    uint32_t ix[4];  // bperm byte addresses (4 x V index) of the lane's pixels in rows 0..3, one per byte
    uint32_t psel;   // v_perm selector taking the lane's (MB, slot) byte of two gathered words
#if ZW_I4P_DOT4 && ZW_I4P_TMV
    uint32_t bsel;   // ... to bytes 0 and 1 (the ranking's packed rows)
#endif
#if !ZW_I4P_TMV
    int tm;          // mode is TrueMotion
#endif
    // the candidate step's quantiser of the lane's coefficient column q (its MB's
    // segment, fixed for the search): read once instead of every step
    uint32_t iq0, bs0, iq1, bs1;
    int q0, qa;
    uint32_t l_i4;
};

DI void i4p_lane_init(const Ctx& C, const Ctx& CB, I4PLane& L)
{
    const int l = C.lane, m = l & 15, mv = m < 10 ? m : 0;
    {
        const ZwSegment* Sh = (l >> 5) ? CB.S : C.S;
        const int q = l & 3;
        L.iq0 = q ? Sh->y1.iq[1] : Sh->y1.iq[0];
        L.bs0 = q ? Sh->y1.bias[1] : Sh->y1.bias[0];
        L.iq1 = Sh->y1.iq[1];
        L.bs1 = Sh->y1.bias[1];
        L.q0 = q ? (int)Sh->y1.q[1] : (int)Sh->y1.q[0];
        L.qa = (int)Sh->y1.q[1];
        L.l_i4 = Sh->l_i4;
    }
    // (the static tables of both frames are alike)
#pragma unroll
    for (int r = 0; r < 4; r++) L.ix[r] = *(const uint32_t*)&C.T->i4qp[mv][4 * r];
    L.psel = i4p_psel(l >> 5, (l >> 4) & 1);
#if ZW_I4P_DOT4 && ZW_I4P_TMV
    L.bsel = i4p_bsel(l >> 5, (l >> 4) & 1);
#endif
#if !ZW_I4P_TMV
    L.tm = mv == 1;
#endif
}

// Value vectors (zw_enc_i4pair.h) of both MBs' step blocks: lane v < ZW_I4P_NV
// holds V[v] of (A slot 0, A slot 1, B slot 0, B slot 1) in bytes 0..3.
template <int NB>
DI uint32_t i4p_values(const Ctx& CA, const Ctx& CB, const int* x0, const int* y0)
{
    const int l = CA.lane;
    const I4PValue vm = i4p_value_map(l);
    const int oa = csel(vm.ka < 4, -vm.ka * ZW_BPS, vm.ka - 4 - 4 * ZW_BPS);
    const int ob = csel(vm.kb < 4, -vm.kb * ZW_BPS, vm.kb - 4 - 4 * ZW_BPS);
    const int oc = csel(vm.kc < 4, -vm.kc * ZW_BPS, vm.kc - 4 - 4 * ZW_BPS);
    const bool dcl = i4p_value_dc_term(l);
    uint32_t v[2], ea[2];
#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
        const uint8_t* ws = (mb ? CB : CA).M->ws;
        v[mb] = ea[mb] = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int hh = NB == 2 ? h : 0;
            const int rowL = (y0[hh] + 3) * ZW_BPS + x0[hh] - 1;
            const int a = ws[rowL + oa], eb = ws[rowL + ob], ec = ws[rowL + oc];
            v[mb] |= (uint32_t)i4p_value(vm, a, eb, ec) << (16 * h);
            ea[mb] |= (uint32_t)a << (16 * h);
        }
    }
    // the DCs of the four blocks (sums < 2^16 per slot)
    const uint32_t da = (uint32_t)__builtin_amdgcn_readfirstlane(red16((int)(dcl ? ea[0] : 0u)));
    const uint32_t db = (uint32_t)__builtin_amdgcn_readfirstlane(red16((int)(dcl ? ea[1] : 0u)));
    const uint32_t dcv = (((da & 0xffffu) + 4) >> 3) | ((((da >> 16) + 4) >> 3) << 8) |
                         ((((db & 0xffffu) + 4) >> 3) << 16) | ((((db >> 16) + 4) >> 3) << 24);
    return l == ZW_I4P_V_DC ? dcv : __builtin_amdgcn_perm(v[1], v[0], 0x06040200u);
}

// The running state of a paired search: in lane form every lane holds its MB's
// (zw_enc_i4pair.h); in scalar form (ZW_I4P_LANES=0) the wave holds both MBs'.
#if ZW_I4P_LANES
typedef I4PState I4PSearch;
#else
struct I4PSearch {
    I4State mb[2];
};
#endif

template <int PASS, int NB>
DI void i4p_step(const Ctx& CA, const Ctx& CB, const int* sbx, const int* sby, int K, const I4PLane& LC,
                 I4PSearch& st, const bool act[2], bool keep)
{
    [[maybe_unused]] const Ctx& C = CA;  // (the phase counters)
    const int l = CA.lane, m = l & 15, hm = l >> 5;
    const int slot = NB == 2 ? (l >> 4) & 1 : 0;
    const int sl = NB == 2 ? 1 : 0;
    int x0[NB], y0[NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        x0[h] = sbx[h] * 4 + 1;
        y0[h] = sby[h] * 4 + 1;
    }
    const int bx = csel(slot, sbx[sl], sbx[0]), by = csel(slot, sby[sl], sby[0]);
#if ZW_I4P_LANES
    // the lane's block's contexts from its MB's state
    const int tctx = i4p_tctx(st, bx, by), lctx = i4p_lctx(st, bx, by), ctx0 = i4p_nzctx(st, bx, by);
#else
    // per (MB, slot) contexts, wave-uniform, then the lane's
    int tc[2][NB], lc[2][NB], nc[2][NB];
#pragma unroll
    for (int h = 0; h < NB; h++) {
        const int i = sby[h] * 4 + sbx[h];
#pragma unroll
        for (int mb = 0; mb < 2; mb++) {
            tc[mb][h] = sby[h] == 0 ? 0 : (int)((st.mb[mb].mpack >> (4 * (i - 4))) & 15);
            lc[mb][h] = sbx[h] == 0 ? 0 : (int)((st.mb[mb].mpack >> (4 * (i - 1))) & 15);
            nc[mb][h] = (sby[h] == 0 ? 0 : (int)((st.mb[mb].tnz >> sbx[h]) & 1)) +
                        (sbx[h] == 0 ? 0 : (int)((st.mb[mb].lnz >> sby[h]) & 1));
        }
    }
    auto pick = [&](const int (&v)[2][NB]) {
        const int a = csel(slot, v[0][sl], v[0][0]), b = csel(slot, v[1][sl], v[1][0]);
        return csel(hm, b, a);
    };
    const int tctx = pick(tc), lctx = pick(lc), ctx0 = pick(nc);
#endif
    const uint8_t* sYh = hm ? CB.sY : CA.sY;
    const LdsTables* Th = hm ? CB.T : CA.T;  // the lane's frame's tables (costs, probabilities)
    const int k = (l >> 2) & 3, q = l & 3;
    // what the candidate phase reads without knowing its mode: the costs of an
    // empty block, its source row q, the mode costs' row
    int hn[2];
    uint32_t swq;
    const uint16_t* fcrow;
    auto read_ctx = [&]() {
        hn[0] = (int)Th->binit[3][0][ctx0] & -(int)(ctx0 == 0);
        hn[1] = (int)Th->beob[3][0][ctx0];
        swq = *(const uint32_t*)(sYh + (by * 4 + q) * 16 + bx * 4);
        fcrow = Th->fci4[tctx][lctx];
    };
    PH_START();
    const uint32_t vp = i4p_values<NB>(CA, CB, x0, y0);
#if !ZW_I4P_TMV
    // TrueMotion offsets V[5 + j] - V[4] of the lane's (MB, slot), as (x0, x1), (x3, x2) pairs
    uint32_t ap01, ap32;
    {
        const uint32_t P = (uint32_t)__builtin_amdgcn_readlane((int)vp, 4);
        uint32_t a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) a[j] = (uint32_t)__builtin_amdgcn_readlane((int)vp, 5 + j);
        const int sh = 8 * (2 * hm + slot);
        const int p_ = (int)((P >> sh) & 255u);
        const int d0 = (int)((a[0] >> sh) & 255u) - p_, d1 = (int)((a[1] >> sh) & 255u) - p_;
        const int d2 = (int)((a[2] >> sh) & 255u) - p_, d3 = (int)((a[3] >> sh) & 255u) - p_;
        ap01 = pack_lo(d0, d1);
        ap32 = pack_lo(d3, d2);
    }
#endif
    PH_MARK_L(10, l, 0);
#if ZW_I4P_INV
    read_ctx();  // (before the ranking: its round trips hide these)
#endif
    // ranking: the four rows of (MB, slot, mode) in one lane
#if ZW_I4P_DOT4
    uint32_t pp = 0, sp = 0;  // sum p^2, sum s p: their key orders the modes as the SSE's does (i4p_rank_key)
#else
    int pse = 0;
#endif
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t ix = LC.ix[r];
        const uint32_t v0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ix & 255u), (int)vp);
        const uint32_t v1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ix >> 8) & 255u), (int)vp);
        const uint32_t v2 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ix >> 16) & 255u), (int)vp);
        const uint32_t v3 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ix >> 24), (int)vp);
        const uint32_t sw = *(const uint32_t*)(sYh + (by * 4 + r) * 16 + bx * 4);
#if ZW_I4P_DOT4 && ZW_I4P_TMV
        // the row's four predictions as bytes, in the source row's order
        const uint32_t b01 = __builtin_amdgcn_perm(v1, v0, LC.bsel), b23 = __builtin_amdgcn_perm(v3, v2, LC.bsel);
        const uint32_t pw = i4p_pack_row(b01, b23);
#else
        const uint32_t q01 = __builtin_amdgcn_perm(v1, v0, LC.psel), q32 = __builtin_amdgcn_perm(v2, v3, LC.psel);
#if ZW_I4P_TMV
        const uint32_t p01 = q01, p32 = q32;
#else
        const uint32_t p01 = LC.tm ? clamp_pk(add_pk(q01, ap01)) : q01;
        const uint32_t p32 = LC.tm ? clamp_pk(add_pk(q32, ap32)) : q32;
#endif
#if ZW_I4P_DOT4
        const uint32_t pw = __builtin_amdgcn_perm(p32, p01, ZW_I4P_PAIRS_TO_ROW);  // (TrueMotion clamps in 16-bit form first)
#endif
#endif
#if ZW_I4P_DOT4
        pp = __builtin_amdgcn_udot4(pw, pw, pp, false);
        sp = __builtin_amdgcn_udot4(sw, pw, sp, false);
#else
        const uint32_t d01 = sub_pk(__builtin_amdgcn_perm(0u, sw, 0x0c010c00u), p01);
        const uint32_t d32 = sub_pk(__builtin_amdgcn_perm(0u, sw, 0x0c020c03u), p32);
        pse = dot2v(d01, d01, pse);
        pse = dot2v(d32, d32, pse);
#endif
    }
#if ZW_I4P_DOT4
    const int key = m < 10 ? (int)i4p_rank_key(pp, sp, m) : 0x7fffffff;
#else
    const int key = m < 10 ? (pse << 4) | m : 0x7fffffff;
#endif
    const int rank = rank16(key);
    PH_MARK_L(11, l, 0);
#if ZW_I4P_INV
    // candidate modes: the ranks of a group's modes are a permutation, so its
    // inverse is one forward permute (lane (g, m) sends m to quad `rank` of its
    // group) and a quad broadcast; nothing goes through the scalar unit
    const int mv = i4p_mode(l, K, qb0(__builtin_amdgcn_ds_permute(4 * i4p_inv_dest(l, rank), m)));
#else
    // candidate modes: k-th of each (MB, slot) group, four bits each, group g at bit 16 g
    unsigned long long modes = 0;
    for (int kk = 0; kk < K; kk++) {
        const unsigned long long b = __ballot(m < 10 && rank == kk);
#pragma unroll
        for (int g = 0; g < 4; g++)
            modes |= (unsigned long long)__builtin_ctz((uint32_t)(b >> (16 * g)) | 0x10000u) << (16 * g + 4 * kk);
    }
    const int mq = (int)((modes >> (16 * (2 * hm + slot) + 4 * k)) & 15ull);
    const int mv = k < K ? mq : 0;  // (k >= K: a valid mode, never eligible)
    read_ctx();
#endif
    const int mcost = fcrow[mv];
    const uint32_t iq0 = LC.iq0, bs0 = LC.bs0, iq1 = LC.iq1, bs1 = LC.bs1;
    const int q0 = LC.q0, qa = LC.qa;
    uint32_t p01, p32;
    {
        const uint32_t iw = *(const uint32_t*)&Th->i4qp[mv][4 * q];
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[j] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((iw >> (8 * j)) & 255u), (int)vp);
        const uint32_t q01 = __builtin_amdgcn_perm(v[1], v[0], LC.psel), q32 = __builtin_amdgcn_perm(v[2], v[3], LC.psel);
#if ZW_I4P_TMV
        p01 = q01;
        p32 = q32;
#else
        const bool tm = mv == 1;
        p01 = tm ? clamp_pk(add_pk(q01, ap01)) : q01;
        p32 = tm ? clamp_pk(add_pk(q32, ap32)) : q32;
#endif
    }
    const uint32_t s01 = __builtin_amdgcn_perm(0u, swq, 0x0c010c00u);
    const uint32_t s32 = __builtin_amdgcn_perm(0u, swq, 0x0c020c03u);
    PH_MARK_L(22, l, 0);
    const uint32_t R01 = sub_pk(s01, p01), R32 = sub_pk(s32, p32);
    int cf[4];
    uvq_fdct(add_pk(R01, R32), sub_pk(R01, R32), q, cf);
    int av[4], dq[4], lv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const bool dcs = r == 0;  // (0, q): the DC for q = 0
        const int v = cf[r];
        const int a = (int)((__umul24((uint32_t)iabs(v), dcs ? iq0 : iq1) + (dcs ? bs0 : bs1)) >> 17);
        av[r] = a;
        lv[r] = v < 0 ? -a : a;
        dq[r] = m24(lv[r], dcs ? q0 : qa);
    }
    int last;
    const int cost = rcost_quad<PASS == 2>(av, q, ctx0, 3, Th, last, hn);
    PH_MARK_L(23, l, 0);
    uint32_t r01, r32;
    uvq_idct_recon(dq, p01, p32, q, r01, r32);
    int sse = 0;
    {
        const uint32_t d01 = sub_pk(s01, r01), d32 = sub_pk(s32, r32);
        sse = dot2v(d01, d01, sse);
        sse = dot2v(d32, d32, sse);
    }
    sse = quad_sum(sse);
    const uint32_t rate = (uint32_t)(mcost + cost);
    const uint32_t score = (uint32_t)sse * 256u + (rate & 0xffffu) * LC.l_i4;
    const uint32_t key2 = k < K ? (score << 2) | (uint32_t)k : 0xffffffffu;
    const uint32_t kmin = min16u(key2);
    const bool actl = hm ? act[1] : act[0];
#if ZW_I4P_LANES
    // the winner: the eligible quad holding its group's smallest key (k in the
    // key's low bits: one quad).  Its words go to every lane of its MB, and every
    // lane takes its MB's winners into its copy of the state.
    const bool winl = key2 == kmin && k < K;
    PH_MARK_L(12, l, 0);
    {
        const I4PWin own = i4p_win(rate, (uint32_t)mcost, last >= 0, (uint32_t)sse, mv);
        uint32_t w0 = winl ? own.pk : 0u, w1 = winl ? own.sm : 0u;
        w0 |= (uint32_t)ror8((int)w0);
        w1 |= (uint32_t)ror8((int)w1);
        w0 |= (uint32_t)ror4((int)w0);
        w1 |= (uint32_t)ror4((int)w1);
        const uint32_t lml = hm ? CB.S->l_mode : CA.S->l_mode;
        if (NB == 2) {
            // [h]: slot h's word in both rows of the MB
            const auto p0 = __builtin_amdgcn_permlane16_swap(w0, w0, false, false);
            const auto p1 = __builtin_amdgcn_permlane16_swap(w1, w1, false, false);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                I4PWin w;
                w.pk = p0[h];
                w.sm = p1[h];
                i4p_state_update(st, sbx[h], sby[h], w, lml);
            }
        } else {
            I4PWin w;
            w.pk = w0;
            w.sm = w1;
            i4p_state_update(st, sbx[0], sby[0], w, lml);
        }
        if (actl && m == 0 && ((l >> 4) & 1) < NB) (hm ? CB.M : CA.M)->modes[by * 4 + bx] = (uint8_t)(w1 >> 24);
    }
#else
    const unsigned long long win = __ballot(key2 == kmin);
    // the winner's u16 rate, mode cost (< 2^15) and nonzero flag in one word: one
    // readlane for them instead of three
    const uint32_t pk = (rate & 0xffffu) | ((uint32_t)mcost << 16) | ((uint32_t)(last >= 0) << 31);
    PH_MARK_L(12, l, 0);
#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
        const ZwSegment& S = *(mb ? CB : CA).S;
        MbLds* M = (mb ? CB : CA).M;
#pragma unroll
        for (int h = 0; h < NB; h++) {
            const int gg = 2 * mb + h;
            const int bk = __builtin_ctz((uint32_t)(win >> (16 * gg)) & 0xffffu) >> 2;
            const int wl = 16 * gg + 4 * bk;
#if ZW_I4P_INV
            const int bmode = __builtin_amdgcn_readlane(mv, wl);
#else
            const int bmode = (int)((modes >> (16 * gg + 4 * bk)) & 15ull);
#endif
            const uint32_t bsse = (uint32_t)__builtin_amdgcn_readlane(sse, wl);
            const uint32_t bpk = (uint32_t)__builtin_amdgcn_readlane((int)pk, wl);
            const uint32_t brate = bpk & 0xffffu;
            const int bnz = (int)(bpk >> 31);
            const int i = sby[h] * 4 + sbx[h];
            I4State& s = st.mb[mb];
            s.tnz = (s.tnz & ~(1u << sbx[h])) | ((uint32_t)bnz << sbx[h]);
            s.lnz = (s.lnz & ~(1u << sby[h])) | ((uint32_t)bnz << sby[h]);
            s.nzm |= (uint32_t)bnz << i;
            s.total_mc += (bpk >> 16) & 0x7fffu;
            s.running += rdscore(bsse, brate, S.l_mode);
            s.mpack |= (unsigned long long)bmode << (4 * i);
            if (act[mb] && l == gg) M->modes[i] = (uint8_t)bmode;
        }
    }
    const bool winl = k == (__builtin_ctz((uint32_t)(win >> (16 * (2 * hm + slot))) & 0xffffu) >> 2);
#endif
    // the winners' quads write their rows of the reconstruction (and levels)
    if (winl && ((l >> 4) & 1) < NB && actl) {
        MbLds* M = hm ? CB.M : CA.M;
        const int xo = csel(slot, x0[sl], x0[0]), yo = csel(slot, y0[sl], y0[0]);
        const uint32_t wd = __builtin_amdgcn_perm(r32, r01, 0x04060200u);
        uint8_t* p = M->ws + (yo + q) * ZW_BPS + xo;
#pragma unroll
        for (int j = 0; j < 4; j++) p[j] = (uint8_t)(wd >> (8 * j));
        if (keep) {
            int16_t* lvp = M->lev[by * 4 + bx];
#pragma unroll
            for (int r = 0; r < 4; r++) lvp[izz_of(4 * r + q)] = (int16_t)lv[r];
        }
    }
    wsync();
    PH_MARK_L(13, l, 0);
}

// pick_best_intra4 (vp8.rs:1790-2040) of two MBs at once (K <= 4): bit mb of
// the result is set when I4 wins MB mb (A, B); each MB's early exits are the
// single search's (pick_i4).  An MB with act* false is not searched (its
// lanes compute on its work buffer with every store masked).
template <int PASS>
__device__ uint32_t pick_i4_pair(const Ctx& CA, const Ctx& CB, unsigned long long i16A, unsigned long long i16B,
                                 bool actA, bool actB, bool keep, uint32_t& nzA, uint32_t& nzB)
{
    const int K = CA.method <= 3 ? 3 : 4;
    I4PSearch st;
#if ZW_I4P_LANES
    i4p_state_init(st, (CA.lane >> 5) ? CB.S->l_mode : CA.S->l_mode);
#else
    st.mb[0].running = 211ull * CA.S->l_mode;
    st.mb[1].running = 211ull * CB.S->l_mode;
#pragma unroll
    for (int mb = 0; mb < 2; mb++) {
        st.mb[mb].total_mc = 0;
        st.mb[mb].mpack = 0;
        st.mb[mb].tnz = st.mb[mb].lnz = st.mb[mb].nzm = 0;
    }
    const unsigned long long lim[2] = {i16A, i16B};
#endif
    bool act[2] = {actA, actB};  // (an MB without a search: its lanes run masked)
    I4PLane LC;
    i4p_lane_init(CA, CB, LC);
    for (int s = 0; s < 10; s++) {
        const int sbyA = s < 4 ? 0 : (s - 2) >> 1;
        const int sbxA = s - 2 * sbyA;
        if (s >= 2 && s <= 7) {
            const int bx[2] = {sbxA, sbxA - 2}, by[2] = {sbyA, sbyA + 1};
            i4p_step<PASS, 2>(CA, CB, bx, by, K, LC, st, act, keep);
        } else {
            i4p_step<PASS, 1>(CA, CB, &sbxA, &sbyA, K, LC, st, act, keep);
        }
#if ZW_I4P_LANES
        // the one way out of the lanes per step: each MB's exits, from its first lane
        if (__ballot(i4p_exit(st, i16A)) & 1ull) act[0] = false;
        if ((__ballot(i4p_exit(st, i16B)) >> 32) & 1ull) act[1] = false;
#else
#pragma unroll
        for (int mb = 0; mb < 2; mb++)
            if (st.mb[mb].running >= lim[mb] || st.mb[mb].total_mc > 256u * 16u * 16u / 4u) act[mb] = false;
#endif
        if (!act[0] && !act[1]) return 0;
    }
#if ZW_I4P_LANES
    nzA = (uint32_t)__builtin_amdgcn_readlane((int)st.nzt, 0) & 0xffffu;
    nzB = (uint32_t)__builtin_amdgcn_readlane((int)st.nzt, 32) & 0xffffu;
#else
    nzA = st.mb[0].nzm;
    nzB = st.mb[1].nzm;
#endif
    return (uint32_t)act[0] | ((uint32_t)act[1] << 1);
}

// Final luma transform (transform_luma_block vp8.rs:2647 / _4x4 :2785).
// Writes zigzag levels to C.M->lev[0..16], recon into C.M->ws.  Returns the
// simple-quant "any nonzero" flag for skip detection (check_all_coeffs_zero).
__device__ int final_luma(const Ctx& C, int mode, bool trel, int y_nz_out[16], int i4_nzm)
{
    WaveLds* W = C.W;
    const ZwSegment& S = *C.S;
    const int l = C.lane;
    int anynz = 0;
    PH_START();
    if (mode == 4 && i4_nzm >= 0) {
        // simple quantisation: the search's winners are the final blocks (same
        // prediction, transform and quantize_coeff); their levels are in
        // C.M->lev, their reconstruction in C.M->ws
#pragma unroll
        for (int i = 0; i < 16; i++) y_nz_out[i] = (i4_nzm >> i) & 1;
        if (l < 16) C.M->lev[16][l] = 0;
        wsync();
        PH_MARK_L(15, l, 0);
        PH_COUNT(7);
        return i4_nzm != 0;
    }
    if (mode != 4) {
        build_luma_border(C);
        const uint8_t* ws = C.M->ws;
        const int above = C.mby != 0, left = C.mbx != 0;
        const int b = l & 15, bx = b & 3, by = b >> 2;
        int dcv;
        {  // DC predictor: lanes 0..15 top row, 16..31 left column
            const int top = l < 16;
            const int v = (int)ws[csel(top, 1 + b, (b + 1) * ZW_BPS)] & -(int)(l < 32 && (top ? above : left));
            const int sum = red16(v);
            const int su = __builtin_amdgcn_readlane(sum, 0) + __builtin_amdgcn_readlane(sum, 16);
            const int shf = 3 + above + left;
            dcv = (!above && !left) ? 128 : ((su + (1 << (shf - 1))) >> shf);
        }
        int c[16], pr[16];
        {
            // every 16-lane group computes its block's coefficients (lanes 16..47
            // feed the ctx-parallel trellis)
            const int P0 = ws[0];
            int L[4], Tp[4], r[16];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                L[i] = ws[(by * 4 + i + 1) * ZW_BPS];
                Tp[i] = ws[1 + bx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t srow = *(const uint32_t*)(C.sY + (by * 4 + i) * 16 + bx * 4);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int p = sel4(mode, dcv, Tp[j], L[i], clamp255(L[i] + Tp[j] - P0));
                    pr[i * 4 + j] = p;
                    r[i * 4 + j] = (int)((srow >> (8 * j)) & 255u) - p;
                }
            }
            fdct16_pk(r, c);
        }
        // Y2 (the 16 DCs) in group form: lane b holds block b's DC
        int y2dq;
        {
            const int d = wht_g(c[0], b);
            const int t = b > 0;
            const int y2q = quantz(d, S.y2.iq[t], S.y2.bias[t]);
            if (l < 16) C.M->lev[16][izz_of(b)] = (int16_t)y2q;
            if (gmask(y2q != 0)) anynz = 1;
            y2dq = iwht_g(m24(y2q, (int)S.y2.q[t]), b);
        }
        PH_MARK_L(16, l, 0);
        int dq[16], lv[16];
        int nzb = 0;
        {
            // simple-quant check on the AC coefficients (check_all_coeffs_zero)
            int snz = 0;
            if (l < 16) {
#pragma unroll
                for (int k = 1; k < 16; k++) snz |= quantz(c[k], S.y1.iq[1], S.y1.bias[1]) != 0;
            }
            anynz |= __any(snz) ? 1 : 0;
        }
        if (trel) {
            // Trellis for every block under all three contexts at once (lane =
            // ctx0*16 + block), then resolve the raster-order nz context chain
            // (left / top neighbours) on the scalar unit and pick each block's result.
            int tnz = 0;
            if (l < 48) {
#pragma unroll
                for (int k = 0; k < 16; k++) dq[k] = c[k];
                tnz = trellis<1, true>(dq, lv, S.y1, S.sharpen, S.lt_i16, C.T, 0, l >> 4);
            }
            PH_MARK_L(17, l, 0);
            const unsigned long long nzm = __ballot(l < 48 && tnz);
            int nt[4], nl[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                nt[q] = __builtin_amdgcn_readfirstlane(C.top_c[C.ocx + 1 + q]);
                nl[q] = __builtin_amdgcn_readfirstlane(C.M->left_c[1 + q]);
            }
            unsigned code = 0, nzbits = 0;
#pragma unroll
            for (int bb = 0; bb < 16; bb++) {
                const int cx = min(nl[bb >> 2] + nt[bb & 3], 2);
                const int z = (int)((nzm >> (cx * 16 + bb)) & 1ull);
                nt[bb & 3] = z;
                nl[bb >> 2] = z;
                code |= (unsigned)cx << (2 * bb);
                nzbits |= (unsigned)z << bb;
            }
            const int srcl = (int)((code >> (2 * b)) & 3u) * 16 + b;
            // gather the chosen context's levels as i16 pairs (|level| <= 2047)
            // and dequantise them again (the trellis leaves level * q at the AC
            // positions; the DC position is replaced by the Y2 output below)
            lv[0] = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t w = (uint32_t)__shfl((int)pack_lo(lv[2 * i], lv[2 * i + 1]), srcl);
                lv[2 * i] = lo16(w);
                lv[2 * i + 1] = hi16(w);
            }
#pragma unroll
            for (int n = 1; n < 16; n++) dq[kZZ(n)] = m24(lv[n], (int)S.y1.q[1]);
            nzb = (nzbits >> b) & 1u;
            PH_MARK_L(18, l, 0);
        } else if (l < 16) {
#pragma unroll
            for (int n = 1; n < 16; n++) {
                const int j = kZZ(n);
                lv[n] = quantz(c[j], S.y1.iq[1], S.y1.bias[1]);
                nzb |= lv[n] != 0;
            }
            dq[0] = 0;
#pragma unroll
            for (int n = 1; n < 16; n++) dq[kZZ(n)] = m24(lv[n], (int)S.y1.q[1]);
        }
        wsync();
        if (l < 16) {
            lv[0] = 0;
#pragma unroll
            for (int n = 0; n < 16; n++) C.M->lev[b][n] = (int16_t)lv[n];
            dq[0] = y2dq;
            idct16(dq);
            uint8_t* wsp = C.M->ws;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int y = by * 4 + (k >> 2), x = bx * 4 + (k & 3);
                wsp[(y + 1) * ZW_BPS + 1 + x] = (uint8_t)clamp255(pr[k] + dq[k]);
            }
        }
        const unsigned nzmask = (unsigned)__ballot(l < 16 && nzb);  // block b's flag at bit b
        for (int k = 0; k < 16; k++) y_nz_out[k] = (int)((nzmask >> k) & 1u);
        wsync();
        PH_MARK_L(14, l, 0);
    } else {
        build_luma_border(C);
        int top_nz[4], left_nz[4];
        for (int k = 0; k < 4; k++) {
            top_nz[k] = C.top_c[C.ocx + 1 + k];
            left_nz[k] = C.M->left_c[1 + k];
        }
        for (int i = 0; i < 16; i++) {
            const int sby = i >> 2, sbx = i & 3, x0 = sbx * 4 + 1, y0 = sby * 4 + 1;
            const int bm = C.M->modes[i];
            i4_values(C, x0, y0);
            // 16-lane group form: every group computes the same block; group 0 stores
            const int k = l & 15;
            const int pk = i4_pred_at(W->V[0], i4_src_index(C.T, bm, k), W->V[0][5 + (k & 3)] - W->V[0][4]);
            const int svk = C.sY[(sby * 4 + (k >> 2)) * 16 + sbx * 4 + (k & 3)];
            const int ck = fdct_g(svk - pk, k);
            const int ctx0 = min(left_nz[sby] + top_nz[sbx], 2);
            if (C.a->dbg && C.a->pass == 2 && l < 16) {
                int* d = C.a->dbg + (((size_t)C.f * C.a->mbw * C.a->mbh + (size_t)C.mby * C.a->mbw + C.mbx) * 16 + i) * 34;
                d[k] = ck;
                d[16 + k] = pk;
                if (k == 0) {
                    d[32] = ctx0;
                    d[33] = bm;
                }
            }
            const int qs = quantz(ck, S.y1.iq[k > 0], S.y1.bias[k > 0]);
            const int snz = gmask(qs != 0) != 0;
            int dqk, nzq;
            if (trel) {
                // lane-parallel trellis: lane n = zigzag position n
                const int cn = gget(ck, zz_of(k));
                int lvn;
                nzq = trellis_g<0>(cn, k, S.y1, S.sharpen, S.lt_i4, C.T, 3, ctx0, lvn);
                if (l < 16) C.M->lev[i][k] = (int16_t)lvn;
                dqk = m24(gget(lvn, izz_of(k)), (int)S.y1.q[k > 0]);
            } else {
                if (l < 16) C.M->lev[i][izz_of(k)] = (int16_t)qs;
                nzq = snz;
                dqk = m24(qs, (int)S.y1.q[k > 0]);
            }
            const int rk = idct_g(dqk, k);
            if (l < 16) C.M->ws[(y0 + (k >> 2)) * ZW_BPS + x0 + (k & 3)] = (uint8_t)clamp255(pk + rk);
            wsync();
            if (l == 0) {
                W->misc[1] = nzq;
                W->misc[2] = snz;
            }
            wsync();
            const int nz = W->misc[1];
            anynz |= W->misc[2];
            top_nz[sbx] = nz;
            left_nz[sby] = nz;
            y_nz_out[i] = nz;
            wsync();
        }
        if (l < 16) C.M->lev[16][l] = 0;
        wsync();
        PH_MARK_L(15, l, 0);
        PH_COUNT(7);
    }
    return anynz;
}

// The final I16 luma transform (final_luma, mode != 4) of both MBs of a frame
// pair in one pass of the wave: frame 0's MB in lanes 0..31, frame 1's in
// lanes 32..63, lane 16 k + b of a half holding block b (a half's second group
// repeats the first; the first stores).  Each frame uses its own segment,
// tables, borders and MbLds.  With the trellis, a block runs only under the
// start contexts its neighbours leave open and not at all when the trellis
// can only return zeros (zw_enc_pairfinal.h): the two MBs' runs are numbered
// onto the wave's lanes and, when they are 64 at the most, worked in one
// trellis call (their coefficients go to the task lanes through C.M->lev[b],
// not yet written; the task table through W->dc); otherwise in one call per
// frame with every block under every context, as final_luma does.  The context
// chains are then resolved on the scalar unit, per frame, and every block
// gathers its resolved context's levels from the lane that ran it.
// res: the MB's per-block has-coefficients flags (bits 0..15) and the
// simple-quant "any nonzero" flag (bit 16), as final_luma returns them.
__device__ void final_luma_pair(const Ctx& CA, const Ctx& CB, int modeA, int modeB, bool trel, uint32_t& resA,
                                uint32_t& resB)
{
    [[maybe_unused]] const Ctx& C = CA;  // (the phase counters)
    WaveLds* W = CA.W;
    const int l = CA.lane, hm = l >> 5, b = l & 15, bx = b & 3, by = b >> 2;
    const bool own = (l & 16) == 0;
    PH_START();
    build_luma_border(CA);
    build_luma_border(CB);
    MbLds* const M = hm ? CB.M : CA.M;
    const ZwSegment* const S = hm ? CB.S : CA.S;
    const uint8_t* const sY = hm ? CB.sY : CA.sY;
    const int mode = hm ? modeB : modeA;
    const uint8_t* ws = M->ws;
    const int above = CA.mby != 0, left = CA.mbx != 0;
    int dcv;
    {  // DC predictor, per half: its first group the top row, its second the left column
        const int v = (int)ws[csel(own, 1 + b, (b + 1) * ZW_BPS)] & -(int)(own ? above : left);
        const int sum = red16(v);
        const int sa = __builtin_amdgcn_readlane(sum, 0) + __builtin_amdgcn_readlane(sum, 16);
        const int sb = __builtin_amdgcn_readlane(sum, 32) + __builtin_amdgcn_readlane(sum, 48);
        const int shf = 3 + above + left;
        dcv = (!above && !left) ? 128 : (((hm ? sb : sa) + (1 << (shf - 1))) >> shf);
    }
    int c[16];
    uint32_t ppk[4];  // the prediction, a row of 4 pixels per word
    {
        const int P0 = ws[0];
        int L[4], Tp[4], r[16];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            L[i] = ws[(by * 4 + i + 1) * ZW_BPS];
            Tp[i] = ws[1 + bx * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t srow = *(const uint32_t*)(sY + (by * 4 + i) * 16 + bx * 4);
            ppk[i] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int p = sel4(mode, dcv, Tp[j], L[i], clamp255(L[i] + Tp[j] - P0));
                ppk[i] |= (uint32_t)p << (8 * j);
                r[i * 4 + j] = (int)((srow >> (8 * j)) & 255u) - p;
            }
        }
        fdct16_pk(r, c);
    }
    // Y2 (the 16 DCs) in group form, and the simple-quant check (check_all_coeffs_zero)
    int y2dq;
    uint32_t anyA, anyB;
    {
        const int d = wht_g(c[0], b);
        const int t = b > 0;
        const int y2q = quantz(d, S->y2.iq[t], S->y2.bias[t]);
        if (own) M->lev[16][izz_of(b)] = (int16_t)y2q;
        y2dq = iwht_g(m24(y2q, (int)S->y2.q[t]), b);
        int snz = y2q != 0;
        const uint32_t iq1 = S->y1.iq[1], bs1 = S->y1.bias[1];
#pragma unroll
        for (int k = 1; k < 16; k++) snz |= quantz(c[k], iq1, bs1) != 0;
        const unsigned long long any = __ballot(snz != 0);
        anyA = (uint32_t)any != 0u;
        anyB = (uint32_t)(any >> 32) != 0u;
    }
    PH_MARK_L(16, l, 0);
    const int q1 = (int)S->y1.q[1];
    int nzb = 0;
    // a block's levels (zigzag, lv[1..15]) to C.M->lev[b], dequantised, inverse
    // transformed and added to the prediction in C.M->ws
    auto finish = [&](bool act, int* lv) {
        wsync();
        if (act) {
            int dq[16];
            lv[0] = 0;
#pragma unroll
            for (int n = 0; n < 16; n++) M->lev[b][n] = (int16_t)lv[n];
#pragma unroll
            for (int n = 1; n < 16; n++) dq[kZZ(n)] = m24(lv[n], q1);
            dq[0] = y2dq;
            idct16(dq);
            uint8_t* wsp = M->ws;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int y = by * 4 + (k >> 2), x = bx * 4 + (k & 3);
                const int p = (int)((ppk[k >> 2] >> (8 * (k & 3))) & 255u);
                wsp[(y + 1) * ZW_BPS + 1 + x] = (uint8_t)clamp255(p + dq[k]);
            }
        }
    };
    if (trel) {
        const bool tzl = pf_trivial(c, (uint32_t)q1, S->y1.iq[1], S->sharpen);
        const unsigned long long tzb = __ballot(tzl);
        const unsigned tzA = (unsigned)tzb & 0xffffu, tzB = (unsigned)(tzb >> 32) & 0xffffu;
        // the MBs' edge flags (the MBs above and to the left are final)
        unsigned eA = 0, eB = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            eA |= (unsigned)(__builtin_amdgcn_readfirstlane(CA.top_c[CA.ocx + 1 + q]) != 0) << q;
            eA |= (unsigned)(__builtin_amdgcn_readfirstlane(CA.M->left_c[1 + q]) != 0) << (4 + q);
            eB |= (unsigned)(__builtin_amdgcn_readfirstlane(CB.top_c[CB.ocx + 1 + q]) != 0) << q;
            eB |= (unsigned)(__builtin_amdgcn_readfirstlane(CB.M->left_c[1 + q]) != 0) << (4 + q);
        }
        // the MBs' tasks: bit cx * 16 + b
        unsigned long long mA = 0, mB = 0;
        {
            const unsigned need = pf_need(b, hm ? tzB : tzA, hm ? eB : eA);
#pragma unroll
            for (int cx = 0; cx < 3; cx++) {
                const unsigned long long nb = __ballot((need >> cx) & 1u);
                mA |= (nb & 0xffffull) << (16 * cx);
                mB |= ((nb >> 32) & 0xffffull) << (16 * cx);
            }
        }
        const bool one = pf_one_call(mA, mB);
        // the coefficients to the task lanes (i16 pairs, natural order)
        if (own) {
            uint32_t* st = (uint32_t*)M->lev[b];
#pragma unroll
            for (int i = 0; i < 8; i++) st[i] = pack_lo(c[2 * i], c[2 * i + 1]);
        }
        if (one) PH_COUNT(24);
        else PH_COUNT(25);
        const int ncall = one ? 1 : 2;
#pragma nounroll
        for (int r = 0; r < ncall; r++) {
            // this call's tasks per frame, frame 1's numbered after frame 0's
            const unsigned long long cA = one ? mA : (r == 0 ? ZW_PF_ALL : 0ull);
            const unsigned long long cB = one ? mB : (r == 1 ? ZW_PF_ALL : 0ull);
            const int nA = pf_count(cA), nT = nA + pf_count(cB);
            const unsigned long long cm = hm ? cB : cA;
            const int base = hm ? nA : 0;
            if (own) {
#pragma unroll
                for (int cx = 0; cx < 3; cx++)
                    if ((cm >> (cx * 16 + b)) & 1ull) W->dc[pf_task(cm, base, b, cx) & 63] = (hm << 6) | (cx << 4) | b;
            }
            wsync();
            int lv[16];
#pragma unroll
            for (int n = 0; n < 16; n++) lv[n] = 0;
            int tnz = 0;
            if (l < nT) {
                const int td = W->dc[l];
                const bool tf = (td >> 6) & 1;
                const ZwSegment* const St = tf ? CB.S : CA.S;
                const uint32_t* st = (const uint32_t*)(tf ? CB.M : CA.M)->lev[td & 15];
                int dq[16];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t w = st[i];
                    dq[2 * i] = lo16(w);
                    dq[2 * i + 1] = hi16(w);
                }
                tnz = trellis<1, true>(dq, lv, St->y1, St->sharpen, St->lt_i16, tf ? CB.T : CA.T, 0, (td >> 4) & 3);
            }
            PH_MARK_L(17, l, 0);
            const unsigned long long nzm = __ballot(l < nT && tnz);
            // the raster-order context chain of a frame worked in this call, on
            // the scalar unit: code = the blocks' contexts (2 bits each)
            auto chain = [&](unsigned long long cmf, int basef, unsigned tz, unsigned e, unsigned& code,
                             unsigned& nzbits) {
                int nt[4], nl[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    nt[q] = (int)((e >> q) & 1u);
                    nl[q] = (int)((e >> (4 + q)) & 1u);
                }
                code = nzbits = 0;
#pragma unroll
                for (int bb = 0; bb < 16; bb++) {
                    const int cx = min(nl[bb >> 2] + nt[bb & 3], 2);
                    const int z = ((tz >> bb) & 1u) ? 0 : (int)((nzm >> (pf_task(cmf, basef, bb, cx) & 63)) & 1ull);
                    nt[bb & 3] = z;
                    nl[bb >> 2] = z;
                    code |= (unsigned)cx << (2 * bb);
                    nzbits |= (unsigned)z << bb;
                }
            };
            unsigned codeA = 0, nzA = 0, codeB = 0, nzB = 0;
            if (one || r == 0) chain(cA, 0, tzA, eA, codeA, nzA);
            if (one || r == 1) chain(cB, nA, tzB, eB, codeB, nzB);
            const int cxb = (int)(((hm ? codeB : codeA) >> (2 * b)) & 3u);
            const int srcl = pf_task(cm, base, b, cxb) & 63;
            // gather the chosen context's levels as i16 pairs (|level| <= 2047)
            const bool act = own && (one || r == hm);
            const bool zero = (((hm ? tzB : tzA) >> b) & 1u) != 0u;
            int gl[16];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t w = (uint32_t)__shfl((int)pack_lo(lv[2 * i], lv[2 * i + 1]), srcl);
                gl[2 * i] = zero ? 0 : lo16(w);
                gl[2 * i + 1] = zero ? 0 : hi16(w);
            }
            if (act) nzb = (int)(((hm ? nzB : nzA) >> b) & 1u);
            PH_MARK_L(18, l, 0);
            finish(act, gl);
            wsync();
        }
    } else {
        int lv[16];
#pragma unroll
        for (int n = 1; n < 16; n++) {
            lv[n] = quantz(c[kZZ(n)], S->y1.iq[1], S->y1.bias[1]);
            nzb |= lv[n] != 0;
        }
        finish(own, lv);
    }
    const unsigned long long nzall = __ballot(own && nzb);
    resA = ((uint32_t)nzall & 0xffffu) | (anyA << 16);
    resB = ((uint32_t)(nzall >> 32) & 0xffffu) | (anyB << 16);
    wsync();
    PH_MARK_L(14, l, 0);
}

// Final chroma transform with error diffusion (transform_chroma_blocks
// vp8.rs:3039, apply_chroma_error_diffusion :572), lane-pair form: lanes b and
// 32 + b work block b (U 0..3, V 4..7) from the coefficients pick_uv left for
// the chosen mode.  Levels to C.M->lev[17..24], recon into cu / cv.  Returns the
// simple-quant "any nonzero" flag; uv_nz[8] receives per-block has-coefficients.
__device__ int final_chroma(const Ctx& C, int mode, int8_t* top_derr, int uv_nz[8])
{
    WaveLds* W = C.W;
    const ZwSegment& S = *C.S;
    const int l = C.lane;
    const int h = l >> 5, b = l & 7, pl = b >> 2, bx = b & 1, by = (b >> 1) & 1;
    const bool act = (l & 31) < 8;
    int cf[2][4];
    uint32_t p01[2], p32[2];
    {
        const uint32_t* e = W->uvc[h * 32 + mode * 8 + b];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            cf[c][0] = lo16(e[2 * c]);
            cf[c][1] = hi16(e[2 * c]);
            cf[c][2] = lo16(e[2 * c + 1]);
            cf[c][3] = hi16(e[2 * c + 1]);
        }
        p01[0] = e[4];
        p32[0] = e[5];
        p01[1] = e[6];
        p32[1] = e[7];
    }
    // DC error diffusion (vp8.rs chroma quirk, per plane: blocks 0,1,2,3 in
    // order), on the scalar unit; block k's DC is cf[0][0] of lane k.
    {
        const int q = (int)S.uv.q[0];
        const uint32_t iq = S.uv.iq[0], bias = S.uv.bias[0];
        const uint32_t zt = S.uv.zthresh[0];  // ((1 << 17) - 1 - bias) / iq, matrix_init
        int dcs[8];
#pragma unroll
        for (int k = 0; k < 8; k++) dcs[k] = __builtin_amdgcn_readlane(cf[0][0], k);
        auto diffuse = [&](int& dc, int te, int le) -> int {
            dc += (7 * te + 8 * le) >> 3;
            const int sign = dc < 0;
            const uint32_t a = (uint32_t)(sign ? -dc : dc);
            const int level = a > zt ? (int)((a * iq + bias) >> 17) : 0;
            const int err = (int)a - level * q;
            const int se = sign ? -err : err;
            const int v = se >> 1;
            return (int)(int8_t)(v < -127 ? -127 : (v > 127 ? 127 : v));
        };
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            int8_t* top = top_derr + ch * 2;
            int8_t* lft = C.M->left_derr + ch * 2;
            const int t0 = __builtin_amdgcn_readfirstlane((int)top[0]), t1 = __builtin_amdgcn_readfirstlane((int)top[1]);
            const int l0 = __builtin_amdgcn_readfirstlane((int)lft[0]), l1 = __builtin_amdgcn_readfirstlane((int)lft[1]);
            int* d = dcs + ch * 4;
            const int e0 = diffuse(d[0], t0, l0);
            const int e1 = diffuse(d[1], t1, e0);
            const int e2 = diffuse(d[2], e0, l1);
            const int e3 = diffuse(d[3], e1, e2);
            const int nl1 = (int)(int8_t)((3 * e3) >> 2);
            wsync();
            if (l == 0) {
                lft[0] = (int8_t)e1;
                lft[1] = (int8_t)nl1;
                top[0] = (int8_t)e2;
                top[1] = (int8_t)(e3 - nl1);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; k++)
            asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(cf[0][0]) : "s"(__builtin_amdgcn_readfirstlane(dcs[k])), "i"(k));
    }
    // quantize_coeff of this lane's 8 coefficients (natural index n = 4 row + 2h + col)
    int dq[2][4];
    int nz = 0;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool dcs = c == 0 && r == 0;
            const uint32_t iq = dcs ? (h ? S.uv.iq[1] : S.uv.iq[0]) : S.uv.iq[1];
            const uint32_t bias = dcs ? (h ? S.uv.bias[1] : S.uv.bias[0]) : S.uv.bias[1];
            const int q_ = dcs ? (int)(h ? S.uv.q[1] : S.uv.q[0]) : (int)S.uv.q[1];
            const int lv = quantz(cf[c][r], iq, bias);
            nz |= lv;
            if (act) C.M->lev[17 + b][izz_of(4 * r + 2 * h + c)] = (int16_t)lv;
            dq[c][r] = m24(lv, q_);
        }
    uint32_t r01[2], r32[2];
    idct_recon_pair(dq, p01, p32, h, r01, r32);
    if (act) {
        uint8_t* w = pl ? W->cv : W->cu;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            uint8_t* row = w + (by * 4 + 2 * h + r + 1) * ZW_BPS + 1 + bx * 4;
            row[0] = (uint8_t)(r01[r] & 255u);
            row[1] = (uint8_t)(r01[r] >> 16);
            row[2] = (uint8_t)(r32[r] >> 16);
            row[3] = (uint8_t)(r32[r] & 255u);
        }
    }
    const int nzb = (nz | hx_partner(nz)) != 0;
    int any = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uv_nz[k] = __builtin_amdgcn_readlane(nzb, k);
        any |= uv_nz[k];
    }
    wsync();
    return any;
}

// Publish borders for the next MBs (vp8.rs:2771-2777, :3101-3118).
__device__ void store_luma_borders(const Ctx& C)
{
    const int l = C.lane;
    if (l < 17) C.M->left_y[l] = C.M->ws[l * ZW_BPS + 16];
    else if (l < 33) C.top_y[C.oy + (l - 17)] = C.M->ws[16 * ZW_BPS + (l - 17) + 1];
    if (C.a->ry && l < 64) {
        uint8_t* ry = C.a->ry + (size_t)C.f * C.a->ysz + (size_t)C.mby * 16 * C.ys + C.mbx * 16;
        for (int k = l; k < 256; k += 64) ry[(size_t)(k >> 4) * C.ys + (k & 15)] = C.M->ws[((k >> 4) + 1) * ZW_BPS + 1 + (k & 15)];
    }
    wsync();
}
__device__ void store_chroma_borders(const Ctx& C)
{
    const int l = C.lane;
    WaveLds* W = C.W;
    if (l < 9) {
        C.M->left_u[l] = W->cu[l * ZW_BPS + 8];
        C.M->left_v[l] = W->cv[l * ZW_BPS + 8];
    } else if (l < 17) {
        C.top_u[C.oc + (l - 9)] = W->cu[8 * ZW_BPS + (l - 9) + 1];
        C.top_v[C.oc + (l - 9)] = W->cv[8 * ZW_BPS + (l - 9) + 1];
    }
    if (C.a->ru) {
        uint8_t* ru = C.a->ru + (size_t)C.f * C.a->csz + (size_t)C.mby * 8 * C.cs + C.mbx * 8;
        uint8_t* rv = C.a->rv + (size_t)C.f * C.a->csz + (size_t)C.mby * 8 * C.cs + C.mbx * 8;
        const int k = l;
        ru[(size_t)(k >> 3) * C.cs + (k & 7)] = W->cu[((k >> 3) + 1) * ZW_BPS + 1 + (k & 7)];
        rv[(size_t)(k >> 3) * C.cs + (k & 7)] = W->cv[((k >> 3) + 1) * ZW_BPS + 1 + (k & 7)];
    }
    wsync();
}

__device__ void write_levels(const Ctx& C, int first_blk, int nblk, bool zero)
{
    ZwMbOut* o = C.a->out + (size_t)C.f * C.a->mbw * C.a->mbh + (size_t)C.mby * C.a->mbw + C.mbx;
    // as words (ZwMbOut records and the LDS levels are 4-byte aligned)
    uint32_t* dst = (uint32_t*)&o->levels[first_blk][0];
    const uint32_t* srcl = (const uint32_t*)&C.M->lev[first_blk][0];
    for (int k = C.lane; k < nblk * 8; k += 64) dst[k] = zero ? 0u : srcl[k];
}

// ---------------------------------------------------------------------------
// Pass-1 chroma chain in quad form, one wave per plane (chain wave 0: U,
// chain wave 1: V).  Lane l = 16 m + 4 b + q works mode m (0 DC, 1 V, 2 H,
// 3 TM) of 4x4 block b (bx = b & 1, by = b >> 1): pixel row q for the
// prediction, residual, row transform input and reconstruction; coefficient
// column q for the column transform, quantisation and rate.  A quad gathers
// its rows' row-transform inputs with DPP broadcasts and each lane forms its
// own column, so a lane does a quarter block and the plane's 4 modes x 4
// blocks fill one wave.  The arithmetic (packing points, rounding) is the pair
// form's (fdct_pair / idct_recon_pair), so the results are identical.  Only the
// mode decision couples the planes -- one RD over U + V (pick_best_uv,
// vp8.rs:2050-2200) -- and the waves trade their per-mode (rate, SSE, AC
// nonzeros) through LDS; the DC error diffusion (vp8.rs:572-647) runs per
// channel, so each wave keeps its own.  Halving the chain's instruction stream
// shortens pass 1, which the chain bounds for single frames (quirk A5 makes it
// serial across rows) and nearly bounds in batches.
// ---------------------------------------------------------------------------
struct UvQ {
    int pl;             // 0 U, 1 V
    uint8_t* w;         // the plane's work buffer (create_border_chroma layout, stride ZW_BPS)
    const uint8_t* sp;  // the MB's staged source plane (8x8, stride 8)
    uint8_t* top;       // frame-wide top row of the plane
    uint8_t* left;      // the wave's left column (corner + 8 rows)
};

// create_border_chroma (prediction.rs:85) of one plane
DI void uvq_border(const Ctx& C, const UvQ& U)
{
    const int l = C.lane;
    if (l < 17) {
        if (l == 0) U.w[0] = C.mby == 0 ? 127 : (C.mbx == 0 ? 129 : U.left[0]);
        else if (l <= 8) U.w[l] = C.mby == 0 ? 127 : U.top[C.mbx * 8 + l - 1];
        else U.w[(l - 8) * ZW_BPS] = C.mbx == 0 ? 129 : U.left[l - 8];
    }
    wsync();
}

// get_residual_cost (cost.rs:1670; ctype 2, first 0, ctx0 0; pass 1: the
// LevelCosts tables are zero, quirk A2) of the quad's block, av[r] = |level|
// at natural index 4 r + q.  Uniform in the quad.
DI int uvq_rcost(const int av[4], int q, const LdsTables* T)
{
    unsigned nz = 0, big = 0;
    int part = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int n = 4 * r + q;
        nz |= (unsigned)min(av[r], 1) << n;
        big |= (unsigned)(av[r] >= 2) << n;
        part += T->lfc[min(av[r], 2047)];
    }
    nz = (unsigned)quad_or((int)nz);
    big = (unsigned)quad_or((int)big);
    const int sum = quad_sum(part);
    const int last = 31 - __clz((int)nz);
    const int ctx_t = ((big >> max(last, 0)) & 1u) ? 2 : 1;
    const int tail = (int)T->beob[2][band_of(min(last + 1, 15))][ctx_t] & -(int)(last < 15);
    const int head = (int)T->binit[2][0][0];
    return csel(last < 0, (int)T->beob[2][0][0], head + sum + tail);  // (no divergent branch)
}

// pick_best_uv (vp8.rs:2050-2200) with the partner plane's wave: returns the
// chroma mode.  Leaves each lane's coefficients and prediction row in
// W->uvc[lane] for uvq_final.  xch: [plane][2][12] exchange words, xflag[2].
DI int uvq_pick(const Ctx& C, const UvQ& U, int* xch, int* xflag, int seq)
{
    const ZwSegment& S = *C.S;
    const LdsTables* T = C.T;
    WaveLds* W = C.W;
    const int l = C.lane, m = l >> 4, b = (l >> 2) & 3, q = l & 3, bx = b & 1, by = b >> 1;
    const int above = C.mby != 0, left = C.mbx != 0;
    // DC predictor (lanes 0..15: i < 8 left pixel i, i >= 8 top pixel i - 8)
    int dc;
    {
        const int i = l & 15;
        const int v = (int)U.w[csel(i < 8, (i + 1) * ZW_BPS, i - 7)] & -(int)(i < 8 ? left : above);
        const int su = __builtin_amdgcn_readlane(red16(v), 0);
        const int shf = 2 + left + above;
        dc = (above | left) ? (su + (1 << (shf - 1))) >> shf : 128;
    }
    // prediction and source of row y = 4 by + q (uv_rows_pk)
    uint32_t p01, p32, s01, s32;
    {
        const int cm = -(int)(m & 1), rm = -(int)(m >= 2);
        const int P = U.w[0];
        const int ro = csel(m == 0, dc, csel(m == 3, -P, 0));
        const uint8_t* tp = U.w + 1 + bx * 4;
        const uint32_t c01 = pack_lo(tp[0] & cm, tp[1] & cm), c32 = pack_lo(tp[3] & cm, tp[2] & cm);
        const int y = by * 4 + q;
        const int rv = (U.w[(y + 1) * ZW_BPS] & rm) + ro;
        const uint32_t rvv = pack_lo(rv, rv);
        p01 = clamp_pk(add_pk(c01, rvv));
        p32 = clamp_pk(add_pk(c32, rvv));
        const uint32_t sw = *(const uint32_t*)(U.sp + y * 8 + bx * 4);
        s01 = __builtin_amdgcn_perm(0u, sw, 0x0c010c00u);
        s32 = __builtin_amdgcn_perm(0u, sw, 0x0c020c03u);
    }
    const uint32_t R01 = sub_pk(s01, p01), R32 = sub_pk(s32, p32);
    int cf[4];
    uvq_fdct(add_pk(R01, R32), sub_pk(R01, R32), q, cf);
    {
        uint32_t* e = W->uvc[l];
        e[0] = pack_lo(cf[0], cf[1]);
        e[1] = pack_lo(cf[2], cf[3]);
        e[2] = p01;
        e[3] = p32;
    }
    // quantize_coeff (no sharpening, cost.rs:457): the DC is (r, q) = (0, 0)
    int av[4], dq[4], nzac = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const bool dcs = r == 0 && q == 0;
        const uint32_t iq = dcs ? S.uv.iq[0] : S.uv.iq[1];
        const uint32_t bias = dcs ? S.uv.bias[0] : S.uv.bias[1];
        const int q_ = dcs ? (int)S.uv.q[0] : (int)S.uv.q[1];
        const int v = cf[r];
        const int a = (int)((__umul24((uint32_t)iabs(v), iq) + bias) >> 17);
        av[r] = a;
        dq[r] = m24(v < 0 ? -a : a, q_);
        nzac += dcs ? 0 : min(a, 1);
    }
    const int cost = uvq_rcost(av, q, T);
    uint32_t r01, r32;
    uvq_idct_recon(dq, p01, p32, q, r01, r32);
    int sse = 0;
    {
        const uint32_t d01 = sub_pk(s01, r01), d32 = sub_pk(s32, r32);
        sse = dot2v(d01, d01, sse);
        sse = dot2v(d32, d32, sse);
    }
    // per-mode plane totals (a block's rate once, from its quad's lane 0)
    const int ct = red16(q == 0 ? cost : 0), st = red16(sse), nt = red16(nzac);
    int* mine = xch + (U.pl * 2 + (seq & 1)) * 12;
    const int* theirs = xch + ((1 - U.pl) * 2 + (seq & 1)) * 12;
    if ((l & 15) == 0) {
        mine[m * 3 + 0] = ct;
        mine[m * 3 + 1] = st;
        mine[m * 3 + 2] = nt;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (l == 0) __hip_atomic_store(&xflag[U.pl], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_wave_barrier();
    while (__hip_atomic_load(&xflag[1 - U.pl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq)
        __builtin_amdgcn_s_sleep(1);
    // the same decision in both waves: rd = (fixed + rate + pen) * lambda_uv + 256 * sse
    long long brd = 0x7fffffffffffffffLL;
    int bm = 0;
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        const int c_o = __builtin_amdgcn_readfirstlane(theirs[mm * 3 + 0]);
        const int s_o = __builtin_amdgcn_readfirstlane(theirs[mm * 3 + 1]);
        const int n_o = __builtin_amdgcn_readfirstlane(theirs[mm * 3 + 2]);
        const int c_m = __builtin_amdgcn_readlane(ct, mm * 16), s_m = __builtin_amdgcn_readlane(st, mm * 16);
        const int n_m = __builtin_amdgcn_readlane(nt, mm * 16);
        const int fixed = sel4(mm, d_FIXED_COSTS_UV[0], d_FIXED_COSTS_UV[1], d_FIXED_COSTS_UV[2], d_FIXED_COSTS_UV[3]);
        const int pen = (mm > 0 && n_m + n_o <= 2) ? 140 * 8 : 0;
        const long long r_m = (long long)(fixed + c_m + c_o + pen) * (long long)S.l_uv + 256LL * (long long)(s_m + s_o);
        const int avail = mm == 0 || (mm == 1 && above) || (mm == 2 && left) || (mm == 3 && above && left);
        if (avail && r_m < brd) {
            brd = r_m;
            bm = mm;
        }
    }
    return bm;
}

// transform_chroma_blocks (vp8.rs:3039-3121) of one plane under mode cm:
// the DC error diffusion of channel U.pl (vp8.rs:572-647), quantisation,
// levels into C.M->lev[17 + 4 pl + b], reconstruction into the work buffer.
DI void uvq_final(const Ctx& C, const UvQ& U, int cm, int8_t* top_derr)
{
    WaveLds* W = C.W;
    const ZwSegment& S = *C.S;
    const int l = C.lane, b = (l >> 2) & 3, q = l & 3, bx = b & 1, by = b >> 1;
    const bool act = l < 16;
    int cf[4];
    uint32_t p01, p32;
    {
        const uint32_t* e = W->uvc[cm * 16 + (l & 15)];
        cf[0] = lo16(e[0]);
        cf[1] = hi16(e[0]);
        cf[2] = lo16(e[1]);
        cf[3] = hi16(e[1]);
        p01 = e[2];
        p32 = e[3];
    }
    {
        const int qd = (int)S.uv.q[0];
        const uint32_t iq = S.uv.iq[0], bias = S.uv.bias[0];
        const uint32_t zt = S.uv.zthresh[0];  // ((1 << 17) - 1 - bias) / iq, matrix_init
        int d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = __builtin_amdgcn_readlane(cf[0], 4 * k);
        auto diffuse = [&](int& dc, int te, int le) -> int {
            dc += (7 * te + 8 * le) >> 3;
            const int sign = dc < 0;
            const uint32_t a = (uint32_t)(sign ? -dc : dc);
            const int level = a > zt ? (int)((a * iq + bias) >> 17) : 0;
            const int err = (int)a - level * qd;
            const int se = sign ? -err : err;
            const int v = se >> 1;
            return (int)(int8_t)(v < -127 ? -127 : (v > 127 ? 127 : v));
        };
        int8_t* top = top_derr + U.pl * 2;
        int8_t* lft = C.M->left_derr;
        const int t0 = __builtin_amdgcn_readfirstlane((int)top[0]), t1 = __builtin_amdgcn_readfirstlane((int)top[1]);
        const int l0 = __builtin_amdgcn_readfirstlane((int)lft[0]), l1 = __builtin_amdgcn_readfirstlane((int)lft[1]);
        const int e0 = diffuse(d[0], t0, l0);
        const int e1 = diffuse(d[1], t1, e0);
        const int e2 = diffuse(d[2], e0, l1);
        const int e3 = diffuse(d[3], e1, e2);
        const int nl1 = (int)(int8_t)((3 * e3) >> 2);
        wsync();
        if (l == 0) {
            lft[0] = (int8_t)e1;
            lft[1] = (int8_t)nl1;
            top[0] = (int8_t)e2;
            top[1] = (int8_t)(e3 - nl1);
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            asm volatile("v_writelane_b32 %0, %1, %2"
                         : "+v"(cf[0])
                         : "s"(__builtin_amdgcn_readfirstlane(d[k])), "i"(4 * k));
    }
    int dq[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const bool dcs = r == 0 && q == 0;
        const int lv = quantz(cf[r], dcs ? S.uv.iq[0] : S.uv.iq[1], dcs ? S.uv.bias[0] : S.uv.bias[1]);
        if (act) C.M->lev[17 + 4 * U.pl + b][izz_of(4 * r + q)] = (int16_t)lv;
        dq[r] = m24(lv, dcs ? (int)S.uv.q[0] : (int)S.uv.q[1]);
    }
    uint32_t r01, r32;
    uvq_idct_recon(dq, p01, p32, q, r01, r32);
    if (act) {
        uint8_t* row = U.w + (by * 4 + q + 1) * ZW_BPS + 1 + bx * 4;
        row[0] = (uint8_t)(r01 & 255u);
        row[1] = (uint8_t)(r01 >> 16);
        row[2] = (uint8_t)(r32 >> 16);
        row[3] = (uint8_t)(r32 & 255u);
    }
    wsync();
}

// Borders of one plane for the next MBs (vp8.rs:3101-3118), and its debug
// reconstruction when asked for.
DI void uvq_store_borders(const Ctx& C, const UvQ& U)
{
    const int l = C.lane;
    if (l < 9) U.left[l] = U.w[l * ZW_BPS + 8];
    else if (l < 17) U.top[C.mbx * 8 + (l - 9)] = U.w[8 * ZW_BPS + (l - 9) + 1];
    uint8_t* rp = U.pl ? C.a->rv : C.a->ru;
    if (rp) {
        rp += (size_t)C.f * C.a->csz + (size_t)C.mby * 8 * C.cs + C.mbx * 8;
        rp[(size_t)(l >> 3) * C.cs + (l & 7)] = U.w[((l >> 3) + 1) * ZW_BPS + 1 + (l & 7)];
    }
    wsync();
}

// What an MB needs from global memory, fetched one MB ahead (the loads are in
// flight while the previous MB is encoded): the lane's word of the source MB
// (luma: row lane>>2, word lane&3; chroma lanes < 32: plane lane>>4, row
// (lane>>1)&7, word lane&1) and the MB's alpha (segment lookup).
struct MbFetch {
    uint32_t y, c;
    int alpha;
};
__device__ __forceinline__ MbFetch fetch_mb(const EncArgs* a, int f, int lane, int mbx, int mby)
{
    const int ys = a->mbw * 16, cs = a->mbw * 8;
    const uint8_t* sy = a->Y + (size_t)f * a->ysz + (size_t)mby * 16 * ys + mbx * 16;
    MbFetch r;
    r.y = *(const uint32_t*)(sy + (size_t)(lane >> 2) * ys + (lane & 3) * 4);
    r.c = 0;
    if (lane < 32) {
        const int pl = lane >> 4, k = lane & 15;
        const uint8_t* sp = (pl ? a->V : a->U) + (size_t)f * a->csz + (size_t)mby * 8 * cs + mbx * 8;
        r.c = *(const uint32_t*)(sp + (size_t)(k >> 1) * cs + (k & 1) * 4);
    }
    r.alpha = a->alpha[(size_t)f * a->mbw * a->mbh + (size_t)mby * a->mbw + mbx];
    return r;
}

__device__ void setup_ctx(Ctx& C, const EncArgs* a, const uint8_t* seg_lut, WaveLds* W, int mbx, int mby,
                          const MbFetch& m)
{
    C.mbx = mbx;
    C.mby = mby;
    const int f = C.f;
    C.ys = a->mbw * 16;
    C.cs = a->mbw * 8;
    C.srcY = a->Y + (size_t)f * a->ysz + (size_t)mby * 16 * C.ys + mbx * 16;
    C.srcU = a->U + (size_t)f * a->csz + (size_t)mby * 8 * C.cs + mbx * 8;
    C.srcV = a->V + (size_t)f * a->csz + (size_t)mby * 8 * C.cs + mbx * 8;
    // stage the source MB in LDS: 64 lanes x 4 B luma, 32 lanes x 4 B chroma
    {
        const int l = C.lane;
        ((uint32_t*)C.M->sy)[l] = m.y;
        if (l < 32) ((uint32_t*)((l >> 4) ? C.M->sv : C.M->su))[l & 15] = m.c;
        C.sY = C.M->sy;
        C.sU = C.M->su;
        C.sV = C.M->sv;
    }
    wsync();
    // wave-uniform: the segment's matrices / lambdas / sharpening come from LDS;
    // seg_lut is the k-means alpha -> segment map (all zero without segments)
    const int seg = __builtin_amdgcn_readfirstlane((int)seg_lut[m.alpha]);
    C.seg = seg;
    C.S = C.Sl + seg;
}

__device__ void wait_row(const int* progress, int wave_of_prev, int need)
{
    while (__hip_atomic_load(&progress[wave_of_prev], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need)
        __builtin_amdgcn_s_sleep(1);
}
// s_setprio with a wave-uniform level
DI void set_prio(int p)
{
    if (p >= 3) __builtin_amdgcn_s_setprio(3);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
__device__ void publish(int* progress, int wave, int val)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(&progress[wave], val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_wave_barrier();
}


// The lane id as a value the compiler cannot prove loop-invariant.  Taken at
// the top of every MB iteration, it keeps lane-derived constants (per-lane
// offsets, 64-bit source pointers, table indices) from being hoisted out of
// the MB loops and held -- or spilled -- across them: they are cheap to
// recompute and the registers go to the search stages.
__device__ __forceinline__ int opaque_lane(int lane)
{
    asm volatile("" : "+v"(lane));
    return lane;
}

// ---------------------------------------------------------------------------
// Row-parallel encode (small batches, single frames): one wave per workgroup,
// MB rows handed out by a per-frame ticket, the row-to-row state (top_y, and in
// pass 2 top_u/v, top_c, top_derr) and the progress counters in global memory.
// A wave only waits for a row whose ticket an already running wave holds, so
// the grid cannot deadlock whatever the residency.  Hand-off: every byte of the
// row state is stored sc1 (write-through) and drained (vmcnt(0)) before the
// sc1 progress store; the consumer polls progress with sc1 loads and reads the
// bytes with sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility).
// Pass 1's chroma raster chain (quirk A5) runs in workgroup 0 of each frame,
// with its top_u/v/derr in its own LDS, as in the batch kernels.
// ---------------------------------------------------------------------------
struct RowsLayout {
    size_t sync, ty, tu, tv, tc, td, frame;
    __host__ __device__ RowsLayout(int mbw, int mbh)
    {
        auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        sync = 0;                                  // int [4 + mbh]: ticket, pad x3, done MBs per row
        ty = a16(4 * (4 + (size_t)mbh));
        tu = ty + a16((size_t)mbw * 16 + 16);
        tv = tu + a16((size_t)mbw * 8);
        tc = tv + a16((size_t)mbw * 8);
        td = tc + a16((size_t)mbw * 12);
        frame = td + a16((size_t)mbw * 4);
    }
};
#define ZW_ROWS_HDR 256  // launch header: [0] error word (a wave gave up waiting)
#define ZW_ENC_SPIN_MAX (1 << 22)
DI uint32_t ld_sc1(const void* p) { return __hip_atomic_load((const uint32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DI void st_sc1(void* p, uint32_t v) { __hip_atomic_store((uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DI int row_ticket(int* ticket)
{
    int t = 0;
    if ((threadIdx.x & 63) == 0) t = atomicAdd(ticket, 1);
    return __builtin_amdgcn_readfirstlane(__shfl(t, 0));
}
// Wait until *prog >= need; seen caches the last value read (the row above
// usually runs ahead, so most waits cost no memory round trip).  After
// ZW_ENC_SPIN_MAX polls, or once another wave gave up, report through *err.
DI void row_wait(const int* prog, int need, int* err, int& seen)
{
    if (seen >= need) return;
    int it = 0;
    for (;;) {
        seen = __builtin_amdgcn_readfirstlane((int)ld_sc1(prog));
        if (seen >= need) break;
        __builtin_amdgcn_s_sleep(1);
        if (++it > ZW_ENC_SPIN_MAX || ((it & 1023) == 0 && ld_sc1(err))) {
            if ((threadIdx.x & 63) == 0) atomicOr(err, 1);
            seen = 1 << 30;
            break;
        }
    }
    // pairs with row_publish's release: the row state loads below may not be
    // hoisted above the poll (C++ memory model, not only GFX9's in-order returns)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
DI void row_publish(int* prog, int val)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's sc1 stores are out
    if ((threadIdx.x & 63) == 0)
        __hip_atomic_store((uint32_t*)prog, (uint32_t)val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_wave_barrier();
}

// Pass 1's chroma chain: two waves in the row-parallel kernels (the quad form,
// one wave per plane), one in the batch kernels (the pair form).  The two-wave
// chain bounds the row-parallel pass 1 (one 1080p frame: 27.7 -> 22.1 ms), and
// those pass-1 workgroups then run two waves (the chain's two planes; two luma
// rows elsewhere).  In the batch kernels a second chain wave costs a luma wave
// and measured slower (34.4 -> 35.0 ms per 256 1080p frames).
template <bool ROWS> struct ChainShape {
    static constexpr int NCH = ROWS ? 2 : 1;
};
template <int PASS> struct RowsShape {
    static constexpr int NW = PASS == 1 ? ChainShape<true>::NCH : 1;
};
// The waves of one encode kernel.
template <int PASS, bool ROWS, int FP> struct EncShape {
    static_assert(FP == 1 || (FP == 2 && !ROWS), "frame pairs: the batch kernels");
    static constexpr bool PAIR = FP == 2;  // frame pairs: the workgroup encodes frames f and f + 1
    static constexpr int NW = ROWS ? RowsShape<PASS>::NW : PassShape<PASS>::NW, WG = NW * 64;
    static constexpr int NCH = PASS == 1 ? ChainShape<ROWS>::NCH : 0;  // chain waves (pass 1)
    // pass 1's chroma chain waves: in frame pairs one per frame (the one-wave
    // form), else NCH (the quad form's two waves in the row kernels)
    static constexpr int NCW = PASS == 1 ? (PAIR ? 2 : NCH) : 0;
};

constexpr size_t a16(size_t v) { return (v + 15) & ~(size_t)15; }

// The dynamic LDS of an encode workgroup: the sizes of its regions and, in
// map(), their order.  The kernel takes every region pointer from map() and
// the host takes its end (bytes(): the launch's size, the widest encodable
// frame, whether frame pairs fit), so a region cannot be sized and not carved,
// or carved and not sized.  Per frame of the workgroup: the tables (sT), the
// frame's 4 segments (sS), the alpha map (sL) and the top rows (sy, su, sv, sc,
// sd); per wave: WaveLds (sW) and, in frame pairs, a second MbLds (sM); then
// the progress words and the two-wave chroma chain's exchange words.
//
// Of the frame-wide row arrays (top_y, top_u, top_v, top_c, top_derr) the batch
// kernels (one workgroup per frame) keep all; in the row-parallel kernels the
// luma waves work from per-MB windows of the global row state, and only pass
// 1's chroma chain keeps top_u / top_v / top_derr, so their LDS no longer grows
// with the width (which is what bounded the encodable width:
// zwk_encode_max_mbw, 1 560 MBs with the batch shapes, any u16 width here).
struct EncLds {
    static constexpr size_t sT = a16(sizeof(LdsTables)), sS = a16(4 * sizeof(ZwSegment)), sL = 256;
    static constexpr size_t sW = a16(sizeof(WaveLds)), sM = a16(sizeof(MbLds));
    size_t sy, su, sv, sc, sd;  // the top-row arrays
    static constexpr size_t sProgress = 64, sXch = 256;
    __host__ __device__ EncLds(int mbw, bool rows, int pass)
    {
        const bool all = !rows, chain = rows && pass == 1;
        sy = all ? (((size_t)mbw * 16 + 48 + 15) & ~(size_t)15) : 0;
        su = sv = all || chain ? (((size_t)mbw * 8 + 48 + 15) & ~(size_t)15) : 0;
        sc = all ? (((size_t)mbw * 12 + 15) & ~(size_t)15) : 0;
        sd = all || chain ? (((size_t)mbw * 4 + 15) & ~(size_t)15) : 0;
    }
    // Byte offset of every region (of its first frame's or wave's share) and the end.
    struct Map {
        size_t T, S, lut, W, M2, progress, xch, top_y, top_u, top_v, top_c, top_derr, end;
    };
    __host__ __device__ Map map(int nw, int fp) const
    {
        Map m;
        size_t o = 0;
        auto region = [&o](size_t n) {
            const size_t at = o;
            o += n;
            return at;
        };
        m.T = region(sT * fp);
        m.S = region(sS * fp);
        m.lut = region(sL * fp);
        m.W = region(sW * nw);
        m.M2 = region(fp == 2 ? sM * nw : 0);
        m.progress = region(sProgress);
        m.xch = region(sXch);
        m.top_y = region(sy * fp);
        m.top_u = region(su * fp);
        m.top_v = region(sv * fp);
        m.top_c = region(sc * fp);
        m.top_derr = region(sd * fp);
        m.end = o;
        return m;
    }
    __host__ __device__ size_t bytes(int nw, int fp) const { return map(nw, fp).end; }
};
static_assert(NW_MAX * sizeof(int) <= 64, "the progress words");

// What the waves of a workgroup share: the launch, the carved LDS (of the
// per-frame regions the first frame's share: frame_lds steps to a frame), the
// wave's own LDS and, in the row-parallel kernels, the frame's row state in
// global memory.
struct EncWg {
    const EncArgs* a;
    const EncLds L;
    int f, nf;  // the workgroup's first frame and its frames (frame pairs: 2, the odd last workgroup 1)
    int wv;
    LdsTables* T;
    ZwSegment* Sl;     // the frame's 4 segments (matrices, lambdas, sharpening)
    uint8_t* seg_lut;  // alpha -> segment (zeros when segmentation is off)
    WaveLds* W;
    MbLds* M2;         // frame pairs: the wave's per-MB state of the second frame
    int* progress;
    int *xch, *xflag;  // two-wave chroma chain: [plane][2][12] exchange words, then 2 flags
    uint8_t *top_y, *top_u, *top_v;
    uint8_t* top_c;    // [mbw][12]: y2, y[4], u[2], v[2]
    int8_t* top_derr;  // [mbw][4]
    // row-parallel kernels: the launch's error word, the frame's ticket and
    // progress words and its row arrays (RowsLayout)
    int *rerr, *rsync;
    uint8_t *gty, *gtu, *gtv, *gtc, *gtd;
    __device__ EncWg(const EncArgs& a_, bool rows, int pass) : a(&a_), L(a_.mbw, rows, pass) {}
};

template <int PASS, bool ROWS, int FP> DI EncWg enc_carve(const EncArgs& a, uint8_t* smem)
{
    using SH = EncShape<PASS, ROWS, FP>;
    EncWg G(a, ROWS, PASS);
    const EncLds::Map at = G.L.map(SH::NW, FP);
    G.f = ROWS ? blockIdx.y : blockIdx.x * FP;
    G.nf = SH::PAIR ? min(2, a.nframes - G.f) : 1;
    G.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    G.T = (LdsTables*)(smem + at.T);
    G.Sl = (ZwSegment*)(smem + at.S);
    G.seg_lut = smem + at.lut;
    G.W = (WaveLds*)(smem + at.W + G.L.sW * G.wv);
    G.M2 = (MbLds*)(smem + at.M2) + G.wv;
    G.progress = (int*)(smem + at.progress);
    G.xch = (int*)(smem + at.xch);
    G.xflag = G.xch + 48;
    G.top_y = smem + at.top_y;
    G.top_u = smem + at.top_u;
    G.top_v = smem + at.top_v;
    G.top_c = smem + at.top_c;
    G.top_derr = (int8_t*)(smem + at.top_derr);
    const RowsLayout RL(a.mbw, a.mbh);
    uint8_t* rb = ROWS ? a.rows + ZW_ROWS_HDR + (size_t)G.f * RL.frame : nullptr;
    G.rerr = ROWS ? (int*)a.rows : nullptr;
    G.rsync = (int*)rb;
    G.gty = ROWS ? rb + RL.ty : nullptr;
    G.gtu = ROWS ? rb + RL.tu : nullptr;
    G.gtv = ROWS ? rb + RL.tv : nullptr;
    G.gtc = ROWS ? rb + RL.tc : nullptr;
    G.gtd = ROWS ? rb + RL.td : nullptr;
    return G;
}

// One frame's share of the workgroup's LDS, and the frame's settings.
struct FrameLds {
    LdsTables* T;
    ZwSegment* Sl;
    uint8_t* seg_lut;
    uint8_t *top_y, *top_u, *top_v, *top_c;
    int8_t* top_derr;
    const ZwFrameParams* P;
    int f;       // frame of the launch
    int method;  // per-frame encoder settings (a launch's frames normally share them)
    bool trel;
    // without trellis (and without the pass-2 I4 dump) the final I4 blocks are
    // the search's winners, which the search leaves in C.M->lev / C.M->ws
    bool keep_i4;
};
// Share fr of the workgroup.  (The odd last workgroup of a pair launch has a
// second share and no second frame: that share carries the first frame's
// number and settings, and nothing is encoded from it.)
template <int PASS> DI FrameLds frame_lds(const EncWg& G, int fr)
{
    const EncLds& L = G.L;
    FrameLds F;
    F.T = (LdsTables*)((uint8_t*)G.T + L.sT * fr);
    F.Sl = (ZwSegment*)((uint8_t*)G.Sl + L.sS * fr);
    F.seg_lut = G.seg_lut + L.sL * fr;
    F.top_y = G.top_y + L.sy * fr;
    F.top_u = G.top_u + L.su * fr;
    F.top_v = G.top_v + L.sv * fr;
    F.top_c = G.top_c + L.sc * fr;
    F.top_derr = G.top_derr + L.sd * fr;
    F.f = G.f + (fr < G.nf ? fr : 0);
    F.P = G.a->params + F.f;
    F.method = __builtin_amdgcn_readfirstlane(F.P->method);
    F.trel = PASS == 2 && __builtin_amdgcn_readfirstlane(F.P->do_trellis);
    F.keep_i4 = !F.trel && (PASS == 1 || G.a->dbg == nullptr);
    return F;
}
// Point C at MB (mbx, mby) of that frame; M: the wave's per-MB state for it.
DI void ctx_enter(Ctx& C, const FrameLds& F, MbLds* M, int mbx, int mby)
{
    C.f = F.f;
    C.P = F.P;
    C.T = F.T;
    C.Sl = F.Sl;
    C.top_y = F.top_y;
    C.top_u = F.top_u;
    C.top_v = F.top_v;
    C.top_c = F.top_c;
    C.top_derr = F.top_derr;
    C.M = M;
    C.method = F.method;
    C.mbx = mbx;
    C.mby = mby;
    C.oy = mbx * 16;
    C.oc = mbx * 8;
    C.ocx = mbx * 12;
    C.od = mbx * 4;
    C.sY = M->sy;
    C.sU = M->su;
    C.sV = M->sv;
}

// Fill the workgroup's shared state (each of its frames), then barrier.
template <int PASS, bool ROWS, int FP> DI void enc_fill(const EncWg& G, bool chain_wg)
{
    constexpr int NW = EncShape<PASS, ROWS, FP>::NW, WG = NW * 64;
    const EncArgs& a = *G.a;
    const int mbw = a.mbw;
#pragma unroll
    for (int fr = 0; fr < FP; fr++) {
        if (fr >= G.nf) break;
        const FrameLds F = frame_lds<PASS>(G, fr);
        const int ff = F.f;
        const ZwFrameParams* Pf = F.P;
        LdsTables* Tf = F.T;
        for (int i = threadIdx.x; i < (int)(sizeof(Tf->lc) / 2); i += WG)
            (&Tf->lc[0][0][0][0])[i] = a.lcost ? (&a.lcost[ff].lc[0][0][0][0])[i] : 0;
        for (int i = threadIdx.x; i < 96; i += WG) {
            (&Tf->eob[0][0][0])[i] = a.lcost ? (&a.lcost[ff].eob[0][0][0])[i] : 0;
            (&Tf->init[0][0][0])[i] = a.lcost ? (&a.lcost[ff].init[0][0][0])[i] : 0;
        }
        for (int i = threadIdx.x; i < 4 * 8 * 3 * 11; i += WG) (&Tf->probs[0][0][0][0])[i] = (&Pf->probs[0][0][0][0])[i];
        static_assert(sizeof(ZwSegment) % 4 == 0, "segment copy by dwords");
        for (int i = threadIdx.x; i < (int)(4 * sizeof(ZwSegment) / 4); i += WG)
            ((uint32_t*)F.Sl)[i] = ((const uint32_t*)Pf->seg)[i];
        for (int i = threadIdx.x; i < 256; i += WG) F.seg_lut[i] = Pf->seg_enabled ? Pf->seg_map_lut[i] : 0;
        load_static_tables(Tf, threadIdx.x, WG, &Pf->probs[0][0][0][0]);
        if (!ROWS || chain_wg) {
            if (!ROWS) {
                for (int i = threadIdx.x; i < mbw * 16 + 48; i += WG) F.top_y[i] = 127;
                for (int i = threadIdx.x; i < mbw * 12; i += WG) F.top_c[i] = 0;
            }
            for (int i = threadIdx.x; i < mbw * 8 + 48; i += WG) {
                F.top_u[i] = 127;
                F.top_v[i] = 127;
            }
            for (int i = threadIdx.x; i < mbw * 4; i += WG)
                F.top_derr[i] = PASS == 2 ? a.derr[(size_t)ff * mbw * 4 + i] : 0;
        }
    }
    if (threadIdx.x < NW) G.progress[threadIdx.x] = -1;
    if (threadIdx.x < 2) G.xflag[threadIdx.x] = 0;
    if (ROWS && (threadIdx.x & 63) < 12) G.W->win_c[threadIdx.x & 63] = 0;  // pass 1: the complexity contexts stay zero
    __syncthreads();
}

// Profiling builds: the wave's phase counters, cleared at the start of the
// kernel and added to the global ones once at its end.
DI void ph_init(const EncWg& G, int lane)
{
#ifdef ZW_PHASE_PROF
    if (lane < ZW_PH_N) G.W->ph[lane] = 0;
    wsync();
#endif
}
template <int PASS> DI void ph_flush(const EncWg& G, int lane)
{
#ifdef ZW_PHASE_PROF
    if (lane < ZW_PH_N) atomicAdd(&zw_phase_cycles_dev[PASS - 1][lane], G.W->ph[lane]);
    if (lane < ZW_PH_N) atomicAdd(&zw_wave_cycles_dev[PASS - 1][G.wv][lane], G.W->ph[lane]);
#endif
}

// A wave starts an MB row: the left borders and contexts of its first MB.
DI void row_start(MbLds* M, int lane)
{
    if (lane < 20) M->left_y[lane] = 129;
    if (lane < 12) {
        M->left_u[lane] = 129;
        M->left_v[lane] = 129;
        M->left_c[lane] = 0;
    }
    if (lane < 4) M->left_derr[lane] = 0;
}

// Issue priority of a batch kernel's luma wave from its slack to the row above
// (which wave prevw works; none at row 0).  VALU issue is arbitrated by
// priority, then wave age: at equal priority the youngest waves of each SIMD
// run slowest and every row behind theirs waits on them (35 % of the oldest
// waves' time).  A row that trails the row above by more than the two-MB
// minimum is the one later rows wait for, so it issues first.
template <int PASS> DI void luma_issue_prio(const int* progress, int prevw, int mbx, int mby, int mbw)
{
#if ZW_DYN_PRIO > 0
    int slack = mbw;
    if (mby > 0) {
        const int v = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&progress[prevw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if ((v >> 16) == mby - 1) slack = (v & 0xffff) - mbx - 1;
    }
    constexpr int dp = PASS == 1 ? ZW_DYN_PRIO1 : ZW_DYN_PRIO;
    const int p = slack >= dp * 3 ? 3 : (slack >= dp * 2 ? 2 : (slack >= dp ? 1 : 0));
    set_prio(PASS == 1 ? min(p, ZW_P1_LUMA_MAX) : p);
#endif
}

// ---------------------------------------------------------------------------
// Everything of an MB after its searches, in three steps: the final luma
// transform, the final chroma transform (pass 2), and the stores.  What the
// transforms hand on is one word each: the blocks' has-coefficients flags
// (luma bits 0..15, chroma bits 0..7) and above them the simple-quant "any
// nonzero" flag (luma bit 16, chroma bit 8).
// ---------------------------------------------------------------------------
DI uint32_t mb_luma(Ctx& C, int lm, bool i4reuse, uint32_t i4nz, bool trel)
{
    int ynz[16];
    uint32_t r = (uint32_t)(final_luma(C, lm, trel, ynz, i4reuse ? (int)i4nz : -1) != 0) << 16;
#pragma unroll
    for (int k = 0; k < 16; k++) r |= (uint32_t)(ynz[k] != 0) << k;
    return r;
}
DI uint32_t mb_chroma(Ctx& C, int cm)
{
    int uvnz[8];
    uint32_t r = (uint32_t)(final_chroma(C, cm, C.top_derr + C.od, uvnz) != 0) << 8;
#pragma unroll
    for (int k = 0; k < 8; k++) r |= (uint32_t)(uvnz[k] != 0) << k;
    return r;
}
// the stores: the complexity contexts (pass 2), the levels, the MB record
// and the borders (the chroma borders only if the caller has not stored them)
template <int PASS> DI void mb_finish(Ctx& C, int lm, int cm, uint32_t lres, uint32_t cres, bool chroma_borders)
{
    const EncArgs& a = *C.a;
    const int lane = C.lane, mbw = a.mbw;
    const size_t nmb = (size_t)mbw * a.mbh;
    int ynz[16], uvnz[8];
#pragma unroll
    for (int k = 0; k < 16; k++) ynz[k] = (int)((lres >> k) & 1u);
#pragma unroll
    for (int k = 0; k < 8; k++) uvnz[k] = (int)((cres >> k) & 1u);
    const int lnz = (int)((lres >> 16) & 1u), cnz = (int)((cres >> 8) & 1u);
    ZwMbOut* o = a.out + (size_t)C.f * nmb + (size_t)C.mby * mbw + C.mbx;
    if (PASS == 2) {
        const int skip = !(lnz | cnz);
        // complexity (encode_residual_data semantics / skip clearing)
        if (lane == 0) {
            uint8_t* tc = C.top_c + C.ocx;
            uint8_t* lc = C.M->left_c;
            if (skip) {
                for (int k = 1; k < 9; k++) tc[k] = lc[k] = 0;
                if (lm != 4) tc[0] = lc[0] = 0;
            } else {
                if (lm != 4) {
                    int y2nz = 0;
                    for (int n = 0; n < 16; n++) y2nz |= C.M->lev[16][n] != 0;
                    tc[0] = lc[0] = (uint8_t)y2nz;
                }
                for (int x = 0; x < 4; x++) tc[1 + x] = (uint8_t)ynz[12 + x];
                for (int y = 0; y < 4; y++) lc[1 + y] = (uint8_t)ynz[y * 4 + 3];
                tc[5] = (uint8_t)uvnz[2];
                tc[6] = (uint8_t)uvnz[3];
                lc[5] = (uint8_t)uvnz[1];
                lc[6] = (uint8_t)uvnz[3];
                tc[7] = (uint8_t)uvnz[6];
                tc[8] = (uint8_t)uvnz[7];
                lc[7] = (uint8_t)uvnz[5];
                lc[8] = (uint8_t)uvnz[7];
            }
            o->skip = (uint8_t)skip;
            o->chroma_mode = (uint8_t)cm;
        }
        if (chroma_borders) store_chroma_borders(C);
        write_levels(C, 0, 25, skip);
        if (a.sizes) {
            // the packed record size k_pack_size would compute from these
            // levels: header, eob bytes and every block's levels up to its eob
            int e = 0;
            if (lane < 25 && !skip) {
                const uint32_t* lw = (const uint32_t*)C.M->lev[lane];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const uint32_t v = lw[q];
                    e = (v >> 16) ? 2 * q + 2 : ((v & 0xffffu) ? 2 * q + 1 : e);
                }
            }
            // lanes 0..24 hold the eobs: DPP sums per 16-lane row, rows 0 and 1 added
            const int r16 = red16(e);
            const int es = __builtin_amdgcn_readlane(r16, 0) + __builtin_amdgcn_readlane(r16, 16);
            if (lane == 0)
                a.sizes[(size_t)C.f * nmb + (size_t)C.mby * mbw + C.mbx] = (uint32_t)(1 + (lm == 4 ? 8 : 0) + 25 + 2 * es);
        }
    } else {
        write_levels(C, 0, 17, false);
        if (lane == 0) o->skip = 0;  // pass-1 skip is decided on the host from the levels
    }
    if (lane == 0) {
        o->luma_mode = (uint8_t)lm;
        o->segment = (uint8_t)C.seg;
    }
    if (lane < 16) o->bpred[lane] = lm == 4 ? C.M->modes[lane] : 0;
    store_luma_borders(C);
}
template <int PASS> DI void mb_store(Ctx& C, int lm, int cm, bool i4reuse, uint32_t i4nz, bool trel)
{
    [[maybe_unused]] const int lane = C.lane;
    PH_START();
    const uint32_t lres = mb_luma(C, lm, i4reuse, i4nz, trel);
    PH_MARK(4);
    const uint32_t cres = PASS == 2 ? mb_chroma(C, cm) : 0u;
    PH_MARK(5);
    mb_finish<PASS>(C, lm, cm, lres, cres, true);
}

// ---------------------------------------------------------------------------
// Pass 1's chroma raster chain, quad form (the row-parallel kernels): wave 0
// the U plane, wave 1 the V plane.
// ---------------------------------------------------------------------------
template <int PASS> DI void chain_quad(const EncWg& G, Ctx& C)
{
    const EncArgs& a = *G.a;
    const int mbw = a.mbw, mbh = a.mbh, f = G.f, lane = C.lane;
    const size_t nmb = (size_t)mbw * mbh;
    if (lane < 4) C.M->left_derr[lane] = 0;
    const int pl = __builtin_amdgcn_readfirstlane(G.wv);  // (wave-uniform: see luma_pairs)
    UvQ U;
    U.pl = pl;
    U.w = G.W->cu;
    U.sp = C.M->su;
    U.top = pl ? G.top_v : G.top_u;
    U.left = C.M->left_u;
    const uint8_t* const P0 = (pl ? a.V : a.U) + (size_t)f * a.csz;
    const int cs = mbw * 8;
    auto fetch_uv = [&](int mbx, int mby) {
        MbFetch r;
        r.y = lane < 16 ? *(const uint32_t*)(P0 + (size_t)(mby * 8 + (lane >> 1)) * cs + mbx * 8 + (lane & 1) * 4) : 0u;
        r.c = 0;
        r.alpha = a.alpha[(size_t)f * nmb + (size_t)mby * mbw + mbx];
        return r;
    };
    C.ys = mbw * 16;
    C.cs = cs;
    MbFetch nx = fetch_uv(0, 0);
    int seq = 0;
    for (int mby = 0; mby < mbh; mby++) {
        if (lane < 12) C.M->left_u[lane] = 129;
        wsync();
        for (int mbx = 0; mbx < mbw; mbx++) {
            PH_START();
            const int lane = opaque_lane(threadIdx.x & 63);
            C.lane = lane;
            const MbFetch cur = nx;
            if (mbx + 1 < mbw) nx = fetch_uv(mbx + 1, mby);
            else if (mby + 1 < mbh) nx = fetch_uv(0, mby + 1);
            C.mbx = mbx;
            C.mby = mby;
            if (lane < 16) ((uint32_t*)C.M->su)[lane] = cur.y;
            wsync();
            const int seg = __builtin_amdgcn_readfirstlane((int)G.seg_lut[cur.alpha]);
            C.seg = seg;
            C.S = C.Sl + seg;
            uvq_border(C, U);
            const int cm = uvq_pick(C, U, G.xch, G.xflag, ++seq);
            PH_MARK(8);
            uvq_final(C, U, cm, G.top_derr + mbx * 4);
            PH_MARK(9);
            uvq_store_borders(C, U);
            ZwMbOut* o = a.out + (size_t)f * nmb + (size_t)mby * mbw + mbx;
            if (pl == 0 && lane == 0) o->chroma_mode = (uint8_t)cm;
            write_levels(C, 17 + 4 * pl, 4, false);
            wsync();
        }
    }
    for (int i = lane; i < mbw * 2; i += 64) {
        const int j = (i >> 1) * 4 + pl * 2 + (i & 1);
        a.derr[(size_t)f * mbw * 4 + j] = G.top_derr[j];
    }
}

// ---------------------------------------------------------------------------
// Pass 1's chroma raster chain, one-wave form (the batch kernels).  In frame
// pairs chain wave k works frame f + k, and returns to take luma rows
// (PairRowSchedule1, from the join row on).
// ---------------------------------------------------------------------------
template <int PASS, int FP> DI void chain_one(const EncWg& G, Ctx& C)
{
    const EncArgs& a = *G.a;
    const int mbw = a.mbw, mbh = a.mbh, lane = C.lane;
    const size_t nmb = (size_t)mbw * mbh;
    const int cfr = FP == 2 ? G.wv : 0;
    // (the odd last workgroup of a pair launch: chain wave 1 has no frame,
    // only its luma rows; it runs no chain row)
    const bool has_chain = cfr < G.nf;
    const FrameLds F = frame_lds<PASS>(G, cfr);
    ctx_enter(C, F, &G.W->mb, 0, 0);
    if (lane < 4) C.M->left_derr[lane] = 0;
    MbFetch nx = fetch_mb(&a, F.f, lane, 0, 0);
    for (int mby = 0; has_chain && mby < mbh; mby++) {
        if (lane < 12) {
            C.M->left_u[lane] = 129;
            C.M->left_v[lane] = 129;
        }
        wsync();
        for (int mbx = 0; mbx < mbw; mbx++) {
            PH_START();
            const int lane = opaque_lane(threadIdx.x & 63);
            C.lane = lane;
            const MbFetch cur = nx;
            if (mbx + 1 < mbw) nx = fetch_mb(&a, F.f, lane, mbx + 1, mby);
            else if (mby + 1 < mbh) nx = fetch_mb(&a, F.f, lane, 0, mby + 1);
            setup_ctx(C, &a, F.seg_lut, G.W, mbx, mby, cur);
            C.oc = mbx * 8;
            C.ocx = mbx * 12;
            build_chroma_border(C);
            const int cm = pick_uv<PASS>(C);
            PH_MARK(8);
            int uvnz[8];
            final_chroma(C, cm, F.top_derr + mbx * 4, uvnz);
            PH_MARK(9);
            store_chroma_borders(C);
            ZwMbOut* o = a.out + (size_t)F.f * nmb + (size_t)mby * mbw + mbx;
            if (lane == 0) o->chroma_mode = (uint8_t)cm;
            write_levels(C, 17, 8, false);
            wsync();
        }
    }
    for (int i = lane; has_chain && i < mbw * 4; i += 64) a.derr[(size_t)F.f * mbw * 4 + i] = F.top_derr[i];
}

// Both frames' Ctx for a stage that works MB (mbx, mby) of the two frames in
// one pass of the wave (pick_i4_pair, final_luma_pair); seg0, seg1: the MBs'
// segments.
DI void ctx_pair(const Ctx& C, const FrameLds& F0, const FrameLds& F1, MbLds* const Mp[2], int mbx, int mby, int seg0,
                 int seg1, Ctx& CA, Ctx& CB)
{
    CA = CB = C;
    CA.lane = CB.lane = opaque_lane(threadIdx.x & 63);
    ctx_enter(CA, F0, Mp[0], mbx, mby);
    ctx_enter(CB, F1, Mp[1], mbx, mby);
    CA.seg = seg0;
    CB.seg = seg1;
    CA.S = CA.Sl + seg0;
    CB.S = CB.Sl + seg1;
}

// ---------------------------------------------------------------------------
// The luma wavefront of frame pairs: every wave works MB row y of both frames
// of the workgroup (which wave takes which row: RP below; in pass 1 the chain
// waves arrive here after their chains and take rows from the join row on), MB
// (x, y) of frame 0 and of frame 1 per iteration.  Both frames' rows advance
// together, so one progress word per wave serves both.  The two MBs' I4
// searches run in one wave (pick_i4_pair): lanes 0..31 frame 0, lanes 32..63
// frame 1.  The other per-MB stages run in loops over the frames, and what an
// MB's stages hand on goes through LDS (W->pst), not registers.
//
// The loops over the frames are unrolled: each stage is emitted twice, with a
// constant frame index (as a two-trip loop, one copy of the code, pass 2
// measured 30.26 against 29.80 ms per 256 1080p frames, pass 1 the same).
// ---------------------------------------------------------------------------
template <int PASS, int NW, int NCW> DI void luma_pairs(const EncWg& G, Ctx& C)
{
    const EncArgs& a = *G.a;
    WaveLds* const W = G.W;
    int* const progress = G.progress;
    const int mbw = a.mbw, mbh = a.mbh, lane = C.lane;
    // (wave-uniform, and said to be: a role is compiled as a function of its
    // own before it becomes part of the kernel, and what it reads through G is
    // then not known to be uniform; the frame count, the wave, its row and the
    // wave of the row above steer every wait and otherwise end up in VGPRs)
    const int nf = __builtin_amdgcn_readfirstlane(G.nf), wv = __builtin_amdgcn_readfirstlane(G.wv);
    const FrameLds F[2] = {frame_lds<PASS>(G, 0), frame_lds<PASS>(G, 1)};
    MbLds* const Mp[2] = {&W->mb, G.M2};
    const int K = F[0].method <= 3 ? 3 : (F[0].method == 4 ? 4 : 10);
    const bool same_k = nf == 1 || (F[1].method == F[0].method && F[1].trel == F[0].trel);
    // pass 2: the waves take the rows in turn; pass 1: fewer rows for the
    // luma waves beside a chain, and from the join row on the chain waves'
    // too (PairRowSchedule1)
    using RP = typename std::conditional<PASS == 1, PairRowSchedule1<NW, NCW>, RowSchedule<PASS, false, NW, NCW, true>>::type;
    for (int mby = RP::first_row(wv, mbh); mby < mbh; mby = RP::next_row(wv, mby, mbh)) {
#pragma unroll
        for (int fr = 0; fr < 2; fr++) row_start(Mp[fr], lane);
        wsync();
        const int prevw = __builtin_amdgcn_readfirstlane(mby > 0 ? RP::wave_of_row(mby - 1, mbh) : 0);
        auto wait_above = [&](int need) {
            if (mby > 0) wait_row(progress, prevw, (mby - 1) * 65536 + need);
        };
        for (int mbx = 0; mbx < mbw; mbx++) {
            PH_START();
            const int lane = opaque_lane(threadIdx.x & 63);
            C.lane = lane;
            // point C at frame fr's MB (x, y)
            auto enter = [&](int fr) {
                // a fresh opaque lane per MB stage: lane-derived constants are
                // recomputed, not held across the other frame's stages
                C.lane = opaque_lane(threadIdx.x & 63);
                ctx_enter(C, F[fr], Mp[fr], mbx, mby);
            };
            auto pst = [&](int fr, int k) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)W->pst[fr][k]); };
            // the MB's segment and its Ctx fields, from the search's word
            auto enter_seg = [&](int fr, uint32_t sm) {
                enter(fr);
                C.seg = (int)(sm >> 8);
                C.S = C.Sl + C.seg;
            };
            wait_above(min(mbx + 1, mbw));
            luma_issue_prio<PASS>(progress, prevw, mbx, mby, mbw);
            PH_MARK(0);
#pragma unroll
            for (int fr = 0; fr < 2; fr++) {
                if (fr >= nf) {
                    if (lane == 0) W->pst[fr][0] = 0;  // (no frame 1: no search)
                    continue;
                }
                enter(fr);
                const MbFetch fm = fetch_mb(&a, C.f, lane, mbx, mby);
                setup_ctx(C, &a, F[fr].seg_lut, W, mbx, mby, fm);
                build_luma_border(C, 0);
                int l_;
                unsigned long long s_;
                pick_i16<PASS>(C, l_, s_);
                const bool n_ = C.method > 1 && (C.method >= 5 || s_ > 211ull * C.S->l_mode || l_ != 0);
                if (lane == 0) {
                    W->pst[fr][0] = (uint32_t)l_ | ((uint32_t)n_ << 4) | ((uint32_t)C.seg << 8);
                    W->pst[fr][1] = (uint32_t)s_;
                    W->pst[fr][2] = (uint32_t)(s_ >> 32);
                    W->pst[fr][3] = 0;
                }
                wsync();
            }
            wsync();
            PH_MARK(1);
            const uint32_t s0 = pst(0, 0), s1 = pst(1, 0);
            const bool n0 = (s0 >> 4) & 1u, n1 = (s1 >> 4) & 1u;
            if (n0 || n1) wait_above(min(mbx + 2, mbw));
#pragma unroll
            for (int fr = 0; fr < 2; fr++) {
                if (!((pst(fr, 0) >> 4) & 1u)) continue;
                enter(fr);
                build_luma_border(C, 1);
            }
            PH_MARK(21);
            if (K <= 4 && same_k && (n0 || n1)) {
                Ctx CA, CB;
                ctx_pair(C, F[0], F[1], Mp, mbx, mby, (int)(s0 >> 8), (int)(s1 >> 8), CA, CB);
                const unsigned long long i0 = pst(0, 1) | ((unsigned long long)pst(0, 2) << 32);
                const unsigned long long i1 = pst(1, 1) | ((unsigned long long)pst(1, 2) << 32);
                uint32_t z0 = 0, z1 = 0;
                const uint32_t r = pick_i4_pair<PASS>(CA, CB, i0, i1, n0, n1, F[0].keep_i4, z0, z1);
                if (lane == 0) {
                    W->pst[0][3] = (r & 1u) ? (z0 | 0x10000u) : 0u;
                    W->pst[1][3] = (r & 2u) ? (z1 | 0x10000u) : 0u;
                }
            } else if (n0 || n1) {
#pragma unroll
                for (int fr = 0; fr < 2; fr++) {
                    const uint32_t sm = pst(fr, 0);
                    if (!((sm >> 4) & 1u)) continue;
                    enter_seg(fr, sm);
                    uint32_t z = 0;
                    const bool w4 =
                        pick_i4<PASS>(C, pst(fr, 1) | ((unsigned long long)pst(fr, 2) << 32), F[fr].keep_i4, z);
                    if (lane == 0) W->pst[fr][3] = w4 ? (z | 0x10000u) : 0u;
                }
            }
            wsync();
            PH_MARK(2);
            // The final stage.  Chroma first, frame by frame (pass 2; in pass 1
            // the chain waves work it): W->uvc, cu and cv are the wave's, so a
            // frame's final chroma and chroma borders are done before the other
            // frame's search.  Its result replaces the I16 score in W->pst.
            if (PASS == 2) {
#pragma unroll
                for (int fr = 0; fr < 2; fr++) {
                    if (fr >= nf) continue;
                    enter_seg(fr, pst(fr, 0));
                    build_chroma_border(C);
                    const int cm = pick_uv<PASS>(C);
                    PH_MARK(3);
                    const uint32_t cres = mb_chroma(C, cm);
                    store_chroma_borders(C);
                    if (lane == 0) W->pst[fr][1] = cres | ((uint32_t)cm << 9);
                    PH_MARK(5);
                }
            }
            // Luma: two I16 MBs in one pass of the wave (final_luma_pair),
            // anything else (an I4 MB, the odd last workgroup, frames whose
            // trellis settings differ) frame by frame.
            const uint32_t w0 = pst(0, 3), w1 = pst(1, 3);
            if (nf == 2 && !((w0 | w1) & 0x10000u) && F[0].trel == F[1].trel) {
                Ctx CA, CB;
                ctx_pair(C, F[0], F[1], Mp, mbx, mby, (int)(s0 >> 8), (int)(s1 >> 8), CA, CB);
                uint32_t r0, r1;
                final_luma_pair(CA, CB, (int)(s0 & 15u), (int)(s1 & 15u), F[0].trel, r0, r1);
                if (lane == 0) {
                    W->pst[0][2] = r0;
                    W->pst[1][2] = r1;
                }
            } else {
#pragma unroll
                for (int fr = 0; fr < 2; fr++) {
                    if (fr >= nf) continue;
                    const uint32_t sm = pst(fr, 0), r4 = pst(fr, 3);
                    enter_seg(fr, sm);
                    const bool w4 = (r4 >> 16) & 1u;
                    const uint32_t lres =
                        mb_luma(C, w4 ? 4 : (int)(sm & 15u), w4 && F[fr].keep_i4, r4 & 0xffffu, F[fr].trel);
                    if (lane == 0) W->pst[fr][2] = lres;
                }
                if (nf == 2) PH_COUNT(26);
            }
            wsync();
            PH_MARK(4);
            // the stores, frame by frame
#pragma unroll
            for (int fr = 0; fr < 2; fr++) {
                if (fr >= nf) continue;
                const uint32_t sm = pst(fr, 0), r4 = pst(fr, 3), cr = pst(fr, 1);
                enter_seg(fr, sm);
                const bool w4 = (r4 >> 16) & 1u;
                mb_finish<PASS>(C, w4 ? 4 : (int)(sm & 15u), PASS == 2 ? (int)(cr >> 9) : 0, pst(fr, 2),
                                PASS == 2 ? cr & 0x1ffu : 0u, false);
            }
            PH_RESET();
            publish(progress, wv, mby * 65536 + mbx + 1);
            PH_MARK(6);
        }
    }
}

// ---------------------------------------------------------------------------
// The row-parallel window: an MB's slice of the row above's state, pulled from
// the frame's global row arrays before the MB and pushed (the MB's own bottom
// row and contexts, for the row below) after it.  Which lane moves which word:
// lanes 0-3 top_y, and in pass 2 (pass 1's luma waves keep only top_y) 4-5
// top_u, 6-7 top_v, 8-10 top_c, 11 top_derr.  op(global word, window word).
// ---------------------------------------------------------------------------
template <int PASS, class Op> DI void win_words(const EncWg& G, int lane, int mbx, Op op)
{
    WaveLds* const W = G.W;
    if (lane < 4) op(G.gty + mbx * 16 + 4 * lane, (uint32_t*)W->win_y + lane);
    else if (PASS == 2 && lane < 6) op(G.gtu + mbx * 8 + 4 * (lane - 4), (uint32_t*)W->win_u + (lane - 4));
    else if (PASS == 2 && lane < 8) op(G.gtv + mbx * 8 + 4 * (lane - 6), (uint32_t*)W->win_v + (lane - 6));
    else if (PASS == 2 && lane < 11) op(G.gtc + mbx * 12 + 4 * (lane - 8), (uint32_t*)W->win_c + (lane - 8));
    else if (PASS == 2 && lane < 12) op(G.gtd + mbx * 4, (uint32_t*)W->win_d);
}
template <int PASS> DI void win_pull(const EncWg& G, int lane, int mbx)
{
    // (every load, then the stores: the arrays' loads are in flight together)
    uint32_t v = 0;
    win_words<PASS>(G, lane, mbx, [&v](const uint8_t* g, uint32_t*) { v = ld_sc1(g); });
    win_words<PASS>(G, lane, mbx, [v](const uint8_t*, uint32_t* w) { *w = v; });
}
// the above-right MB's bottom row (luma only: the I4 search reads it), behind the MB's own
DI void win_pull_right(const EncWg& G, int lane, int mbx)
{
    win_words<1>(G, lane, mbx + 1, [](const uint8_t* g, uint32_t* w) { w[4] = ld_sc1(g); });
}
template <int PASS> DI void win_push(const EncWg& G, int lane, int mbx)
{
    win_words<PASS>(G, lane, mbx, [](uint8_t* g, const uint32_t* w) { st_sc1(g, *w); });
}

// ---------------------------------------------------------------------------
// The luma wavefront of the one-frame batch kernels (rows dealt to the waves by
// RowSchedule, progress in LDS) and of the row-parallel kernels (rows by
// ticket, progress and the row above's state in global memory).
// ---------------------------------------------------------------------------
template <int PASS, bool ROWS, int NW, int NCH> DI void luma_rows(const EncWg& G, Ctx& C)
{
    const EncArgs& a = *G.a;
    WaveLds* const W = G.W;
    int* const progress = G.progress;
    const int mbw = a.mbw, mbh = a.mbh, f = G.f, lane = C.lane;
    const int wv = __builtin_amdgcn_readfirstlane(G.wv);  // (wave-uniform: see luma_pairs)
    const FrameLds F = frame_lds<PASS>(G, 0);
    // which wave works which row (zw_enc_rows.h)
    using RS = RowSchedule<PASS, ROWS, NW, NCH>;
    constexpr bool skip_mode = RS::skip_mode;
    constexpr int nrw = RS::nrw;
    const int rw = ROWS ? 0 : RS::first_row(wv, mbh);
    if (ROWS) {
        // the wave's window stands in for the frame-wide top arrays (offsets 0)
        C.top_y = W->win_y;
        C.top_u = W->win_u;
        C.top_v = W->win_v;
        C.top_c = W->win_c;
        C.top_derr = W->win_d;
    }
    // Pass 1 loads the MB's source words and alpha at the top of its iteration,
    // in flight during the wait for the row above; pass 2 fetches them one MB
    // ahead.  (Fetched ahead, pass 1's words do not stay in registers: each is
    // spilled to scratch right after its load, so the three loads run one after
    // another, each also waiting for the previous MB's stores -- vmcnt counts
    // stores.  Measured per 256 1080p frames: pass 1 29.12 -> 28.98 ms loading
    // at the top, pass 2 37.38 -> 37.64 ms.)
    constexpr bool fetch_ahead = PASS == 2;
    for (int it = 0, yk = rw;; it++) {
        const int mby = __builtin_amdgcn_readfirstlane(ROWS ? row_ticket(&G.rsync[0]) : (skip_mode ? yk : rw + it * nrw));
        if (skip_mode) yk = RS::next_row(wv, yk, mbh);
        if (mby >= mbh) break;
        row_start(C.M, lane);
        wsync();
        const int prevw = (!ROWS && mby > 0) ? RS::wave_of_row(mby - 1) : 0;
        int seen = -1;  // ROWS: last progress value read of the row above
        int* const prog_above = ROWS ? G.rsync + 4 + (mby > 0 ? mby - 1 : 0) : nullptr;
        // the row above has finished `need` MBs
        auto wait_above = [&](int need) {
            if (mby == 0) return;
            if (ROWS) row_wait(prog_above, need, G.rerr, seen);
            else wait_row(progress, prevw, (mby - 1) * 65536 + need);
        };
        MbFetch nx;
        if (fetch_ahead) nx = fetch_mb(&a, f, lane, 0, mby);
        for (int mbx = 0; mbx < mbw; mbx++) {
            PH_START();
            const int lane = opaque_lane(threadIdx.x & 63);
            C.lane = lane;
            MbFetch cur;
            if (fetch_ahead) {
                cur = nx;
                if (mbx + 1 < mbw) nx = fetch_mb(&a, f, lane, mbx + 1, mby);
            } else {
                cur = fetch_mb(&a, f, lane, mbx, mby);
            }
            // the I16 and chroma searches need only the MB above (x, y-1); the
            // I4 search also reads the above-right MB's bottom row: wait for
            // (x+1, y-1) only then, so the wait overlaps the first searches
            wait_above(min(mbx + 1, mbw));
            if (ROWS) {
                if (mby > 0) {
                    win_pull<PASS>(G, lane, mbx);
                } else if (PASS == 2) {
                    // row 0: zero contexts; top_derr from pass 1 (quirk A6)
                    if (lane < 3) ((uint32_t*)W->win_c)[lane] = 0;
                    else if (lane == 3)
                        ((uint32_t*)W->win_d)[0] = *(const uint32_t*)(a.derr + (size_t)f * mbw * 4 + mbx * 4);
                }
                wsync();
            } else {
                C.oy = mbx * 16;
                C.oc = mbx * 8;
                C.ocx = mbx * 12;
                C.od = mbx * 4;
            }
            if (!ROWS) luma_issue_prio<PASS>(progress, prevw, mbx, mby, mbw);
            PH_MARK(0);
            setup_ctx(C, &a, G.seg_lut, W, mbx, mby, cur);
            build_luma_border(C, 0);
            int lm;
            unsigned long long i16s;
            pick_i16<PASS>(C, lm, i16s);
            wsync();
            PH_MARK(1);
            int cm = 0;
            uint32_t i4nz = 0;
            bool i4reuse = false;
            if (PASS == 2) {
                build_chroma_border(C);
                cm = pick_uv<PASS>(C);
            }
            PH_MARK(3);
            if (C.method > 1) {
                const unsigned long long thr = 211ull * C.S->l_mode;
                if (C.method >= 5 || i16s > thr || lm != 0) {
                    wait_above(min(mbx + 2, mbw));
                    if (ROWS && mby > 0 && mbx + 1 < mbw) {
                        win_pull_right(G, lane, mbx);
                        wsync();
                    }
                    build_luma_border(C, 1);
                    PH_MARK(21);
                    if (pick_i4<PASS>(C, i16s, F.keep_i4, i4nz)) {
                        lm = 4;
                        i4reuse = F.keep_i4;
                    }
                }
            }
            PH_MARK(2);
            mb_store<PASS>(C, lm, cm, i4reuse, i4nz, F.trel);
            PH_RESET();
            if (ROWS) {
                // push this MB's state for the row below (sc1), then publish
                if (mby + 1 < mbh) {
                    win_push<PASS>(G, lane, mbx);
                    row_publish(G.rsync + 4 + mby, mbx + 1);
                }
            } else {
                publish(progress, wv, mby * 65536 + mbx + 1);
            }
            PH_MARK(6);
        }
    }
}

// ---------------------------------------------------------------------------
// An encode kernel: carve the LDS, fill the shared state, build the wave's Ctx,
// then the wave's role.
// ---------------------------------------------------------------------------
template <int PASS, bool ROWS, int FP = 1> DI void encode_body(const EncArgs& a)
{
    using SH = EncShape<PASS, ROWS, FP>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const EncWg G = enc_carve<PASS, ROWS, FP>(a, smem);
    // pass 1's chroma chain: workgroup 0 of each frame in the row-parallel
    // kernels (it keeps the frame-wide top_u/v/derr in LDS), the first waves of
    // the batch kernels
    const bool chain_wg = PASS == 1 && (ROWS ? blockIdx.x == 0 : G.wv < SH::NCW);
    enc_fill<PASS, ROWS, FP>(G, chain_wg);

    Ctx C;
    C.a = &a;
    C.W = G.W;
    C.lane = lane;
    ctx_enter(C, frame_lds<PASS>(G, 0), &G.W->mb, 0, 0);
    ph_init(G, lane);

    if (chain_wg) {
        __builtin_amdgcn_s_setprio(ZW_CHAIN_PRIO);  // (issue priority: see ZW_CHAIN_PRIO)
        if constexpr (SH::NCH == 2 && !SH::PAIR) chain_quad<PASS>(G, C);
        else chain_one<PASS, FP>(G, C);
    }
    // (in frame pairs the chain waves, their chains done, take luma rows)
    if (!chain_wg || SH::PAIR) {
        if (PASS == 1) __builtin_amdgcn_s_setprio(ZW_LUMA_PRIO);
        if constexpr (SH::PAIR) luma_pairs<PASS, SH::NW, SH::NCW>(G, C);
        else luma_rows<PASS, ROWS, SH::NW, SH::NCH>(G, C);
    }
    ph_flush<PASS>(G, lane);
}

extern "C" __global__ __launch_bounds__(PassShape<1>::WG) void k_encode_pass1(EncArgs a) { encode_body<1, false>(a); }
extern "C" __global__ __launch_bounds__(PassShape<1>::WG) void k_encode_pass1_fp(EncArgs a) { encode_body<1, false, 2>(a); }
extern "C" __global__ __launch_bounds__(PassShape<2>::WG) void k_encode_pass2(EncArgs a) { encode_body<2, false>(a); }
extern "C" __global__ __launch_bounds__(PassShape<2>::WG) void k_encode_pass2_fp(EncArgs a) { encode_body<2, false, 2>(a); }
extern "C" __global__ __launch_bounds__(64 * RowsShape<1>::NW) void k_encode_rows_pass1(EncArgs a) { encode_body<1, true>(a); }
extern "C" __global__ __launch_bounds__(64) void k_encode_rows_pass2(EncArgs a) { encode_body<2, true>(a); }

static size_t encode_lds_bytes(int mbw, int nw, bool rows, int pass, int fp = 1)
{
    return EncLds(mbw, rows, pass).bytes(nw, fp);
}

// Frame pairs (k_encode_pass1_fp / k_encode_pass2_fp) for launches of at
// least two frames per CU whose pair shape fits in LDS; ZW_ENC_FP=0/1 forces
// them off/on (where they fit), ZW_ENC_FP1 the same for pass 1 alone.
static bool encode_fp_for(int pass, int mbw, int nframes)
{
    static const int mode2 = [] { const char* e = getenv("ZW_ENC_FP"); return e && *e ? atoi(e) : -1; }();
    static const int mode1 = [] { const char* e = getenv("ZW_ENC_FP1"); return e && *e ? atoi(e) : mode2; }();
    const int mode = pass == 1 ? mode1 : mode2;
    static const int cus = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        return hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                       prop.multiProcessorCount > 0
                   ? prop.multiProcessorCount
                   : 256;
    }();
    if (mode == 0 || nframes < 2) return false;
    if (encode_lds_bytes(mbw, pass == 1 ? PassShape<1>::NW : PassShape<2>::NW, false, pass, 2) > 160 * 1024) return false;
    return mode == 1 || nframes >= 2 * cus;
}
extern "C" int zwk_encode_fp(int pass, int mbw, int nframes) { return encode_fp_for(pass, mbw, nframes) ? 1 : 0; }

// The widest frame (in MBs) whose LDS fits the 160 KiB of a CU in the batch
// shapes (rows = false: every row array of the frame in LDS) or in the
// row-parallel shapes (rows = true: only pass 1's chroma chain keeps rows).
// encode_frame_lossy takes any u16 width (vp8.rs:3143-3148): 4 096 MBs, which
// the row-parallel kernels hold; wider frames than the batch shapes take go to them.
extern "C" int zwk_encode_max_mbw(int rows)
{
    int lo = 1, hi = 65536 / 16;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        const bool ok = rows ? encode_lds_bytes(mid, RowsShape<1>::NW, true, 1) <= 160 * 1024 &&
                                   encode_lds_bytes(mid, RowsShape<2>::NW, true, 2) <= 160 * 1024
                             : encode_lds_bytes(mid, PassShape<1>::NW, false, 1) <= 160 * 1024 &&
                                   encode_lds_bytes(mid, PassShape<2>::NW, false, 2) <= 160 * 1024;
        if (ok) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Bytes of zero-filled scratch the row-parallel kernels need for nframes frames.
extern "C" size_t zwk_encode_rows_bytes(int mbw, int mbh, int nframes)
{
    return ZW_ROWS_HDR + (size_t)nframes * RowsLayout(mbw, mbh).frame;
}

// rows: null -> one 12-wave workgroup per frame (batches); otherwise the
// row-parallel kernels with that zero-filled scratch (zwk_encode_rows_bytes).
extern "C" hipError_t zwk_encode(hipStream_t s, int pass, const uint8_t* Y, const uint8_t* U, const uint8_t* V,
                                 const uint8_t* alpha, const ZwFrameParams* params, const ZwLevelCosts* lcost,
                                 int8_t* derr, ZwMbOut* out, uint8_t* ry, uint8_t* ru, uint8_t* rv, size_t ysz,
                                 size_t csz, int mbw, int mbh, int nframes, int* dbg, uint8_t* rows, uint32_t* sizes)
{
    EncArgs a;
    a.dbg = dbg;
    a.sizes = pass == 2 ? sizes : nullptr;
    a.Y = Y; a.U = U; a.V = V; a.alpha = alpha; a.params = params; a.lcost = lcost; a.derr = derr; a.out = out;
    a.ry = ry; a.ru = ru; a.rv = rv; a.ysz = ysz; a.csz = csz; a.mbw = mbw; a.mbh = mbh; a.pass = pass;
    a.rows = rows;
    a.nframes = nframes;
    static const bool attr_set = []() {
        (void)hipFuncSetAttribute((const void*)k_encode_pass1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_encode_pass2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_encode_pass2_fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_encode_pass1_fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_encode_rows_pass1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_encode_rows_pass2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return true;
    }();
    (void)attr_set;
    if (rows) {
        // one wave per MB row (+ pass 1's chroma chain in workgroup 0)
        if (pass == 1) {
            constexpr int nw = RowsShape<1>::NW;
            hipLaunchKernelGGL(k_encode_rows_pass1, dim3(1 + (mbh + nw - 1) / nw, nframes), dim3(64 * nw),
                               encode_lds_bytes(mbw, nw, true, 1), s, a);
        } else {
            hipLaunchKernelGGL(k_encode_rows_pass2, dim3(mbh, nframes), dim3(64), encode_lds_bytes(mbw, 1, true, 2), s,
                               a);
        }
        return hipGetLastError();
    }
    if (encode_fp_for(pass, mbw, nframes)) {
        if (pass == 1)
            hipLaunchKernelGGL(k_encode_pass1_fp, dim3((nframes + 1) / 2), dim3(PassShape<1>::WG),
                               encode_lds_bytes(mbw, PassShape<1>::NW, false, 1, 2), s, a);
        else
            hipLaunchKernelGGL(k_encode_pass2_fp, dim3((nframes + 1) / 2), dim3(PassShape<2>::WG),
                               encode_lds_bytes(mbw, PassShape<2>::NW, false, 2, 2), s, a);
        return hipGetLastError();
    }
    const size_t lds = encode_lds_bytes(mbw, pass == 1 ? PassShape<1>::NW : PassShape<2>::NW, false, pass);
    if (pass == 1) hipLaunchKernelGGL(k_encode_pass1, dim3(nframes), dim3(PassShape<1>::WG), lds, s, a);
    else hipLaunchKernelGGL(k_encode_pass2, dim3(nframes), dim3(PassShape<2>::WG), lds, s, a);
    return hipGetLastError();
}
