// zw_host_emit.h -- host half of the encoder, the emission: the sequential
// boolean coder stays on the CPU (north star).  Every byte of a VP8 frame
// leaves through emit_frames.  Restates, for the product path:
//   ArithmeticEncoder               encoder/arithmetic.rs:7-196
//   encode_coefficients / residuals encoder/vp8.rs:650-958
//   frame tag, partitions           encoder/vp8.rs:315-330, RFC 6386 9.5
//
// Split emission: the token walk records each MB's decisions (bit, probability)
// and a tight loop codes them.  The boolean coder's cost is its serial
// dependence through `range` (multiply, select, count-leading-zeros, shift per
// decision); with the token logic out of that loop, the coders of several
// streams -- a stream is one (frame, token partition) pair -- run side by side
// in one thread, so their independent chains overlap.  Byte-identical to the
// serial walk with one coder per partition (tools/emit_ref.h; tools/
// emit_equiv.cpp compares them): the same arithmetic in the same order per
// stream.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <immintrin.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "zw_host_entropy.h"

namespace zwh {

struct DecRec {  // a coder's interface; each decision appended as prob | bit << 8
    uint16_t* p;
    inline void put(int bit, int prob) { *p++ = (uint16_t)((uint32_t)prob | ((uint32_t)(bit != 0) << 8)); }
    void flag(int f) { put(f, 128); }
    void literal(int nbits, int v)
    {
        for (int b = nbits - 1; b >= 0; b--) put(((1 << b) & v) > 0, 128);
    }
    inline void path(const uint8_t* bits, const uint8_t* pidx, int n, const uint8_t* probs)
    {
        for (int i = 0; i < n; i++) put(bits[i], probs[pidx[i]]);
    }
};
// decisions of one MB's tokens: at most 25 blocks x 16 positions x (11 tree +
// 11 extra + 1 sign) + 25 end-of-block decisions
constexpr int kMbDecisionsMax = 25 * 16 * 23 + 25;

// One stream's coder state and bytes (ArithmeticEncoder, arithmetic.rs:7-196).
// The reference renormalises one bit per loop iteration; the coders below take
// all bits of one renormalisation at once (libvpx's batched form: `count` =
// -bit_num, `low` = bottom: 16..23 bits pending once a byte is out), with the
// carry into bytes already written propagated as the reference's add_one does
// (one spare byte in front for a carry out of the first byte).
struct RawBool {
    std::vector<uint8_t> buf;
    size_t lo = 1, pos = 1;  // first byte, next byte
    uint32_t low = 0, range = 255;
    int count = -24;
    void reset()  // an empty stream; the buffer stays
    {
        lo = pos = 1;
        low = 0;
        range = 255;
        count = -24;
    }
    void reserve_more(size_t n)
    {
        if (pos + n + 8 > buf.size()) buf.resize((pos + n + 8) * 2);
    }
    void carry(uint8_t* b)
    {
        size_t i = pos;
        while (i > lo) {
            i--;
            if (b[i] < 255) {
                b[i]++;
                return;
            }
            b[i] = 0;
        }
        b[--lo] = 1;
    }
    void flush()
    {
        reserve_more(8);
        uint8_t* b = buf.data();
        const int bit_num = -count;
        int c = bit_num;
        uint32_t v = low;
        if (low & (1u << (32 - bit_num))) carry(b);
        v <<= (c & 7);
        c = (c >> 3) - 1;
        while (c >= 0) {
            v <<= 8;
            c--;
        }
        for (c = 3; c >= 0; c--) {
            b[pos++] = (uint8_t)(v >> 24);
            v <<= 8;
        }
    }
    const uint8_t* data() const { return buf.data() + lo; }
    size_t size() const { return pos - lo; }
};

// M streams, n decisions each, interleaved (M independent dependency chains).
// RawBool's arithmetic with the low end of the interval in 64 bits: L holds
// 8 + c bits (c pending above the 8-bit range) and 48 pending bits go out at a
// time, so the byte-out branch -- unpredictable across four interleaved
// streams -- is taken once per ~64 decisions instead of ~11.  A carry out of L
// goes into the bytes already out at once.  The state enters and leaves in
// RawBool's form (low, count), so the bytes are those of a coder that writes
// every byte when it is due.  (Measured on the box, four distinct frames'
// streams: 0.93 ms per stream with 32 bits at a time, 1.07 with one byte.)
template <int M>
inline void raw_codeM(RawBool* const* S, const uint16_t* const* d, int n)
{
    uint8_t* b[M];
    uint64_t lo[M];
    uint32_t ra[M];
    int co[M];
    size_t po[M];
#pragma GCC unroll 4
    for (int k = 0; k < M; k++) {
        S[k]->reserve_more((size_t)n);
        b[k] = S[k]->buf.data();
        lo[k] = S[k]->low, ra[k] = S[k]->range, co[k] = S[k]->count + 24, po[k] = S[k]->pos;
        if (lo[k] >> (8 + co[k])) {  // (a carry the 32-bit form had not yet taken out)
            S[k]->carry(b[k]);
            lo[k] &= (1ull << (8 + co[k])) - 1;
        }
    }
    for (int i = 0; i < n; i++) {
#pragma GCC unroll 4
        for (int k = 0; k < M; k++) {
            const uint32_t D = d[k][i], prob = D & 255u, m = 0u - (D >> 8);
            const uint32_t split = 1 + (((ra[k] - 1) * prob) >> 8);
            lo[k] += split & m;
            if (__builtin_expect((lo[k] >> (8 + co[k])) != 0, 0)) {
                S[k]->pos = po[k];
                S[k]->carry(b[k]);
                lo[k] &= (1ull << (8 + co[k])) - 1;
            }
            const uint32_t r = split ^ ((split ^ (ra[k] - split)) & m);
            const int sh = __builtin_clz(r) - 24;
            ra[k] = r << sh;
            lo[k] <<= sh;
            co[k] += sh;
            if (co[k] >= 48) {  // the top 48 of the 8 + c bits, as 8 bytes (the last 2 rewritten later)
                const uint64_t be = __builtin_bswap64(lo[k] << (56 - co[k]));
                memcpy(b[k] + po[k], &be, 8);
                po[k] += 6;
                co[k] -= 48;
                lo[k] &= (1ull << (8 + co[k])) - 1;
            }
        }
    }
#pragma GCC unroll 4
    for (int k = 0; k < M; k++) {
        while (co[k] >= 24) {
            b[k][po[k]++] = (uint8_t)(lo[k] >> co[k]);
            lo[k] &= (1ull << co[k]) - 1;
            co[k] -= 8;
        }
        while (co[k] < 16 && po[k] > S[k]->lo) {  // bytes back in (at most 5)
            lo[k] |= (uint64_t)b[k][--po[k]] << (8 + co[k]);
            co[k] += 8;
        }
        S[k]->low = (uint32_t)lo[k], S[k]->range = ra[k], S[k]->count = co[k] - 24, S[k]->pos = po[k];
    }
}

// Up to 16 streams at once, one per lane of AVX-512 vectors: raw_codeM's
// arithmetic (low end in 64 bits, 48 pending bits out at a time) on 16 lanes,
// each lane's decision fetched by a gather from the shared arena `base` at
// element offset off[k] + i; lanes past their stream's length n[k] are masked.
// The rare events -- a carry, 48 bits due -- are handled per lane in scalar
// code.  Same bytes as raw_codeM (one independent coder per lane).
__attribute__((target("avx512f,avx512cd,avx512vl,avx512dq,avx512bw"))) inline void raw_code16(
    RawBool* const* S, const uint16_t* base, const uint32_t* off, const int* n, int K)
{
    alignas(64) uint64_t lo[16];
    alignas(64) uint32_t ra[16], ix[16], nn[16];
    alignas(64) int32_t co[16];
    uint8_t* b[16];
    size_t po[16];
    int nmax = 0;
    for (int k = 0; k < 16; k++) {
        if (k < K) {
            S[k]->reserve_more((size_t)n[k]);
            b[k] = S[k]->buf.data();
            lo[k] = S[k]->low, ra[k] = S[k]->range, co[k] = S[k]->count + 24, po[k] = S[k]->pos;
            if (lo[k] >> (8 + co[k])) {
                S[k]->carry(b[k]);
                lo[k] &= (1ull << (8 + co[k])) - 1;
            }
            ix[k] = off[k];
            nn[k] = (uint32_t)n[k];
            nmax = n[k] > nmax ? n[k] : nmax;
        } else {
            b[k] = nullptr;
            lo[k] = 0, ra[k] = 255, co[k] = 0, po[k] = 0, ix[k] = 0, nn[k] = 0;
        }
    }
    __m512i vlo0 = _mm512_load_si512(lo), vlo1 = _mm512_load_si512(lo + 8);
    __m512i vra = _mm512_load_si512(ra), vco = _mm512_load_si512(co), vix = _mm512_load_si512(ix);
    const __m512i vnn = _mm512_load_si512(nn), one = _mm512_set1_epi32(1), c255 = _mm512_set1_epi32(255);
    const __m512i c256 = _mm512_set1_epi32(0x100), c24 = _mm512_set1_epi32(24), c8 = _mm512_set1_epi32(8);
    const __m512i c48 = _mm512_set1_epi32(48);
    __m512i vi = _mm512_setzero_si512();
    for (int i = 0; i < nmax; i++) {
        const __mmask16 act = _mm512_cmpgt_epu32_mask(vnn, vi);
        vi = _mm512_add_epi32(vi, one);
        const __m512i d = _mm512_mask_i32gather_epi32(_mm512_setzero_si512(), act, vix, (const void*)base, 2);
        vix = _mm512_add_epi32(vix, one);
        const __m512i prob = _mm512_and_si512(d, c255);
        const __mmask16 bit = _mm512_mask_test_epi32_mask(act, d, c256);
        const __m512i split = _mm512_add_epi32(one, _mm512_srli_epi32(_mm512_mullo_epi32(_mm512_sub_epi32(vra, one), prob), 8));
        const __m512i r = _mm512_mask_sub_epi32(split, bit, vra, split);
        const __m512i sh = _mm512_maskz_sub_epi32(act, _mm512_lzcnt_epi32(r), c24);
        vra = _mm512_mask_sllv_epi32(vra, act, r, sh);
        // low += split (bit lanes), in two halves of 8 x 64 bits
        const __m512i add = _mm512_maskz_mov_epi32(bit, split);
        vlo0 = _mm512_add_epi64(vlo0, _mm512_cvtepu32_epi64(_mm512_castsi512_si256(add)));
        vlo1 = _mm512_add_epi64(vlo1, _mm512_cvtepu32_epi64(_mm512_extracti64x4_epi64(add, 1)));
        const __m512i w = _mm512_add_epi32(vco, c8);  // the bits L may hold
        const __m512i w0 = _mm512_cvtepu32_epi64(_mm512_castsi512_si256(w)), w1 = _mm512_cvtepu32_epi64(_mm512_extracti64x4_epi64(w, 1));
        const __mmask8 cy0 = _mm512_test_epi64_mask(_mm512_srlv_epi64(vlo0, w0), _mm512_srlv_epi64(vlo0, w0));
        const __mmask8 cy1 = _mm512_test_epi64_mask(_mm512_srlv_epi64(vlo1, w1), _mm512_srlv_epi64(vlo1, w1));
        if (__builtin_expect((cy0 | cy1) != 0, 0)) {
            _mm512_store_si512(lo, vlo0);
            _mm512_store_si512(lo + 8, vlo1);
            const unsigned cm = (unsigned)cy0 | ((unsigned)cy1 << 8);
            for (int k = 0; k < 16; k++)
                if ((cm >> k) & 1u) {
                    S[k]->pos = po[k];
                    S[k]->carry(b[k]);
                    lo[k] &= (1ull << (8 + co[k])) - 1;
                }
            vlo0 = _mm512_load_si512(lo);
            vlo1 = _mm512_load_si512(lo + 8);
        }
        vlo0 = _mm512_sllv_epi64(vlo0, _mm512_cvtepu32_epi64(_mm512_castsi512_si256(sh)));
        vlo1 = _mm512_sllv_epi64(vlo1, _mm512_cvtepu32_epi64(_mm512_extracti64x4_epi64(sh, 1)));
        vco = _mm512_add_epi32(vco, sh);
        _mm512_store_si512(co, vco);  // (co[] stays current for the scalar paths)
        const __mmask16 fm = _mm512_cmpge_epi32_mask(vco, c48);
        if (fm) {
            _mm512_store_si512(lo, vlo0);
            _mm512_store_si512(lo + 8, vlo1);
            for (unsigned m = fm; m; m &= m - 1) {
                const int k = __builtin_ctz(m);
                const uint64_t be = __builtin_bswap64(lo[k] << (56 - co[k]));
                memcpy(b[k] + po[k], &be, 8);
                po[k] += 6;
                co[k] -= 48;
                lo[k] &= (1ull << (8 + co[k])) - 1;
            }
            vlo0 = _mm512_load_si512(lo);
            vlo1 = _mm512_load_si512(lo + 8);
            vco = _mm512_load_si512(co);
        }
    }
    _mm512_store_si512(lo, vlo0);
    _mm512_store_si512(lo + 8, vlo1);
    _mm512_store_si512(ra, vra);
    _mm512_store_si512(co, vco);
    for (int k = 0; k < K; k++) {
        while (co[k] >= 24) {
            b[k][po[k]++] = (uint8_t)(lo[k] >> co[k]);
            lo[k] &= (1ull << co[k]) - 1;
            co[k] -= 8;
        }
        while (co[k] < 16 && po[k] > S[k]->lo) {
            lo[k] |= (uint64_t)b[k][--po[k]] << (8 + co[k]);
            co[k] += 8;
        }
        S[k]->low = (uint32_t)lo[k], S[k]->range = ra[k], S[k]->count = co[k] - 24, S[k]->pos = po[k];
    }
}
inline bool have_code16()
{
    static const bool ok = [] {
        if (const char* e = getenv("ZW_CODE16"))
            if (atoi(e) == 0) return false;
        return __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512cd") &&
               __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("avx512dq") &&
               __builtin_cpu_supports("avx512bw");
    }();
    return ok;
}

// K (<= 4) streams of different lengths: interleaved over the common length,
// then over the longer ones' remainders.
inline void raw_code_multi(RawBool* const* S, const uint16_t* const* d, const int* n, int K)
{
    const uint16_t* dd[4];
    int nn[4];
    for (int k = 0; k < K; k++) dd[k] = d[k], nn[k] = n[k];
    for (;;) {
        RawBool* as[4];
        const uint16_t* ad[4];
        int ai[4], m = 0, mn = 1 << 30;
        for (int k = 0; k < K; k++)
            if (nn[k] > 0) {
                as[m] = S[k];
                ad[m] = dd[k];
                ai[m++] = k;
                mn = nn[k] < mn ? nn[k] : mn;
            }
        if (m == 0) return;
        switch (m) {
        case 4: raw_codeM<4>(as, ad, mn); break;
        case 3: raw_codeM<3>(as, ad, mn); break;
        case 2: raw_codeM<2>(as, ad, mn); break;
        default: raw_codeM<1>(as, ad, mn); break;
        }
        for (int j = 0; j < m; j++) dd[ai[j]] += mn, nn[ai[j]] -= mn;
    }
}

// The token tree paths as decision templates: per (after-a-zero, token) the
// decisions bit << 8 | probability index, padded to 12 with index 0.
struct TokTmpl {
    uint8_t n[2][12];
    uint16_t d[2][12][12];
    TokTmpl()
    {
        const TokenPaths& TP = token_paths();
        for (int s = 0; s < 2; s++)
            for (int v = 0; v < 12; v++) {
                n[s][v] = TP.n[s][v];
                for (int i = 0; i < 12; i++)
                    d[s][v][i] = i < TP.n[s][v] ? (uint16_t)((TP.bits[s][v][i] << 8) | TP.pidx[s][v][i]) : 0;
            }
    }
};
inline const TokTmpl& tok_tmpl()
{
    static const TokTmpl T;
    return T;
}

// The token paths with the frame's probabilities filled in: per (type, band,
// ctx, after-a-zero, token) the path's decisions (bit << 8 | probability),
// its length in entry 15.  Built once per frame (the probabilities are fixed
// for the frame's tokens), so a token's decisions are one 32-byte copy.
struct TokRes {
    alignas(32) uint16_t d[4][8][3][2][12][16];
};
inline void tok_resolve(TokRes& R, const uint8_t (*probs)[8][3][11])
{
    const TokTmpl& TT = tok_tmpl();
    for (int t = 0; t < 4; t++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 3; c++)
                for (int s = 0; s < 2; s++)
                    for (int v = 0; v < 12; v++) {
                        uint16_t* o = R.d[t][b][c][s][v];
                        const int n = TT.n[s][v];
                        for (int i = 0; i < 16; i++)
                            o[i] = i < n ? (uint16_t)((TT.d[s][v][i] & 0xff00u) | probs[t][b][c][TT.d[s][v][i] & 0xffu]) : 0;
                        o[15] = (uint16_t)n;
                    }
}

// The token decisions of one already-quantized packed block (eob = last
// nonzero + 1; encode_coefficients' token part, vp8.rs:845-958) recorded at o
// (which has 16 entries of slack: a path is copied whole).  Rt: the block
// type's resolved paths, P its probabilities.  Returns the block's context
// bit, eob > 0.
inline int rec_block(uint16_t*& o, const uint16_t (*Rt)[3][2][12][16], const uint8_t (*P)[3][11], const uint8_t* lv,
                     int eobi, int first, int ctx)
{
    if (eobi <= first) {  // no coefficient: the end of block at `first` (bit 0)
        *o++ = P[COEFF_BANDS[first]][ctx][0];
        return eobi > 0;
    }
    int s = 0;
    uint16_t* q = o;
    for (int idx = first; idx < eobi; idx++) {
        const int coeff = lv_at(lv, idx);
        const int a = coeff < 0 ? -coeff : coeff;
        const int token = token_of(a);
        const uint16_t* t = Rt[COEFF_BANDS[idx]][ctx][s][token];
        memcpy(q, t, 32);
        q += t[15];
        if (token >= 5) {
            const uint8_t* cp = PROB_DCT_CAT[token - 5];
            const int extra = a - DCT_CAT_BASE[token - 5];
            int mask = token == 10 ? 1 << 10 : 1 << (token - 5);
            for (int k = 0; k < 12 && cp[k]; k++) {
                *q++ = (uint16_t)(cp[k] | ((extra & mask) ? 0x100 : 0));
                mask >>= 1;
            }
        }
        // the sign (token != 0), written always and kept only for a nonzero
        *q = (uint16_t)(128u | (((uint32_t)coeff >> 31) << 8));
        q += token != 0;
        s = token == 0;
        ctx = token >= 2 ? 2 : token;
    }
    if (eobi < 16) *q++ = P[COEFF_BANDS[eobi]][ctx][0];
    o = q;
    return 1;
}

// Blocks b0 .. b0 + nb - 1 (nb <= 16) of one block type in order, contexts cx,
// ne the mask of the non-empty ones (eob > first): the empty blocks' decisions
// (an end of block each) go out as whole runs -- one copy per run, from every
// block's end-of-block decision made up front -- so only the non-empty blocks
// take a branch (most blocks are empty: 85 % of a Q75 1080p frame's).
inline void rec_block_runs(uint16_t*& o, const uint16_t (*Rt)[3][2][12][16], const uint8_t (*P)[3][11],
                           const PackedMb& m, int b0, int nb, const int* cx, int first, uint32_t ne)
{
    uint16_t eobd[32] = {};  // (zeroed: a run's copy below takes 16 entries from any i < nb)
    const uint8_t* pb = P[COEFF_BANDS[first]][0];
    for (int i = 0; i < nb; i++) eobd[i] = pb[11 * cx[i]];
    uint16_t* q = o;
    int i = 0;
    for (;;) {
        const int j = ne ? __builtin_ctz(ne) : nb;
        memcpy(q, eobd + i, 32);  // (the run i .. j - 1; the rest is rewritten)
        q += j - i;
        if (j >= nb) break;
        rec_block(q, Rt, P, m.lv[b0 + j], m.eob[b0 + j], first, cx[j]);
        ne &= ne - 1;
        i = j + 1;
    }
    o = q;
}

// The token decisions of one MB (encode_residual_data, vp8.rs:650-800) with
// its left / top complexity (non-zero) contexts.  A block's context bit is
// eob > 0, so every block's context is taken from the eobs up front: the
// blocks' walks do not wait on each other.
inline void rec_mb_tokens(uint16_t*& o, const TokRes& R, const uint8_t (*probs)[8][3][11], const PackedMb& m, Cplx& left,
                          Cplx& top)
{
    const bool i4 = m.luma == 4;
    if (m.skip) {
        left.clear(!i4);
        top.clear(!i4);
        return;
    }
    const int plane = i4 ? 3 : 0;
    const uint8_t* e = m.eob;
    if (!i4) {
        const int c = left.y2 + top.y2;
        left.y2 = top.y2 = (uint8_t)(e[16] > 0);
        rec_block(o, R.d[1], probs[1], m.lv[16], e[16], 0, c);
    }
    const int first = i4 ? 0 : 1;
    int ctx[16];
    for (int by = 0; by < 4; by++)
        for (int bx = 0; bx < 4; bx++) {
            const int b = by * 4 + bx;
            const int l = bx ? (int)(e[b - 1] > 0) : left.y[by];
            const int t = by ? (int)(e[b - 4] > 0) : top.y[bx];
            ctx[b] = l + t;
        }
    for (int k = 0; k < 4; k++) {
        left.y[k] = (uint8_t)(e[4 * k + 3] > 0);
        top.y[k] = (uint8_t)(e[12 + k] > 0);
    }
    uint32_t ne = 0;
    for (int b = 0; b < 16; b++) ne |= (uint32_t)(e[b] > first) << b;
    rec_block_runs(o, R.d[plane], probs[plane], m, 0, 16, ctx, first, ne);
    int cc[8];
    uint32_t nc = 0;
    for (int pl = 0; pl < 2; pl++) {
        uint8_t* lc = pl ? left.v : left.u;
        uint8_t* tc = pl ? top.v : top.u;
        const int b0 = 17 + 4 * pl;
        cc[4 * pl] = lc[0] + tc[0];
        cc[4 * pl + 1] = (e[b0] > 0) + tc[1];
        cc[4 * pl + 2] = lc[1] + (e[b0] > 0);
        cc[4 * pl + 3] = (e[b0 + 2] > 0) + (e[b0 + 1] > 0);
        lc[0] = (uint8_t)(e[b0 + 1] > 0);
        lc[1] = (uint8_t)(e[b0 + 3] > 0);
        tc[0] = (uint8_t)(e[b0 + 2] > 0);
        tc[1] = (uint8_t)(e[b0 + 3] > 0);
        for (int k = 0; k < 4; k++) nc |= (uint32_t)(e[b0 + k] > 0) << (4 * pl + k);
    }
    rec_block_runs(o, R.d[2], probs[2], m, 17, 8, cc, 0, nc);
}

// K coders over their decision runs d[k] (n[k] decisions each): the 16-lane
// coder when the host has AVX-512, there are more than four and the runs lie
// within 2^31 elements of `base` (its gather offsets), else four at a time.
inline void code_streams(RawBool* const* S, const uint16_t* base, const uint16_t* const* d, const int* n, int K)
{
    if (K > 4 && have_code16()) {
        uint32_t off[16];
        bool fit = true;
        for (int k = 0; k < K; k++) {
            const size_t o = (size_t)(d[k] - base);
            fit = fit && o + (size_t)n[k] < ((size_t)1 << 31);
            off[k] = (uint32_t)o;
        }
        if (fit) {
            raw_code16(S, base, off, n, K);
            return;
        }
    }
    for (int k0 = 0; k0 < K; k0 += 4) raw_code_multi(S + k0, d + k0, n + k0, std::min(4, K - k0));
}

// Frame tag (write_uncompressed_frame_header vp8.rs:315-330), the first
// partition, then for nparts > 1 the nparts - 1 3-byte partition sizes, and the
// token partitions (RFC 6386 9.5; read back by decoder/vp8.rs:421-450).
inline void assemble_frame(std::vector<uint8_t>& out, const RawBool& H, const RawBool* T, int nparts, int width,
                           int height)
{
    const size_t hs = H.size();
    size_t tot = 10 + hs + 3 * (size_t)(nparts - 1);
    for (int p = 0; p < nparts; p++) tot += T[p].size();
    out.resize(tot);
    uint8_t* o = out.data();
    const uint32_t tag = ((uint32_t)hs << 5) | (1u << 4);
    o[0] = (uint8_t)tag;
    o[1] = (uint8_t)(tag >> 8);
    o[2] = (uint8_t)(tag >> 16);
    o[3] = 0x9d;
    o[4] = 0x01;
    o[5] = 0x2a;
    o[6] = (uint8_t)(width & 0xff);
    o[7] = (uint8_t)((width >> 8) & 0x3f);
    o[8] = (uint8_t)(height & 0xff);
    o[9] = (uint8_t)((height >> 8) & 0x3f);
    memcpy(o + 10, H.data(), hs);
    size_t w = 10 + hs;
    for (int p = 0; p + 1 < nparts; p++, w += 3) {
        const size_t n = T[p].size();
        o[w] = (uint8_t)n;
        o[w + 1] = (uint8_t)(n >> 8);
        o[w + 2] = (uint8_t)(n >> 16);
    }
    for (int p = 0; p < nparts; p++) {
        memcpy(o + w, T[p].data(), T[p].size());
        w += T[p].size();
    }
}

// Worst-case decisions of the first partition of a frame: the frame header's
// (at most 4 x 8 x 3 x 11 x 9 probability updates and ~100 others), then the MB
// headers' (at most 2 + 1 + 4 + 16 x 9 + 3 per MB); and of one MB row's tokens
// (+ rec_block's slack, + the gather's).
inline size_t emit_header_decisions(int mbw, int mbh) { return 4 * 8 * 3 * 11 * 9 + 256 + (size_t)mbw * mbh * 160; }
inline size_t emit_row_decisions(int mbw) { return (size_t)mbw * kMbDecisionsMax + 32; }

// Bytes of emit_frames' decision arenas per frame of a group with nparts token
// partitions (worst case, mostly never touched): callers size their groups
// with it.
inline size_t emit_arena_bytes(int mbw, int mbh, int nparts)
{
    return 2 * (emit_header_decisions(mbw, mbh) + (size_t)nparts * emit_row_decisions(mbw));
}

// The buffers of emit_frames (decision records, coders, row state) for up to
// kMax streams.  Kept between calls (a caller's pool, or one per thread): the
// record buffers are sized for the worst case, and allocating and faulting
// them in afresh cost more than the emission of a frame.
struct EmitWs {
    static constexpr int kMax = 16;
    struct Fr {
        RawBool H, T[8];  // first partition; token partitions
        std::vector<Cplx> top;
        std::vector<uint8_t> top_bp;
        uint8_t probs[4][8][3][11];
        TokRes res;
    } F[kMax];
    // Decision records: n slices of cap entries in one block (the 16-lane coder
    // gathers from it by 32-bit offsets), sized for the worst case and left
    // uninitialised, so only the pages a frame writes are ever touched.
    struct Arena {
        std::unique_ptr<uint16_t[]> d;
        size_t cap = 0;
        int n = 0;
        // at least n_ slices of cap_ entries.  The old block goes first (two
        // worst-case blocks need not exist at once) and the arena is empty
        // meanwhile, so a failed allocation leaves it consistent.
        uint16_t* fit(size_t cap_, int n_)
        {
            if (cap < cap_ || n < n_) {
                d.reset();
                cap = 0, n = 0;
                d.reset(new uint16_t[cap_ * (size_t)n_ + 32]);
                cap = cap_, n = n_;
            }
            return d.get();
        }
    };
    Arena hd, td;  // a slice per frame: its first partition; a slice per stream: one MB row's tokens
    std::vector<uint8_t> out[kMax], alph;  // (for the caller: container assembly)
};

// K frames of one size, nparts (1, 2, 4, 8) token partitions each, K x nparts
// <= EmitWs::kMax streams, emitted at once.  MB row y's tokens go to partition
// y % nparts (vp8.rs:1419-1421), so the rows are taken in bands of nparts: per
// frame in turn the band's rows are recorded in raster order -- the MB headers
// into the frame's first-partition slice, each row's tokens into a slice of its
// own; left / top contexts carry on serially -- then all the band's rows are
// coded side by side, row y by its frame's coder T[y % nparts].  Last the
// first partitions are coded, and each frame assembled.
inline void emit_frames(std::vector<uint8_t>* const* out, const ZwFrameParams* const* P, const uint8_t* const* packed,
                        int K, int nparts, int width, int height, const bool* have_updated,
                        const uint8_t (*const* upd)[8][3][11], EmitWs* ws = nullptr)
{
    using Fr = EmitWs::Fr;
    thread_local std::unique_ptr<EmitWs> own;
    if (!ws) {
        if (!own) own.reset(new EmitWs);
        ws = own.get();
    }
    Fr* F = ws->F;
    const int mbw = P[0]->mbw, mbh = P[0]->mbh;
    uint16_t* const hd = ws->hd.fit(emit_header_decisions(mbw, mbh), K);
    uint16_t* const td = ws->td.fit(emit_row_decisions(mbw), K * nparts);
    const size_t hst = ws->hd.cap, tst = ws->td.cap;
    const uint8_t* q[EmitWs::kMax];
    size_t hn[EmitWs::kMax];
    for (int k = 0; k < K; k++) {
        Fr& f = F[k];
        f.H.reset();
        for (int p = 0; p < nparts; p++) {
            f.T[p].reset();
            f.T[p].reserve_more((size_t)mbw * mbh * 16 / nparts + 4096);
        }
        f.top.assign(mbw, Cplx{});
        f.top_bp.assign((size_t)mbw * 4, 0);
        DecRec R{hd + (size_t)k * hst};
        emit_frame_header(R, *P[k], have_updated[k], upd[k], nparts, f.probs);
        tok_resolve(f.res, f.probs);
        q[k] = packed[k];
        hn[k] = (size_t)(R.p - (hd + (size_t)k * hst));
    }
    RawBool* ts[EmitWs::kMax];
    const uint16_t* tp[EmitWs::kMax];
    int tn[EmitWs::kMax];
    for (int y0 = 0; y0 < mbh; y0 += nparts) {
        const int rows = std::min(nparts, mbh - y0);
        int s = 0;  // the band's streams: frame k's row y0 + r is stream k * rows + r
        for (int k = 0; k < K; k++) {
            Fr& f = F[k];
            DecRec R{hd + (size_t)k * hst + hn[k]};
            for (int r = 0; r < rows; r++, s++) {
                Cplx left;
                memset(&left, 0, sizeof left);
                uint8_t left_bp[4] = {0, 0, 0, 0};
                uint16_t* const o0 = td + (size_t)s * tst;
                uint16_t* o = o0;
                for (int x = 0; x < mbw; x++) {
                    PackedMb m;
                    q[k] = view_mb(q[k], m);
                    emit_mb_header(R, *P[k], m, f.top_bp.data(), left_bp, x);
                    rec_mb_tokens(o, f.res, f.probs, m, left, f.top[x]);
                }
                tp[s] = o0;
                tn[s] = (int)(o - o0);
                ts[s] = &f.T[r];  // (y0 is a multiple of nparts)
            }
            hn[k] = (size_t)(R.p - (hd + (size_t)k * hst));
        }
        code_streams(ts, td, tp, tn, s);
    }
    // the first partitions
    RawBool* hs[EmitWs::kMax];
    const uint16_t* hp[EmitWs::kMax];
    int hl[EmitWs::kMax];
    for (int k = 0; k < K; k++) {
        hp[k] = hd + (size_t)k * hst;
        hl[k] = (int)hn[k];
        hs[k] = &F[k].H;
    }
    code_streams(hs, hd, hp, hl, K);
    for (int k = 0; k < K; k++) {
        F[k].H.flush();
        for (int p = 0; p < nparts; p++) F[k].T[p].flush();
        assemble_frame(*out[k], F[k].H, F[k].T, nparts, width, height);
    }
}

}  // namespace zwh

