// emit_ref.h -- the direct emission walk, for the tools only: one boolean coder
// per partition fed decision by decision from one serial raster walk.  It was
// the product's emitter before the split emission (csrc/zw_host_emit.h) and is
// now what emit_equiv.cpp and emit_bench.cpp compare zwh::emit_frames against;
// bool_equiv.cpp compares its two coders with each other.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "zw_host_entropy.h"

namespace zwh {

// ArithmeticEncoder (arithmetic.rs:7-196).  The reference renormalises one bit
// per loop iteration; here all `shift` bits of one renormalisation are taken
// at once (the same arithmetic in libvpx's batched form: `count` = -bit_num,
// `low` = bottom), with the carry into already-written bytes propagated as the
// reference's add_one does.  Byte-identical output (tests/test_host_entropy.py
// drives both forms over random decision streams).
struct BoolEncoder {
    std::vector<uint8_t> buf;
    uint32_t low = 0, range = 255;
    int count = -24;  // = -bit_num

    BoolEncoder() { buf.reserve(1 << 16); }
    void add_one()
    {
        size_t i = buf.size();
        while (i > 0) {
            i--;
            if (buf[i] < 255) {
                buf[i]++;
                return;
            }
            buf[i] = 0;
        }
        buf.insert(buf.begin(), 1);
    }
    inline void put(int bit, int prob)
    {
        const uint32_t split = 1 + (((range - 1) * (uint32_t)prob) >> 8);
        // branch-free: the coded bits are by construction unpredictable
        const uint32_t m = 0u - (uint32_t)(bit != 0);
        low += split & m;
        const uint32_t r = split ^ ((split ^ (range - split)) & m);
        // renormalise: range back to [128, 255]
        const int shift = __builtin_clz(r) - 24;
        range = r << shift;
        count += shift;
        if (count >= 0) {  // a byte is complete after `offset` of the shifts
            const int offset = shift - count;
            if ((low << (offset - 1)) & 0x80000000u) add_one();
            buf.push_back((uint8_t)(low >> (24 - offset)));
            low = (low << offset) & 0xffffffu;
            low <<= count;
            count -= 8;
        } else {
            low <<= shift;
        }
    }
    void flag(int f) { put(f, 128); }
    void literal(int nbits, int v)
    {
        for (int b = nbits - 1; b >= 0; b--) put(((1 << b) & v) > 0, 128);
    }
    // a precomputed tree path: n bits, MSB-first bits / probability indices
    inline void path(const uint8_t* bits, const uint8_t* pidx, int n, const uint8_t* probs)
    {
        for (int i = 0; i < n; i++) put(bits[i], probs[pidx[i]]);
    }
    void flush()  // the reference's flush (arithmetic.rs:176-196) on its state (bottom, bit_num)
    {
        const int bit_num = -count;
        int c = bit_num;
        uint32_t v = low;
        if (low & (1u << (32 - bit_num))) add_one();
        v <<= (c & 7);
        c = (c >> 3) - 1;
        while (c >= 0) {
            v <<= 8;
            c--;
        }
        for (c = 3; c >= 0; c--) {
            buf.push_back((uint8_t)(v >> 24));
            v <<= 8;
        }
    }
};

// The reference's bit-at-a-time form, kept for the equivalence test only.
struct BoolEncoderRef {
    std::vector<uint8_t> buf;
    uint32_t bottom = 0, range = 255;
    int bit_num = 24;
    void add_one()
    {
        size_t i = buf.size();
        while (i > 0) {
            i--;
            if (buf[i] < 255) {
                buf[i]++;
                return;
            }
            buf[i] = 0;
        }
        buf.insert(buf.begin(), 1);
    }
    void put(int bit, int prob)
    {
        uint32_t split = 1 + (((range - 1) * (uint32_t)prob) >> 8);
        if (bit) {
            bottom += split;
            range -= split;
        } else {
            range = split;
        }
        while (range < 128) {
            range <<= 1;
            if (bottom & (1u << 31)) add_one();
            bottom <<= 1;
            if (--bit_num == 0) {
                buf.push_back((uint8_t)(bottom >> 24));
                bottom &= (1u << 24) - 1;
                bit_num = 8;
            }
        }
    }
    void flush()
    {
        int c = bit_num;
        uint32_t v = bottom;
        if (bottom & (1u << (32 - bit_num))) add_one();
        v <<= (c & 7);
        c = (c >> 3) - 1;
        while (c >= 0) { v <<= 8; c--; }
        for (c = 3; c >= 0; c--) { buf.push_back((uint8_t)(v >> 24)); v <<= 8; }
    }
};

// encode_coefficients token part (vp8.rs:845-958) for an already-quantized
// packed block (eob = last nonzero + 1).
template <class Enc>
inline int emit_block(Enc& E, const uint8_t (*P)[3][11], const uint8_t* lv, int eobi, int first, int ctx)
{
    const TokenPaths& TP = token_paths();
    int skip_eob = 0;
    for (int idx = first; idx < eobi; idx++) {
        const int coeff = lv_at(lv, idx);
        const uint8_t* pr = P[COEFF_BANDS[idx]][ctx];
        const int a = coeff < 0 ? -coeff : coeff;
        const int token = token_of(a);
        E.path(TP.bits[skip_eob][token], TP.pidx[skip_eob][token], TP.n[skip_eob][token], pr);
        if (token >= 5) {
            const int cat = token;
            const uint8_t* cp = PROB_DCT_CAT[cat - 5];
            int extra = a - DCT_CAT_BASE[cat - 5];
            int mask = cat == 10 ? 1 << 10 : 1 << (cat - 5);
            for (int k = 0; k < 12 && cp[k]; k++) {
                E.put((extra & mask) > 0, cp[k]);
                mask >>= 1;
            }
        }
        skip_eob = token == 0;
        if (token != 0) E.flag(!(coeff > 0));
        ctx = token == 0 ? 0 : (token == 1 ? 1 : 2);
    }
    if (eobi < 16) {
        int bi = first > eobi ? first : eobi;
        E.path(TP.bits[0][11], TP.pidx[0][11], TP.n[0][11], P[COEFF_BANDS[bi]][ctx]);
    }
    return eobi > 0;
}

// encode_residual_data (vp8.rs:650-800) of one MB with its left / top
// complexity (non-zero) contexts.
template <class Enc>
inline void emit_mb_tokens(Enc& E, const uint8_t (*probs)[8][3][11], const PackedMb& m, Cplx& left, Cplx& top)
{
    const bool i4 = m.luma == 4;
    if (m.skip) {
        left.clear(!i4);
        top.clear(!i4);
        return;
    }
    const int plane = i4 ? 3 : 0;
    if (!i4) left.y2 = top.y2 = (uint8_t)emit_block(E, probs[1], m.lv[16], m.eob[16], 0, left.y2 + top.y2);
    const int first = i4 ? 0 : 1;
    for (int by = 0; by < 4; by++) {
        int l = left.y[by];
        for (int bx = 0; bx < 4; bx++) {
            const int b = by * 4 + bx;
            l = emit_block(E, probs[plane], m.lv[b], m.eob[b], first, l + top.y[bx]);
            top.y[bx] = (uint8_t)l;
        }
        left.y[by] = (uint8_t)l;
    }
    for (int pl = 0; pl < 2; pl++) {
        uint8_t* lc = pl ? left.v : left.u;
        uint8_t* tc = pl ? top.v : top.u;
        for (int by = 0; by < 2; by++) {
            int l = lc[by];
            for (int bx = 0; bx < 2; bx++) {
                const int b = 17 + 4 * pl + by * 2 + bx;
                l = emit_block(E, probs[2], m.lv[b], m.eob[b], 0, l + tc[bx]);
                tc[bx] = (uint8_t)l;
            }
            lc[by] = (uint8_t)l;
        }
    }
}

// Frame tag (write_uncompressed_frame_header vp8.rs:315-330), the first
// partition, then for nparts > 1 the nparts - 1 3-byte partition sizes and the
// token partitions (RFC 6386 9.5; read back by decoder/vp8.rs:421-450).
inline void assemble_frame(std::vector<uint8_t>& out, const std::vector<uint8_t>& H, const BoolEncoder* T, int nparts,
                           int width, int height)
{
    size_t tot = 10 + H.size() + 3 * (size_t)(nparts - 1);
    for (int p = 0; p < nparts; p++) tot += T[p].buf.size();
    out.resize(tot);
    uint8_t* o = out.data();
    uint32_t tag = ((uint32_t)H.size() << 5) | (1u << 4);
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
    memcpy(o + 10, H.data(), H.size());
    size_t w = 10 + H.size();
    for (int p = 0; p + 1 < nparts; p++, w += 3) {
        const size_t n = T[p].buf.size();
        o[w] = (uint8_t)n;
        o[w + 1] = (uint8_t)(n >> 8);
        o[w + 2] = (uint8_t)(n >> 16);
    }
    for (int p = 0; p < nparts; p++) {
        memcpy(o + w, T[p].buf.data(), T[p].buf.size());
        w += T[p].buf.size();
    }
}

// One frame: compressed header (vp8.rs:332), MB headers (:498), residual
// tokens (:650), frame tag (:315), in one raster walk.  nparts (1, 2, 4, 8)
// token partitions: MB row y's tokens go to partition y % nparts
// (vp8.rs:1419-1421).
inline void emit_frame(std::vector<uint8_t>& out, const ZwFrameParams& P, const uint8_t* packed, int width,
                       int height, bool have_updated, const uint8_t upd[4][8][3][11], int nparts = 1)
{
    PackedMb m;
    const int mbw = P.mbw, mbh = P.mbh;
    BoolEncoder H, T[8];
    for (int p = 0; p < nparts; p++) T[p].buf.reserve((size_t)mbw * mbh * 16 / nparts + 4096);
    uint8_t probs[4][8][3][11];
    emit_frame_header(H, P, have_updated, upd, nparts, probs);
    std::vector<Cplx> top(mbw);
    memset(top.data(), 0, sizeof(Cplx) * mbw);
    std::vector<uint8_t> top_bp((size_t)mbw * 4, 0);
    for (int y = 0; y < mbh; y++) {
        Cplx left;
        memset(&left, 0, sizeof left);
        uint8_t left_bp[4] = {0, 0, 0, 0};
        for (int x = 0; x < mbw; x++) {
            packed = view_mb(packed, m);
            emit_mb_header(H, P, m, top_bp.data(), left_bp, x);
            emit_mb_tokens(T[y % nparts], probs, m, left, top[x]);
        }
    }
    H.flush();
    for (int p = 0; p < nparts; p++) T[p].flush();
    assemble_frame(out, H.buf, T, nparts, width, height);
}

}  // namespace zwh
