// zw_dec_parse.h -- the decoder's CPU-only half: the boolean decoder, the frame
// header / mode / token parser (-> packed MB records), the CPU replay of the
// device token parse and the RIFF container parser (zw_dec_parse.cpp).  No
// device code: the translation unit builds with a plain C++17 compiler, so the
// parser of untrusted bytes can run stand-alone under sanitizers
// (tools/dec_parse_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zw_common.h"

#pragma GCC visibility push(hidden)  // internal to the library: not part of its ABI
namespace zwdec {

struct DecQuant {
    int32_t ydc, yac, y2dc, y2ac, uvdc, uvac;
};

// bit_reader.rs:254-640
struct BitReader {
    const uint8_t* d = nullptr;
    size_t len = 0, pos = 0;
    uint64_t value = 0;
    uint32_t range = 254;  // range - 1
    int bits = -8;
    bool eof = false;

    void init(const uint8_t* data, size_t n)
    {
        d = data;
        len = n;
        pos = 0;
        value = 0;
        range = 254;
        bits = -8;
        eof = false;
        load();
    }
    void load()
    {
        const size_t rem = len - pos;
        if (rem >= 7) {
            uint64_t v = 0;
            if (rem >= 8) {
                for (int i = 0; i < 8; i++) v = (v << 8) | d[pos + i];
                v >>= 8;
            } else {
                for (int i = 0; i < 7; i++) v = (v << 8) | d[pos + i];
            }
            value = v | (value << 56);
            bits += 56;
            pos += 7;
        } else if (pos < len) {
            bits += 8;
            value = (uint64_t)d[pos] | (value << 8);
            pos++;
        } else if (!eof) {
            value <<= 8;
            bits += 8;
            eof = true;
        } else {
            bits = 0;
        }
    }
    // branch-free: the decoded bit selects the new range and the value
    // update by masks (a data-dependent branch here mispredicts on every
    // other token bit; 25 % faster measured on 1080p streams)
    inline int bit(int prob)
    {
        if (bits < 0) load();
        const uint32_t r = range;
        const int p = bits;
        const uint32_t split = (r * (uint32_t)prob) >> 8;
        const uint32_t v = (uint32_t)(value >> p);
        const uint32_t b = v > split;
        const uint32_t m = 0u - b;  // all ones when the bit is 1
        const uint32_t nr = ((r - split) & m) | ((split + 1) & ~m);
        value -= (uint64_t)((split + 1) & m) << p;
        const int shift = 7 ^ (31 ^ __builtin_clz(nr));
        bits -= shift;
        range = (nr << shift) - 1;
        return (int)b;
    }
    int lit(int n)
    {
        int v = 0;
        for (int i = 0; i < n; i++) v = (v << 1) | bit(128);
        return v;
    }
    int sgn(int n)
    {
        if (!bit(128)) return 0;
        const int m = lit(n);
        return bit(128) ? -m : m;
    }
    int tree(const int8_t* t, const uint8_t* probs)
    {
        int i = 0;
        for (;;) {
            const int n = t[i + bit(probs[i >> 1])];
            if (n <= 0) return -n;
            i = n;
        }
    }
};

struct DecFrame {
    int width = 0, height = 0, mbw = 0, mbh = 0;
    int filter_type = 0, filter_level = 0, sharpness = 0;
    int segments_enabled = 0, seg_update_map = 0, seg_delta_values = 0;
    int lf_adj_enabled = 0, ref_delta0 = 0, mode_delta0 = 0;
    int8_t seg_quant[4] = {0, 0, 0, 0}, seg_lf[4] = {0, 0, 0, 0};
    uint8_t seg_probs[3] = {255, 255, 255};
    int nparts = 1;
    int skip_prob = -1;
    DecQuant q[4];
    uint8_t probs[4][8][3][11];
    BitReader hdr;
    BitReader part[8];
};

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// read_frame_header decoder/vp8.rs:553-670 (+ partitions :421-450, quant :452-504)
int parse_header(DecFrame& F, const uint8_t* data, size_t len);
// MB headers + tokens for the whole frame as packed records in raster order
// into recs (room for nmb * ZW_DREC_MAX bytes); moff[i] = byte offset of MB i's
// record (moff[nmb] = total).
int parse_mbs(DecFrame& F, uint8_t* recs, uint32_t* moff);
// The first partition's half of parse_mbs for the device token parse: each
// MB's first ZW_TOK_MODE record header bytes into mrec.
int parse_modes(DecFrame& F, uint8_t* mrec);
// calculate_filter_parameters decoder/vp8.rs:1470-1523, tabulated per (segment, is_i4).
void filter_table(ZwFilterParams& fp, int filter_type, int filter_level, int sharpness, int seg_enabled, int seg_delta,
                  const int8_t* seg_lf, int adj, int ref_delta0, int mode_delta0, int mbw, int mbh);
// The 14-bit width and height in a frame's first ten bytes, before any other
// check (parse_header validates the rest); false when data is null or shorter.
bool peek_dims(const uint8_t* data, size_t len, int* width, int* height);

}  // namespace zwdec
#pragma GCC visibility pop
