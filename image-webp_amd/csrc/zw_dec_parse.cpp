// zw_dec_parse.cpp -- the decoder's CPU-only code (zw_dec_parse.h):
//
//   frame header (decoder/vp8.rs:553-670), partitions (:421-450), quantiser
//   indices (:452-504), MB modes (:681-734) and residual tokens (:872-1058) ->
//   one packed record per macroblock.  The boolean decoder follows
//   decoder/bit_reader.rs (libwebp-style 56-bit refill, one zero byte past the
//   end then eof).  Then the CPU replay of the device token parse
//   (zw_dbg_tokl_frame), the resampling rule's host hook (zw_dbg_resize_taps)
//   and the WebP container parser (zw_webp_parse).
#include "zw_dec_parse.h"

#include <cstring>
#include <vector>

#include "../../include/zwebp.h"
#include "zw_vp8_tables.h"
#include "zw_tokl.h"
#include "zw_resize.h"

using namespace zwh;

namespace zwdec {

// read_frame_header decoder/vp8.rs:553-670 (+ partitions :421-450, quant :452-504)
int parse_header(DecFrame& F, const uint8_t* data, size_t len)
{
    if (len < 3) return ZW_EBITSTREAM;
    const uint32_t tag = data[0] | (data[1] << 8) | (data[2] << 16);
    if (tag & 1) return ZW_EUNSUPPORTED_FEATURE;  // interframes
    const uint32_t fps = tag >> 5;
    if (len < 6) return ZW_EBITSTREAM;
    if (data[3] != 0x9d || data[4] != 0x01 || data[5] != 0x2a) return ZW_EVP8_MAGIC;
    if (len < 10) return ZW_EBITSTREAM;
    F.width = (data[6] | (data[7] << 8)) & 0x3fff;
    F.height = (data[8] | (data[9] << 8)) & 0x3fff;
    F.mbw = (F.width + 15) / 16;
    F.mbh = (F.height + 15) / 16;
    size_t off = 10;
    if (len - off < fps) return ZW_EBITSTREAM;
    if (fps == 0) return ZW_ENOT_ENOUGH_INIT_DATA;
    BitReader& b = F.hdr;
    b.init(data + off, fps);
    off += fps;
    const int cs = b.lit(1);
    (void)b.lit(1);
    if (cs != 0) return ZW_ECOLORSPACE;
    F.segments_enabled = b.bit(128);
    int delta_values[4] = {0, 0, 0, 0};
    if (F.segments_enabled) {
        F.seg_update_map = b.bit(128);
        if (b.bit(128)) {
            const int mode = b.bit(128);
            for (int i = 0; i < 4; i++) delta_values[i] = !mode;
            for (int i = 0; i < 4; i++) F.seg_quant[i] = (int8_t)b.sgn(7);
            for (int i = 0; i < 4; i++) F.seg_lf[i] = (int8_t)b.sgn(6);
        }
        if (F.seg_update_map)
            for (int i = 0; i < 3; i++) F.seg_probs[i] = b.bit(128) ? (uint8_t)b.lit(8) : 255;
        if (b.eof) return ZW_EBITSTREAM;
    }
    F.filter_type = b.bit(128);
    F.filter_level = b.lit(6);
    F.sharpness = b.lit(3);
    F.lf_adj_enabled = b.bit(128);
    if (F.lf_adj_enabled) {
        if (b.bit(128)) {
            int rd[4], md[4];
            for (int i = 0; i < 4; i++) rd[i] = b.sgn(6);
            for (int i = 0; i < 4; i++) md[i] = b.sgn(6);
            F.ref_delta0 = rd[0];
            F.mode_delta0 = md[0];
        }
        if (b.eof) return ZW_EBITSTREAM;
    }
    F.nparts = 1 << b.lit(2);
    if (b.eof) return ZW_EBITSTREAM;
    const size_t sz_off = off;
    if (F.nparts > 1) {
        if (len - off < (size_t)(3 * F.nparts - 3)) return ZW_EBITSTREAM;
        off += 3 * F.nparts - 3;
    }
    for (int p = 0; p < F.nparts; p++) {
        size_t psz;
        if (p < F.nparts - 1) {
            const uint8_t* s = data + sz_off + 3 * p;
            psz = s[0] | (s[1] << 8) | (s[2] << 16);
            if (len - off < psz) return ZW_EBITSTREAM;
        } else {
            psz = len - off;
        }
        F.part[p].init(data + off, psz);
        off += psz;
    }
    const int yac = b.lit(7);
    const int ydc_d = b.sgn(4), y2dc_d = b.sgn(4), y2ac_d = b.sgn(4), uvdc_d = b.sgn(4), uvac_d = b.sgn(4);
    const int n = F.segments_enabled ? 4 : 1;
    for (int i = 0; i < n; i++) {
        const int base = F.segments_enabled ? (delta_values[i] ? F.seg_quant[i] + yac : F.seg_quant[i]) : yac;
        DecQuant& s = F.q[i];
        s.ydc = DC_QUANT[clampi(base + ydc_d, 0, 127)];
        s.yac = AC_QUANT[clampi(base, 0, 127)];
        s.y2dc = DC_QUANT[clampi(base + y2dc_d, 0, 127)] * 2;
        s.y2ac = AC_QUANT[clampi(base + y2ac_d, 0, 127)] * 155 / 100;
        s.uvdc = DC_QUANT[clampi(base + uvdc_d, 0, 127)];
        s.uvac = AC_QUANT[clampi(base + uvac_d, 0, 127)];
        if (s.y2ac < 8) s.y2ac = 8;
        if (s.uvdc > 132) s.uvdc = 132;
    }
    for (int i = n; i < 4; i++) F.q[i] = F.q[0];
    if (b.eof) return ZW_EBITSTREAM;
    (void)b.lit(1);  // refresh_entropy_probs
    memcpy(F.probs, COEFF_PROBS, sizeof F.probs);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++)
            for (int k = 0; k < 3; k++)
                for (int t = 0; t < 11; t++)
                    if (b.bit(COEFF_UPDATE_PROBS[i][j][k][t])) F.probs[i][j][k][t] = (uint8_t)b.lit(8);
    if (b.eof) return ZW_EBITSTREAM;
    F.skip_prob = b.lit(1) ? b.lit(8) : -1;
    if (b.eof) return ZW_EBITSTREAM;
    F.seg_delta_values = delta_values[0];
    return ZW_OK;
}

// read_coefficients decoder/vp8.rs:872-1058: one block's levels (not
// dequantised), written as the zigzag prefix straight into dst (the packed
// record's level array, zw_common.h ZW_DREC_*): positions 0..eob-1, zeros
// included (position 0 is 0 when first = 1); *eob = last nonzero position + 1.
// Returns -1 on eof, else whether the run was non-empty.
static int read_levels_into(BitReader& r, const uint8_t P[8][3][11], int16_t* dst, int first, int ctx, int* eob)
{
    *eob = 0;
    int n = first, written = 0;
    const uint8_t* p = P[COEFF_BANDS[n]][ctx];
    while (n < 16) {
        if (!r.bit(p[0])) break;
        while (!r.bit(p[1])) {
            n++;
            if (n >= 16) return r.eof ? -1 : 1;
            p = P[COEFF_BANDS[n]][0];
        }
        int v, nctx;
        if (!r.bit(p[2])) {
            v = 1;
            nctx = 1;
        } else {
            if (!r.bit(p[3])) {
                if (!r.bit(p[4])) v = 2;
                else v = 3 + r.bit(p[5]);
            } else if (!r.bit(p[6])) {
                if (!r.bit(p[7])) v = 5 + r.bit(159);
                else {
                    v = 7 + 2 * r.bit(165);
                    v += r.bit(145);
                }
            } else {
                const int b1 = r.bit(p[8]);
                const int b0 = r.bit(p[9 + b1]);
                const int cat = 2 * b1 + b0;
                const uint8_t* cp = PROB_DCT_CAT[2 + cat];
                int extra = 0;
                for (int k = 0; k < 12 && cp[k]; k++) extra = extra + extra + r.bit(cp[k]);
                v = 3 + (8 << cat) + extra;
            }
            nctx = 2;
        }
        while (written < n) dst[written++] = 0;
        dst[n] = (int16_t)(r.bit(128) ? -v : v);
        written = n + 1;
        n++;
        *eob = n;
        if (n < 16) p = P[COEFF_BANDS[n]][nctx];
    }
    if (r.eof) return -1;
    return n > first;
}

// MB headers + tokens for the whole frame (decoder/vp8.rs:681-734, :1060-1168),
// as packed records in raster order into recs (room for nmb * ZW_DREC_MAX
// bytes); moff[i] = byte offset of MB i's record (moff[nmb] = total).
int parse_mbs(DecFrame& F, uint8_t* recs, uint32_t* moff)
{
    size_t used = 0;
    const int mbw = F.mbw, mbh = F.mbh;
    std::vector<uint8_t> top_cx((size_t)mbw * 9, 0), top_bp((size_t)mbw * 4, 0);
    BitReader& b = F.hdr;
    for (int mby = 0; mby < mbh; mby++) {
        BitReader& pr = F.part[mby % F.nparts];
        uint8_t left_cx[9] = {0}, left_bp[4] = {0};
        for (int mbx = 0; mbx < mbw; mbx++) {
            moff[(size_t)mby * mbw + mbx] = (uint32_t)used;
            // the record is built in place: header, level starts, levels
            uint8_t* rec = recs + used;
            memset(rec, 0, ZW_DREC_HDR);
            uint16_t* start = (uint16_t*)(rec + 16);
            int16_t* lv = (int16_t*)(rec + ZW_DREC_HDR);
            uint8_t* tcx = &top_cx[(size_t)mbx * 9];
            uint8_t* tbp = &top_bp[(size_t)mbx * 4];
            int seg = 0;
            if (F.segments_enabled && F.seg_update_map) seg = b.tree(SEGMENT_ID_TREE, F.seg_probs);
            const int skip = F.skip_prob >= 0 ? b.bit(F.skip_prob) : 0;
            const int lm = b.tree(YMODE_TREE, KEYFRAME_YMODE_PROBS);
            if (lm == 4) {
                for (int y = 0; y < 4; y++)
                    for (int x = 0; x < 4; x++) {
                        const int m = b.tree(BMODE_TREE, KEYFRAME_BPRED_MODE_PROBS[tbp[x]][left_bp[y]]);
                        rec[8 + ((x + y * 4) >> 1)] |= (uint8_t)(m << (4 * ((x + y * 4) & 1)));
                        tbp[x] = (uint8_t)m;
                        left_bp[y] = (uint8_t)m;
                    }
            } else {
                static const uint8_t intra_of[4] = {0, 2, 3, 1};  // DC,V,H,TM -> B_DC,B_VE,B_HE,B_TM
                for (int i = 0; i < 4; i++) tbp[i] = left_bp[i] = intra_of[lm];
            }
            const int cm = b.tree(UVMODE_TREE, KEYFRAME_UV_MODE_PROBS);
            if (b.eof) return ZW_EBITSTREAM;
            rec[0] = (uint8_t)(lm | (cm << 3) | (skip << 5));
            rec[1] = (uint8_t)seg;
            if (skip) {
                if (lm != 4) left_cx[0] = tcx[0] = 0;
                for (int i = 1; i < 9; i++) left_cx[i] = tcx[i] = 0;
                used += ZW_DREC_HDR;  // no levels (every start 0); 80 is a multiple of 16
                continue;
            }
            uint32_t nzm = 0;
            int first = 0, eob, nlv = 0;
            if (lm != 4) {  // Y2 (parsed first) goes first
                const int nz = read_levels_into(pr, F.probs[1], lv, 0, tcx[0] + left_cx[0], &nlv);
                if (nz < 0) return ZW_EBITSTREAM;
                left_cx[0] = tcx[0] = (uint8_t)nz;
                first = 1;
            }
            auto block = [&](int i, const uint8_t P[8][3][11], int fst, int ctx) -> int {
                start[i] = (uint16_t)nlv;
                const int nz = read_levels_into(pr, P, lv + nlv, fst, ctx, &eob);
                if (nz > 0 && fst == 1) lv[nlv] = 0;  // position 0 of an I16 luma block
                nlv += eob;
                return nz;
            };
            const int plane = lm != 4 ? 0 : 3;
            for (int y = 0; y < 4; y++) {
                int left = left_cx[y + 1];
                for (int x = 0; x < 4; x++) {
                    const int i = x + y * 4;
                    const int nz = block(i, F.probs[plane], first, tcx[x + 1] + left);
                    if (nz < 0) return ZW_EBITSTREAM;
                    nzm |= (uint32_t)nz << i;
                    left = nz;
                    tcx[x + 1] = (uint8_t)nz;
                }
                left_cx[y + 1] = (uint8_t)left;
            }
            for (int j = 5; j <= 7; j += 2) {
                for (int y = 0; y < 2; y++) {
                    int left = left_cx[y + j];
                    for (int x = 0; x < 2; x++) {
                        const int i = x + y * 2 + (j == 5 ? 16 : 20);
                        const int nz = block(i, F.probs[2], 0, tcx[x + j] + left);
                        if (nz < 0) return ZW_EBITSTREAM;
                        nzm |= (uint32_t)nz << i;
                        left = nz;
                        tcx[x + j] = (uint8_t)nz;
                    }
                    left_cx[y + j] = (uint8_t)left;
                }
            }
            start[24] = (uint16_t)nlv;  // the end of block 23
            memcpy(rec + 4, &nzm, 4);
            const size_t bytes = ZW_DREC_HDR + (size_t)nlv * 2, padded = (bytes + 15) & ~(size_t)15;
            memset(rec + bytes, 0, padded - bytes);
            used += padded;
        }
    }
    moff[(size_t)mbw * mbh] = (uint32_t)used;
    return ZW_OK;
}

// The first partition's half of parse_mbs for the device token parse
// (k_dec_tokl): each MB's modes, segment, skip flag and I4 sub-modes as the
// first ZW_TOK_MODE bytes of its record header (decoder/vp8.rs:681-734), from
// the same bool decoder in the same order, so the same streams fail.
int parse_modes(DecFrame& F, uint8_t* mrec)
{
    const int mbw = F.mbw, mbh = F.mbh;
    std::vector<uint8_t> top_bp((size_t)mbw * 4, 0);
    BitReader& b = F.hdr;
    for (int mby = 0; mby < mbh; mby++) {
        uint8_t left_bp[4] = {0};
        for (int mbx = 0; mbx < mbw; mbx++) {
            uint8_t* rec = mrec + ((size_t)mby * mbw + mbx) * ZW_TOK_MODE;
            memset(rec, 0, ZW_TOK_MODE);
            uint8_t* tbp = &top_bp[(size_t)mbx * 4];
            int seg = 0;
            if (F.segments_enabled && F.seg_update_map) seg = b.tree(SEGMENT_ID_TREE, F.seg_probs);
            const int skip = F.skip_prob >= 0 ? b.bit(F.skip_prob) : 0;
            const int lm = b.tree(YMODE_TREE, KEYFRAME_YMODE_PROBS);
            if (lm == 4) {
                for (int y = 0; y < 4; y++)
                    for (int x = 0; x < 4; x++) {
                        const int m = b.tree(BMODE_TREE, KEYFRAME_BPRED_MODE_PROBS[tbp[x]][left_bp[y]]);
                        rec[8 + ((x + y * 4) >> 1)] |= (uint8_t)(m << (4 * ((x + y * 4) & 1)));
                        tbp[x] = (uint8_t)m;
                        left_bp[y] = (uint8_t)m;
                    }
            } else {
                static const uint8_t intra_of[4] = {0, 2, 3, 1};  // DC,V,H,TM -> B_DC,B_VE,B_HE,B_TM
                for (int i = 0; i < 4; i++) tbp[i] = left_bp[i] = intra_of[lm];
            }
            const int cm = b.tree(UVMODE_TREE, KEYFRAME_UV_MODE_PROBS);
            if (b.eof) return ZW_EBITSTREAM;
            rec[0] = (uint8_t)(lm | (cm << 3) | (skip << 5));
            rec[1] = (uint8_t)seg;
        }
    }
    return ZW_OK;
}

// calculate_filter_parameters decoder/vp8.rs:1470-1523, tabulated per
// (segment, is_i4).
void filter_table(ZwFilterParams& fp, int filter_type, int filter_level, int sharpness, int seg_enabled, int seg_delta,
                  const int8_t* seg_lf, int adj, int ref_delta0, int mode_delta0, int mbw, int mbh)
{
    memset(&fp, 0, sizeof fp);
    fp.filter_type = filter_type;
    fp.mbw = mbw;
    fp.mbh = mbh;
    for (int s = 0; s < 4; s++)
        for (int i4 = 0; i4 < 2; i4++) {
            int fl = filter_level, L = 0, I = 0, H = 0;
            if (fl != 0) {
                if (seg_enabled) fl = seg_delta ? fl + seg_lf[s] : seg_lf[s];
                fl = clampi(fl, 0, 63);
                if (adj) {
                    fl += ref_delta0;
                    if (i4) fl += mode_delta0;
                }
                fl = clampi(fl, 0, 63);
                int il = fl;
                if (sharpness > 0) {
                    il >>= sharpness > 4 ? 2 : 1;
                    if (il > 9 - sharpness) il = 9 - sharpness;
                }
                if (il == 0) il = 1;
                L = fl;
                I = il;
                H = fl >= 40 ? 2 : (fl >= 15 ? 1 : 0);
            }
            fp.level[s][i4] = (uint8_t)L;
            fp.ilimit[s][i4] = (uint8_t)I;
            fp.hev[s][i4] = (uint8_t)H;
        }
}

bool peek_dims(const uint8_t* data, size_t len, int* width, int* height)
{
    if (!data || len < 10) return false;
    *width = (data[6] | (data[7] << 8)) & 0x3fff;
    *height = (data[8] | (data[9] << 8)) & 0x3fff;
    return true;
}

}  // namespace zwdec

using namespace zwdec;

// ---------------------------------------------------------------------------
// CPU check of the device token parse (zw_tokl.h, the code k_dec_tok1 and
// k_dec_tok2 run per lane): the same functions step one frame here over host
// memory -- stage 1 over the whole frame (snapshots), stage 2 per MB from each
// snapshot (count, offsets, records) -- and the records must equal parse_mbs's
// byte for byte (or both fail).  Test hook only (tests/test_tokl.py); no device work.
// ---------------------------------------------------------------------------
namespace {
static uint64_t host_bits64(const uint8_t* stream, size_t len, uint32_t bp)
{
    uint64_t v = 0;
    const size_t b0 = bp >> 3;
    for (int i = 0; i < 9; i++) {
        const uint64_t byte = b0 + i < len ? stream[b0 + i] : 0;
        if (i < 8) v = (v << 8) | byte;
        else v = (bp & 7) ? (v << (bp & 7)) | (byte >> (8 - (bp & 7))) : v;
    }
    return v;
}

struct HostTok1Mem {
    static constexpr uint32_t U = 1;
    const uint32_t* T1;
    const uint8_t* P;
    const uint8_t* stream;
    size_t len;
    const uint8_t* modes;
    uint32_t nmb, mbw;
    std::vector<uint16_t> tcxv;
    std::vector<uint32_t> snaps;  // 4 words per MB
    uint32_t prob_at(uint32_t a) const { return P[a]; }
    void tt1(uint32_t s8, uint32_t& t0, uint32_t& t1) const
    {
        t0 = T1[s8 / 4];
        t1 = T1[s8 / 4 + 1];
    }
    void desc1(uint32_t i, uint32_t* d) const { tok1::desc1<1>(i / tok1::NDESC1, i % tok1::NDESC1, d); }
    uint64_t bits64(uint32_t bp) const { return host_bits64(stream, len, bp); }
    uint32_t cls(uint32_t mbi) const
    {
        const uint8_t b0 = modes[(size_t)mbi * ZW_TOK_MODE];
        return (uint32_t)((b0 & 7) == 4) | ((uint32_t)((b0 >> 5) & 1) << 1);
    }
    uint32_t tcx(uint32_t mbx) const { return tcxv[mbx]; }
    void set_tcx(uint32_t mbx, uint32_t v) { tcxv[mbx] = (uint16_t)v; }
    void snap(bool c, uint32_t mbi, uint32_t s0, uint32_t s1, uint32_t tl)
    {
        if (!c) return;
        uint32_t* w = &snaps[(size_t)mbi * 4];
        w[0] = s0;
        w[1] = s1;
        w[2] = tl;
        w[3] = 0;
    }
};

struct HostTok2Mem {
    static constexpr uint32_t U = 1;
    static constexpr uint32_t lane0 = 0;
    const uint32_t* TT;
    const uint8_t* P;
    const uint8_t* stream;
    size_t len;
    uint8_t* rec = nullptr;  // null: count only
    uint32_t lim = 0;        // the MB's record end (stores past it belong to the next MB)

    void tt(uint32_t st, uint32_t& t0, uint32_t& t1) const
    {
        t0 = TT[2 * st];
        t1 = TT[2 * st + 1];
    }
    void desc(uint32_t i, uint32_t* d) const { tokl::desc(i / tokl::NDESC, i % tokl::NDESC, d); }
    uint32_t prob_at(uint32_t i) const { return P[i]; }
    uint64_t bits64(uint32_t bp) const { return host_bits64(stream, len, bp); }
    void st16c(bool c, uint32_t off, uint32_t v)
    {
        const uint16_t h = (uint16_t)v;
        if (rec && c && off < lim) memcpy(rec + off, &h, 2);
    }
    void st128(uint32_t off, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
    {
        const uint32_t w[4] = {a, b, c, d};
        if (rec) memcpy(rec + off, w, 16);
    }
};

// stage 2 for MB i of a frame (its record at hb); returns the record's bytes, *bad = the eof rule failed
static uint32_t host_tok2_mb(HostTok2Mem& m, const uint8_t* modes, const uint32_t* snap, uint32_t hb, bool* bad)
{
    uint32_t mr[4];
    memcpy(mr, modes, 16);
    if ((mr[0] >> 5) & 1u) {
        tokl::mb_skip(m, hb, mr);
        return ZW_DREC_HDR;
    }
    tokl::Lane L;
    tokl::from_snapshot(L, m, snap[0], snap[1], (uint32_t)m.len);
    L.hb = hb;
    tokl::mb_begin(L, m, mr, snap[2]);
    while (L.phase == tokl::PH_DECIDE) {
        if (L.vb < 8) tokl::topup(L, m);
        tokl::step(L, m);
    }
    tokl::mb_end(L, m);
    *bad = *bad || L.bad;
    return L.hb - hb;
}
}  // namespace

// zw_resize.h's tap function on the host (the one k_yuv2rgb_resize runs per pixel).
extern "C" int zw_dbg_resize_taps(uint32_t src, uint32_t dst, uint32_t o, int32_t out[3])
{
    if (!out || src == 0 || dst == 0 || o >= dst || src > (1u << 23)) return ZW_EINVAL;
    const ZwTap t = zw_resize_tap(src, dst, o);
    out[0] = t.i0;
    out[1] = t.i1;
    out[2] = t.f;
    return ZW_OK;
}

// zw_resize.h's antialiased taps on the host (the functions k_resize_aa_weights runs).
extern "C" int zw_dbg_resize_aa_taps(uint32_t src, uint32_t dst, uint32_t o, int32_t* first, int32_t* count,
                                     uint16_t* weights, int cap)
{
    if (!first || !count || !weights || src == 0 || dst == 0 || o >= dst || src > (1u << 23)) return ZW_EINVAL;
    const ZwAaSpan s = zw_resize_aa_span(src, dst, o);
    if (cap < s.count) return ZW_EINVAL;
    *first = s.first;
    *count = s.count;
    zw_resize_aa_weights(src, dst, o, s, [&](int32_t k, uint32_t w) { weights[k] = (uint16_t)w; });
    return ZW_OK;
}

extern "C" int zw_dbg_tokl_frame(const uint8_t* vp8, size_t len, int* match)
{
    if (!match || (!vp8 && len)) return ZW_EINVAL;
    *match = -1;
    DecFrame A, B;
    if (int r = parse_header(A, vp8, len)) return r;
    (void)parse_header(B, vp8, len);
    const size_t nmb = (size_t)A.mbw * A.mbh;
    if (nmb == 0) return ZW_EINVALID_DIMENSIONS;
    std::vector<uint8_t> ref(nmb * ZW_DREC_MAX), modes(nmb * ZW_TOK_MODE);
    std::vector<uint32_t> moff_ref(nmb + 1), moff(nmb + 1);
    const int rc = parse_mbs(A, ref.data(), moff_ref.data());
    if (B.nparts != 1 || B.mbw < 2 || parse_modes(B, modes.data()) != ZW_OK) return rc;  // the host keeps such frames
    // stage 1
    static const tok1::Table<1> T1;
    HostTok1Mem m1;
    m1.T1 = T1.e;
    m1.P = &B.probs[0][0][0][0];
    m1.stream = B.part[0].d;
    m1.len = B.part[0].len;
    m1.modes = modes.data();
    m1.nmb = (uint32_t)nmb;
    m1.mbw = (uint32_t)B.mbw;
    m1.tcxv.assign(B.mbw + 1, 0);
    m1.snaps.assign(nmb * 4, 0);
    tok1::Lane1 L1;
    tok1::init1(L1, true);
    for (uint64_t st = 0; L1.k != tok1::K_DONE; st++) {
        if ((st & 7) == 0) tok1::topup1(L1, m1);  // (the device's schedule)
        tok1::step1(L1, m1);  // (as the device: a lane waiting for its MB phase steps in SINK)
        if ((st & 15) == 15)
            for (int r = 0; r < 8 && L1.k == tok1::K_MB; r++) tok1::mb1(L1, m1);
    }
    // stage 2: count, offsets, records
    static const uint32_t TT[2 * tokl::NST] = ZW_TOKL_TT_INIT;
    HostTok2Mem m2;
    m2.TT = TT;
    m2.P = &B.probs[0][0][0][0];
    m2.stream = B.part[0].d;
    m2.len = B.part[0].len;
    bool bad = false;
    moff[0] = 0;
    for (size_t i = 0; i < nmb; i++)
        moff[i + 1] = moff[i] + host_tok2_mb(m2, modes.data() + i * ZW_TOK_MODE, &m1.snaps[i * 4], 0, &bad);
    std::vector<uint8_t> rec(moff[nmb] + 16);
    m2.rec = rec.data();
    bool bad2 = false;
    for (size_t i = 0; i < nmb; i++) {
        m2.lim = moff[i + 1];
        const uint32_t sz = host_tok2_mb(m2, modes.data() + i * ZW_TOK_MODE, &m1.snaps[i * 4], moff[i], &bad2);
        if (sz != moff[i + 1] - moff[i]) return ZW_EINVAL;  // (the two passes must agree)
    }
    if (rc != ZW_OK || bad) {
        *match = (rc == ZW_EBITSTREAM && bad) ? 1 : 0;
        return rc;
    }
    *match = moff == moff_ref && !memcmp(rec.data(), ref.data(), moff_ref[nmb]) ? 1 : 0;
    return rc;
}

// ---------------------------------------------------------------------------
// WebP container, lossy subset: WebPDecoder::new -> read_data
// (decoder/api.rs:334-510) for a simple "VP8 " file or a VP8X file whose image
// is a VP8 chunk, then read_image (:640-700) + decode_rgb / decode_rgba
// (:938-993).  Lossless (VP8L) and animation are outside the lossy
// block-transform path: ZW_EUNSUPPORTED, and so is alpha (ALPH) unless the
// caller opts in with ZW_WEBP_ALPHA (zw_webp_parse_ex); a still VP8L image
// parses with ZW_WEBP_LOSSLESS.
// ---------------------------------------------------------------------------
namespace {
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t rd24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
bool fourcc_is(const uint8_t* p, const char* s) { return memcmp(p, s, 4) == 0; }
}  // namespace

// The first five bytes of a VP8L payload (decoder/api.rs:378-395): the signature
// byte, 14 + 14 bits of size, the alpha bit (bit 28 of the four bytes after the
// signature) and a 3-bit version that must be 0.
static int vp8l_header(const uint8_t* p, uint64_t avail, uint32_t* w, uint32_t* h, int* alpha)
{
    if (avail < 5) return ZW_EBITSTREAM;
    if (p[0] != 0x2f) return ZW_ELOSSLESS_SIGNATURE;
    const uint32_t v = rd32(p + 1);
    if (v >> 29) return ZW_EVERSION_NUMBER;
    *w = (v & 0x3fff) + 1;
    *h = ((v >> 14) & 0x3fff) + 1;
    *alpha = (int)((v >> 28) & 1u);
    return ZW_OK;
}

// zw_webp_parse (flags 0) and zw_webp_parse_ex: with ZW_WEBP_ALPHA a VP8X file
// with the alpha flag and a "VP8 " chunk parses, its first ALPH chunk recorded;
// the flag without the chunk is ChunkMissing (read_image, decoder/api.rs:675-678).
// With ZW_WEBP_LOSSLESS a simple "VP8L" file and a VP8X file whose image is a
// "VP8L" chunk parse, vp8_offset / vp8_len giving that chunk's payload.
static int webp_parse_flags(const uint8_t* data, size_t len, int flags, zw_webp_info_ex* info)
{
    memset(info, 0, sizeof *info);
    if (len < 8) return ZW_EBITSTREAM;
    if (!fourcc_is(data, "RIFF")) return ZW_ECHUNK_HEADER;  // ChunkHeaderInvalid(b"RIFF")
    const uint64_t riff_size = rd32(data + 4);
    if (len < 12) return ZW_EBITSTREAM;
    if (!fourcc_is(data + 8, "WEBP")) return ZW_EWEBP_SIGNATURE;
    if (len < 20) return ZW_EBITSTREAM;
    const uint8_t* ch = data + 12;
    const uint64_t csize = rd32(ch + 4), crounded = csize + (csize & 1);
    const uint64_t start = 20;
    if (fourcc_is(ch, "VP8 ")) {
        if (len < start + 10) return ZW_EBITSTREAM;
        const uint32_t tag = rd24(data + start);
        if (tag & 1) return ZW_EUNSUPPORTED_FEATURE;  // non-keyframe
        const uint8_t* m = data + start + 3;
        if (m[0] != 0x9d || m[1] != 0x01 || m[2] != 0x2a) return ZW_EVP8_MAGIC;
        info->width = (data[start + 6] | (data[start + 7] << 8)) & 0x3fff;
        info->height = (data[start + 8] | (data[start + 9] << 8)) & 0x3fff;
        if (info->width == 0 || info->height == 0) return ZW_EINCONSISTENT_SIZES;
        info->is_lossy = 1;
        info->vp8_offset = start;
        info->vp8_len = csize;
    } else if (fourcc_is(ch, "VP8L")) {
        info->is_lossless = 1;
        if (!(flags & ZW_WEBP_LOSSLESS)) return ZW_EUNSUPPORTED;
        if (int r = vp8l_header(data + start, len - start, &info->width, &info->height, &info->has_alpha)) return r;
        info->vp8_offset = start;
        info->vp8_len = csize;
    } else if (fourcc_is(ch, "VP8X")) {
        if (len < start + 10) return ZW_EBITSTREAM;
        const uint8_t chunk_flags = data[start];
        info->has_alpha = (chunk_flags & 0x10) != 0;
        info->is_animated = (chunk_flags & 0x02) != 0;
        info->width = rd24(data + start + 4) + 1;
        info->height = rd24(data + start + 7) + 1;
        if ((uint64_t)info->width * info->height > 0xffffffffull) return ZW_EIMAGE_TOO_LARGE;
        uint64_t pos = start + crounded;
        const uint64_t max_pos = pos + (riff_size > 12 ? riff_size - 12 : 0);
        int have_vp8 = 0, have_vp8l = 0, have_alph = 0;
        uint64_t vp8l_off = 0, vp8l_len = 0;
        while (pos < max_pos) {
            if (pos + 8 > len) break;  // read_chunk_header hits the end: BitStreamError -> stop scanning
            const uint8_t* c = data + pos;
            const uint64_t sz = rd32(c + 4), rsz = sz + (sz & 1);
            if (fourcc_is(c, "VP8 ") && !have_vp8) {
                have_vp8 = 1;
                info->vp8_offset = pos + 8;
                info->vp8_len = sz;
            } else if (fourcc_is(c, "VP8L")) {
                if (!have_vp8l && !have_vp8) {
                    vp8l_off = pos + 8;
                    vp8l_len = sz;
                }
                have_vp8l = 1;
            } else if (fourcc_is(c, "ALPH") && !have_alph) {
                have_alph = 1;
                info->alph_offset = pos + 8;
                info->alph_len = sz;
            }
            pos += 8 + rsz;
        }
        info->is_lossy = have_vp8;
        info->is_lossless = have_vp8l && !have_vp8;
        if ((flags & ZW_WEBP_LOSSLESS) && info->is_lossless && !info->is_animated) {
            // the image is the VP8L chunk (read_image, decoder/api.rs:648-660); has_alpha stays the VP8X flag
            if (vp8l_off + vp8l_len > len) return ZW_EBITSTREAM;
            uint32_t lw = 0, lh = 0;
            int la = 0;
            if (int r = vp8l_header(data + vp8l_off, vp8l_len, &lw, &lh, &la)) return r;
            info->vp8_offset = vp8l_off;
            info->vp8_len = vp8l_len;
            return ZW_OK;
        }
        const bool alpha_ok = (flags & ZW_WEBP_ALPHA) && have_vp8;
        if (info->is_animated || have_vp8l || (info->has_alpha && !alpha_ok)) return ZW_EUNSUPPORTED;
        if (!have_vp8) return ZW_ECHUNK_MISSING;
        if (info->has_alpha) {
            if (!have_alph) return ZW_ECHUNK_MISSING;
            if (info->alph_offset + info->alph_len > len) return ZW_EBITSTREAM;
        }
    } else {
        return ZW_ECHUNK_HEADER;
    }
    if (info->vp8_offset + info->vp8_len > len) return ZW_EBITSTREAM;
    return ZW_OK;
}

extern "C" int zw_webp_parse_ex(const uint8_t* data, size_t len, int flags, zw_webp_info_ex* info)
{
    if (!info || (!data && len) || (flags & ~(ZW_WEBP_ALPHA | ZW_WEBP_LOSSLESS))) return ZW_EINVAL;
    return webp_parse_flags(data, len, flags, info);
}

extern "C" int zw_webp_parse(const uint8_t* data, size_t len, zw_webp_info* info)
{
    if (!info || (!data && len)) return ZW_EINVAL;
    zw_webp_info_ex e;
    const int r = webp_parse_flags(data, len, 0, &e);
    memset(info, 0, sizeof *info);
    info->width = e.width;
    info->height = e.height;
    info->has_alpha = e.has_alpha;
    info->is_lossy = e.is_lossy;
    info->is_lossless = e.is_lossless;
    info->is_animated = e.is_animated;
    info->vp8_offset = e.vp8_offset;
    info->vp8_len = e.vp8_len;
    return r;
}
