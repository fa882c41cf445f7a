// zw_host_entropy.h -- host half of the encoder, everything but the coder
// (zw_host_emit.h): the packed record view, statistics, probabilities, level
// costs, contexts and the headers' decisions.  Restates, for the product path:
//   record_coeffs / ProbaStats      encoder/cost.rs:1173-1397
//   compute_updated_probabilities   encoder/vp8.rs:1202-1238
//   LevelCosts::calculate           encoder/cost.rs:1500-1545
//   headers                         encoder/vp8.rs:332-560
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "zw_common.h"
#include "zw_vp8_tables.h"

namespace zwh {

// Path of `value` through a VP8 tree (write_with_tree_start_index,
// arithmetic.rs:120): bits root-first and the probability index of each.
inline int tree_path(const int8_t* t, int tlen, int value, int start, uint8_t* bits, uint8_t* pidx)
{
    int cur = -1;
    for (int i = 0; i < tlen; i++)
        if (t[i] == -value) { cur = i; break; }
    int enc[16], pr[16], cnt = 0;
    for (;;) {
        if (cur == start) { enc[cnt] = 0; pr[cnt++] = cur / 2; break; }
        if (cur == start + 1) { enc[cnt] = 1; pr[cnt++] = cur / 2; break; }
        int ev = 0;
        if (cur % 2) { cur -= 1; ev = 1; }
        enc[cnt] = ev;
        pr[cnt++] = cur / 2;
        int pi = -1;
        for (int i = 0; i < tlen; i++)
            if (t[i] == cur) { pi = i; break; }
        cur = pi;
    }
    for (int i = 0; i < cnt; i++) {
        bits[i] = (uint8_t)enc[cnt - 1 - i];
        pidx[i] = (uint8_t)pr[cnt - 1 - i];
    }
    return cnt;
}

// Precomputed paths of the mode trees (the per-MB header symbols).
struct TreePaths {
    uint8_t n[10], bits[10][16], pidx[10][16];
    TreePaths(const int8_t* t, int tlen, int nsym)
    {
        for (int v = 0; v < nsym; v++) n[v] = (uint8_t)tree_path(t, tlen, v, 0, bits[v], pidx[v]);
    }
    template <class Enc>
    void put(Enc& E, const uint8_t* probs, int v) const
    {
        E.path(bits[v], pidx[v], n[v], probs);
    }
};

// TOKEN_TREE paths for tokens 0..11 from start index 0 / 2 (after a zero token)
struct TokenPaths {
    uint8_t n[2][12], bits[2][12][12], pidx[2][12][12];
    TokenPaths()
    {
        for (int s = 0; s < 2; s++)
            for (int v = 0; v < 12; v++) n[s][v] = (uint8_t)tree_path(TOKEN_TREE, 22, v, 2 * s, bits[s][v], pidx[s][v]);
    }
};
inline const TokenPaths& token_paths()
{
    static const TokenPaths P;
    return P;
}

inline uint16_t bitcost(int bit, int p) { return bit ? VP8_ENTROPY_COST[255 - p] : VP8_ENTROPY_COST[p]; }

// Packed MB record view (zw_pack_kernels.hip): header, sub-modes, eobs and a
// pointer to each block's zigzag levels (little-endian i16, eob of them).
struct PackedMb {
    int luma, skip, segment, chroma;
    uint8_t bpred[16];
    const uint8_t* eob;
    const uint8_t* lv[25];
};
inline const uint8_t* view_mb(const uint8_t* p, PackedMb& m)
{
    const uint8_t h = p[0];
    m.luma = h & 7;
    m.skip = (h >> 3) & 1;
    m.segment = (h >> 4) & 3;
    m.chroma = h >> 6;
    p++;
    if (m.luma == 4) {
        for (int i = 0; i < 8; i++) {
            m.bpred[2 * i] = p[i] & 15;
            m.bpred[2 * i + 1] = p[i] >> 4;
        }
        p += 8;
    }
    m.eob = p;
    p += 25;
    for (int b = 0; b < 25; b++) {
        m.lv[b] = p;
        p += 2 * m.eob[b];
    }
    return p;
}
inline int lv_at(const uint8_t* lv, int n) { return (int)(int16_t)(uint16_t)(lv[2 * n] | (lv[2 * n + 1] << 8)); }

// LevelCosts::calculate (cost.rs:1500)
inline void level_costs(ZwLevelCosts& L, const uint8_t probs[4][8][3][11])
{
    for (int t = 0; t < 4; t++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 3; c++) {
                const uint8_t* p = probs[t][b][c];
                uint16_t cost0 = c > 0 ? bitcost(1, p[0]) : 0;
                uint16_t base = (uint16_t)(bitcost(1, p[1]) + cost0);
                L.lc[t][b][c][0] = (uint16_t)(bitcost(0, p[1]) + cost0);
                for (int v = 1; v <= 67; v++) {
                    int idx = (v < 67 ? v : 67) - 1;
                    int pat = VP8_LEVEL_CODES[idx][0], bits = VP8_LEVEL_CODES[idx][1];
                    uint16_t vc = 0;
                    for (int i = 2; pat; i++) {
                        if (pat & 1) vc = (uint16_t)(vc + bitcost(bits & 1, p[i]));
                        bits >>= 1;
                        pat >>= 1;
                    }
                    L.lc[t][b][c][v] = (uint16_t)(base + vc);
                }
                L.eob[t][b][c] = bitcost(0, p[0]);
                L.init[t][b][c] = bitcost(1, p[0]);
            }
}

struct Stats {
    uint32_t s[4][8][3][11];
};

inline void rec_stat(uint32_t& s, int bit)
{
    if (s >= 0xfffe0000u) s = ((s + 1) >> 1) & 0x7fff7fffu;
    s += 0x00010000u + (bit ? 1u : 0u);
}

inline int token_of(int a)  // |level| -> token (0..10)
{
    return a <= 4 ? a : (a <= 6 ? 5 : a <= 10 ? 6 : a <= 18 ? 7 : a <= 34 ? 8 : a <= 66 ? 9 : 10);
}

// record_coeffs (cost.rs:1297) over a packed block: eob = last nonzero + 1,
// lv = its zigzag levels.  (The branchy form measured faster than walking the
// token paths: most tokens are 0 / 1 and predict well.)  Quirk
// (cost.rs:1325-1342): skip_eob is never cleared once a zero token was seen.
inline void record_coeffs(Stats& S, const uint8_t* lv, int eob, int t, int first, int ctx)
{
    if (eob <= first) {
        rec_stat(S.s[t][VP8_ENC_BANDS[first]][ctx][0], 0);
        return;
    }
    int n = first, skip_eob = 0;
    while (n < eob) {
        uint32_t* st = S.s[t][VP8_ENC_BANDS[n]][ctx];
        const int c = lv_at(lv, n);
        int v = c < 0 ? -c : c;
        n++;
        if (!skip_eob) rec_stat(st[0], 1);
        if (v == 0) {
            rec_stat(st[1], 0);
            skip_eob = 1;
            ctx = 0;
            continue;
        }
        rec_stat(st[1], 1);
        if (v == 1) {
            rec_stat(st[2], 0);
            ctx = 1;
        } else {
            rec_stat(st[2], 1);
            if (v > 67) v = 67;
            if (v <= 4) {
                rec_stat(st[3], 0);
                if (v == 2) rec_stat(st[4], 0);
                else {
                    rec_stat(st[4], 1);
                    rec_stat(st[5], v == 4);
                }
            } else if (v <= 10) {
                rec_stat(st[3], 1);
                rec_stat(st[6], 0);
                rec_stat(st[7], v > 6);
            } else {
                rec_stat(st[3], 1);
                rec_stat(st[6], 1);
                if (v < 3 + (8 << 2)) {
                    rec_stat(st[8], 0);
                    rec_stat(st[9], v >= 3 + (8 << 1));
                } else {
                    rec_stat(st[8], 1);
                    rec_stat(st[10], v >= 3 + (8 << 3));
                }
            }
            ctx = 2;
        }
    }
    if (n < 16) rec_stat(S.s[t][VP8_ENC_BANDS[n]][ctx][0], 0);
}

struct Cplx {
    uint8_t y2, y[4], u[2], v[2];
    void clear(bool with_y2)
    {
        memset(y, 0, 4);
        memset(u, 0, 2);
        memset(v, 0, 2);
        if (with_y2) y2 = 0;
    }
};

// check_all_coeffs_zero on pass-1 (simple-quant) levels: a block has a
// nonzero at index >= first exactly when its eob > first.
inline bool mb_all_zero_p1(const PackedMb& m)
{
    const bool i4 = m.luma == 4;
    if (!i4 && m.eob[16] > 0) return false;
    const int first = i4 ? 0 : 1;
    for (int b = 0; b < 16; b++)
        if (m.eob[b] > first) return false;
    for (int b = 17; b < 25; b++)
        if (m.eob[b] > 0) return false;
    return true;
}

// Skip probability from the MB counts (vp8.rs:1387-1394).
inline int skip_prob(uint32_t total, uint32_t ns)
{
    uint32_t p = (255 * ns + total / 2) / total;
    if (p > 255) p = 255;
    int sp = (int)(uint8_t)p;
    return sp < 1 ? 1 : (sp > 254 ? 254 : sp);
}

// Pass-1 statistics replay in raster order (vp8.rs:1337-1385 + record_residual_stats :1027).
// Returns the skip probability.
inline int replay_stats(Stats& S, const uint8_t* packed, int mbw, int mbh)
{
    PackedMb m;
    memset(&S, 0, sizeof S);
    std::vector<Cplx> top(mbw);
    memset(top.data(), 0, sizeof(Cplx) * mbw);
    uint32_t total = 0, skipped = 0;
    for (int y = 0; y < mbh; y++) {
        Cplx left;
        memset(&left, 0, sizeof left);
        for (int x = 0; x < mbw; x++) {
            packed = view_mb(packed, m);
            total++;
            const bool i4 = m.luma == 4;
            if (mb_all_zero_p1(m)) {
                skipped++;
                left.clear(!i4);
                top[x].clear(!i4);
                continue;
            }
            if (!i4) {
                int cx = left.y2 + top[x].y2;
                record_coeffs(S, m.lv[16], m.eob[16], 1, 0, cx < 2 ? cx : 2);
                left.y2 = top[x].y2 = m.eob[16] > 0;
            }
            const int tt = i4 ? 3 : 0, first = i4 ? 0 : 1;
            for (int by = 0; by < 4; by++) {
                int l = left.y[by];
                for (int bx = 0; bx < 4; bx++) {
                    int cx = l + top[x].y[bx];
                    const int b = by * 4 + bx;
                    record_coeffs(S, m.lv[b], m.eob[b], tt, first, cx < 2 ? cx : 2);
                    l = m.eob[b] > first;
                    top[x].y[bx] = (uint8_t)l;
                }
                left.y[by] = (uint8_t)l;
            }
            for (int pl = 0; pl < 2; pl++) {
                uint8_t* lc = pl ? left.v : left.u;
                uint8_t* tc = pl ? top[x].v : top[x].u;
                for (int by = 0; by < 2; by++) {
                    int l = lc[by];
                    for (int bx = 0; bx < 2; bx++) {
                        int cx = l + tc[bx];
                        const int b = 17 + 4 * pl + by * 2 + bx;
                        record_coeffs(S, m.lv[b], m.eob[b], 2, 0, cx < 2 ? cx : 2);
                        l = m.eob[b] > 0;
                        tc[bx] = (uint8_t)l;
                    }
                    lc[by] = (uint8_t)l;
                }
            }
        }
    }
    return skip_prob(total, total - skipped);
}

// compute_updated_probabilities (vp8.rs:1202); returns whether any update applies.
inline bool updated_probs(const Stats& S, uint8_t out[4][8][3][11])
{
    memcpy(out, COEFF_PROBS, sizeof(COEFF_PROBS));
    int32_t total = 0;
    uint32_t nup = 0;
    for (int t = 0; t < 4; t++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 3; c++)
                for (int p = 0; p < 11; p++) {
                    uint32_t st = S.s[t][b][c][p];
                    int nb = (int)(st & 0xffff), tot = (int)(st >> 16);
                    if (tot == 0) continue;
                    uint8_t oldp = COEFF_PROBS[t][b][c][p], upp = COEFF_UPDATE_PROBS[t][b][c][p];
                    uint8_t newp = (uint8_t)(255 - (uint32_t)nb * 255 / (uint32_t)tot);
                    int oc = nb * VP8_ENTROPY_COST[255 - oldp] + (tot - nb) * VP8_ENTROPY_COST[oldp] + bitcost(0, upp);
                    int nc = nb * VP8_ENTROPY_COST[255 - newp] + (tot - nb) * VP8_ENTROPY_COST[newp] + bitcost(1, upp) + 8 * 256;
                    int sav = oc - nc;
                    if (sav > 0) {
                        out[t][b][c][p] = newp;
                        total += sav;
                        nup++;
                    }
                }
    if (!(total > 0 && nup > 0)) {
        memcpy(out, COEFF_PROBS, sizeof(COEFF_PROBS));
        return false;
    }
    return true;
}

// Compressed frame header (encode_compressed_frame_header vp8.rs:332-372) with
// log2(nparts) token partitions; `probs` leaves with the probabilities in force.
// Enc takes the decisions (put / flag / literal / path): the product's recorder
// (DecRec, zw_host_emit.h) or a coder (tools/emit_ref.h).
template <class Enc>
inline void emit_frame_header(Enc& H, const ZwFrameParams& P, bool have_updated,
                              const uint8_t upd[4][8][3][11], int nparts, uint8_t probs[4][8][3][11])
{
    memcpy(probs, COEFF_PROBS, sizeof(COEFF_PROBS));
    H.literal(1, 0);
    H.literal(1, 0);
    H.flag(P.seg_enabled);
    if (P.seg_enabled) {
        H.flag(P.seg_update_map);
        H.flag(1);
        H.flag(0);
        for (int s = 0; s < 4; s++) {
            int ql = P.seg[s].quantizer_level;
            H.flag(ql != 0);
            if (ql != 0) {
                H.literal(7, ql < 0 ? -ql : ql);
                H.flag(ql < 0);
            }
        }
        for (int s = 0; s < 4; s++) H.flag(0);
        if (P.seg_update_map)
            for (int i = 0; i < 3; i++) {
                H.flag(P.seg_probs[i] != 255);
                if (P.seg_probs[i] != 255) H.literal(8, P.seg_probs[i]);
            }
    }
    H.flag(0);
    H.literal(6, P.filter_level);
    H.literal(3, 0);
    H.flag(0);
    H.literal(2, nparts == 8 ? 3 : nparts >> 1);  // vp8.rs:352-354
    H.literal(7, P.base_qi);
    for (int i = 0; i < 5; i++) H.flag(0);
    H.literal(1, 0);
    for (int t = 0; t < 4; t++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 3; c++)
                for (int p = 0; p < 11; p++) {
                    uint8_t oldp = probs[t][b][c][p];
                    if (have_updated && upd[t][b][c][p] != oldp) {
                        H.put(1, COEFF_UPDATE_PROBS[t][b][c][p]);
                        H.literal(8, upd[t][b][c][p]);
                        probs[t][b][c][p] = upd[t][b][c][p];
                    } else {
                        H.put(0, COEFF_UPDATE_PROBS[t][b][c][p]);
                    }
                }
    H.literal(1, 1);
    H.literal(8, P.skip_prob);
}

// write_macroblock_header (vp8.rs:498-560) of MB x of the current row.
template <class Enc>
inline void emit_mb_header(Enc& H, const ZwFrameParams& P, const PackedMb& m, uint8_t* top_bp, uint8_t left_bp[4], int x)
{
    static const TreePaths seg_t(SEGMENT_ID_TREE, 6, 4), ymode_t(YMODE_TREE, 8, 5), bmode_t(BMODE_TREE, 18, 10),
        uvmode_t(UVMODE_TREE, 6, 4);
    if (P.seg_enabled && P.seg_update_map) seg_t.put(H, P.seg_probs, m.segment);
    H.put(m.skip, P.skip_prob);
    ymode_t.put(H, KEYFRAME_YMODE_PROBS, m.luma);
    if (m.luma == 4) {
        for (int by = 0; by < 4; by++) {
            int l = left_bp[by];
            for (int bx = 0; bx < 4; bx++) {
                int t = top_bp[x * 4 + bx], md = m.bpred[by * 4 + bx];
                bmode_t.put(H, KEYFRAME_BPRED_MODE_PROBS[t][l], md);
                l = md;
                top_bp[x * 4 + bx] = (uint8_t)md;
            }
            left_bp[by] = (uint8_t)l;
        }
    } else {
        static const int intra_of[4] = {0, 2, 3, 1};
        for (int i = 0; i < 4; i++) left_bp[i] = top_bp[x * 4 + i] = (uint8_t)intra_of[m.luma];
    }
    uvmode_t.put(H, KEYFRAME_UV_MODE_PROBS, m.chroma);
}

// quality_to_quant_index (vp8.rs:37-55) with fast_math::cbrt/round (fast_math.rs:15-42).
inline int quality_to_qi(int quality)
{
    double c = (double)quality / 100.0;
    double lin = c < 0.75 ? c * (2.0 / 3.0) : 2.0 * c - 1.0;
    double y = 0.0;
    if (lin != 0.0) {
        uint64_t bits;
        memcpy(&bits, &lin, 8);
        uint64_t ab = bits / 3 + (uint64_t)(1023ull * 2 / 3) * (1ull << 52);
        memcpy(&y, &ab, 8);
        for (int i = 0; i < 4; i++) {
            double y2 = y * y;
            y = (2.0 * y + lin / y2) / 3.0;
        }
    }
    double r = (double)(int64_t)(127.0 * (1.0 - y) + 0.5);
    int q = (int)r;
    return q < 0 ? 0 : (q > 127 ? 127 : q);
}

// compute_filter_level (cost.rs:271) with sharpness 0, strength 50.
inline int filter_level_for(int qi)
{
    uint32_t level0 = 250;
    int qstep = (uint8_t)(VP8_AC_TABLE[qi] >> 2);
    uint32_t base = LEVELS_FROM_DELTA[0][qstep < 63 ? qstep : 63];
    uint32_t f = base * level0 / 256;
    if (f < 2) return 0;
    return f > 63 ? 63 : (int)f;
}

}  // namespace zwh
