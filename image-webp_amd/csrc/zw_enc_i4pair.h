// zw_enc_i4pair.h -- the lane maps and the lane-form state of the paired I4
// search (i4p_step / pick_i4_pair in zw_enc_kernels.hip).
//
// Plain integers only (no HIP types): the kernels read it on the device,
// tools/i4_pair_check.cpp walks it on the host.  A wrong map makes a candidate
// lane transform another group's mode (or read a lane of another group), a
// wrong state update gives the next step another context or ends a search at
// another block than the reference does, so the tool checks both against a
// plain per-MB model.
// The value vector's lane map, the paired index table's rule, the v_perm
// selectors and the ranking's key are here too; tools/i4_rank_check.cpp walks
// them against the ten predictors written plainly and against the exact SSE.
//
// Lanes of a step: group g = lane >> 4 = 2 hm + slot (hm: the MB of the pair,
// slot: the block of the anti-diagonal); the ranking works mode m = lane & 15
// of its group (m < 10), the candidate phase quad k = (lane >> 2) & 3 of its
// group, lane q = lane & 3 of the quad.  In a one-block step (NB = 1) the
// slot-1 rows repeat their MB's slot-0 rows.
#pragma once
#include <stdint.h>

#ifndef ZW_HD
#ifdef __HIPCC__
#define ZW_HD __host__ __device__
#else
#define ZW_HD
#endif
#endif

// A/B knobs (0: the forms before them, for `make exp` builds).
#ifndef ZW_I4P_INV
#define ZW_I4P_INV 1  // candidate modes by the inverse-rank permute, not by ballots
#endif
#ifndef ZW_I4P_LANES
#define ZW_I4P_LANES 1  // the search's running state in lanes, not in scalars
#endif

#ifndef ZW_I4P_TMV
#define ZW_I4P_TMV 1  // TrueMotion's sixteen predictions are value-vector entries, not per-lane arithmetic
#endif
#ifndef ZW_I4P_DOT4
#define ZW_I4P_DOT4 1  // the ranking's sort key from two byte dot products, not from an exact SSE
#endif

#define ZW_I4P_KMAX 4  // candidates per block of the paired form (methods <= 4)

// ---------------------------------------------------------------------------
// The value vector of a block.  From its thirteen edge pixels
// E = [L3 L2 L1 L0 P A0..A7] (left column bottom-up, corner, above and
// above-right), entry v is (E[ka] + wb E[kb] + wc E[kc] + rnd) >> sh, clamped
// to 0..255:
//   V[0..12]  E[k]                            V[13..23] avg3(E[k], E[k+1], E[k+2])
//   V[24..35] avg2(E[k], E[k+1])              V[36] avg3(A6,A7,A7)  V[37] avg3(L2,L3,L3)
//   V[38]     DC = (4 + L0..L3 + A0..A3) >> 3 (a reduction, not this formula)
//   V[39 + 4r + j] TrueMotion's pixel (r, j): clamp(L[r] + A[j] - P)   (ZW_I4P_TMV)
// Only TrueMotion's entries can leave 0..255 before the clamp.  Lane v of the
// wave forms entry v; the lanes past the vector form a valid entry nobody reads.
// ---------------------------------------------------------------------------
#define ZW_I4P_NV (ZW_I4P_TMV ? 55 : 39)
#define ZW_I4P_V_DC 38
#define ZW_I4P_V_TM 39

// (mode, pixel) -> index into the value vector in the single form's numbering
// (d_I4_IDX, zw_dev.h): 255 = DC, 254 = TrueMotion.
#define ZW_I4_IDX_ROWS \
    {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}, \
    {254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254}, \
    {17, 18, 19, 20, 17, 18, 19, 20, 17, 18, 19, 20, 17, 18, 19, 20}, \
    {15, 15, 15, 15, 14, 14, 14, 14, 13, 13, 13, 13, 37, 37, 37, 37}, \
    {18, 19, 20, 21, 19, 20, 21, 22, 20, 21, 22, 23, 21, 22, 23, 36}, \
    {16, 17, 18, 19, 15, 16, 17, 18, 14, 15, 16, 17, 13, 14, 15, 16}, \
    {28, 29, 30, 31, 16, 17, 18, 19, 15, 28, 29, 30, 14, 16, 17, 18}, \
    {29, 30, 31, 32, 18, 19, 20, 21, 30, 31, 32, 22, 19, 20, 21, 23}, \
    {27, 16, 17, 18, 26, 15, 27, 16, 25, 14, 26, 15, 24, 13, 25, 14}, \
    {26, 14, 25, 13, 25, 13, 24, 37, 24, 37, 0, 0, 0, 0, 0, 0},

struct I4PValue {
    int ka, kb, kc;  // indices into E
    int wb, wc, sh;
};
ZW_HD inline I4PValue i4p_value_map(int l)
{
    // t: 0 copy, 1 avg3, 2 avg2, 3/4 the two special avg3, 5 TrueMotion
    // (arithmetic only: lane-dependent selects must not become branches)
    const int t = (int)(l >= 13) + (int)(l >= 24) + (int)(l >= 36) + (int)(l >= 37);
    const int k0 = l - 13 * (int)(l >= 13) - 11 * (int)(l >= 24), k = k0 < 12 ? k0 : 12;
    const int t3 = (int)(t == 3), t4 = (int)(t >= 4), t12 = (int)(t == 1 || t == 2);
    const int kc0 = k + 2 * (int)(t == 1);
    I4PValue v;
    v.ka = k + t3 * (11 - k) + t4 * (1 - k);
    v.kb = k + t12 + t3 * (12 - k) - t4 * k;
    v.kc = kc0 < 12 ? kc0 : 12;
    v.wb = 2 * (int)(t == 1) + (int)(t == 2) + 3 * (t3 + t4);
    v.wc = (int)(t == 1);
    v.sh = (int)(t != 0) + (int)(t != 0 && t != 2);
#if ZW_I4P_TMV
    const bool t5 = l >= ZW_I4P_V_TM;
    const int i = l - ZW_I4P_V_TM, r = (i >> 2) & 3, j = i & 3;
    v.ka = t5 ? 3 - r : v.ka;
    v.kb = t5 ? 5 + j : v.kb;
    v.kc = t5 ? 4 : v.kc;
    v.wb = t5 ? 1 : v.wb;
    v.wc = t5 ? -1 : v.wc;
    v.sh = t5 ? 0 : v.sh;
#endif
    return v;
}
ZW_HD inline int i4p_value(const I4PValue& v, int ea, int eb, int ec)
{
    const int x = (ea + v.wb * eb + v.wc * ec + ((1 << v.sh) >> 1)) >> v.sh;
#if ZW_I4P_TMV
    return x < 0 ? 0 : (x > 255 ? 255 : x);
#else
    return x;
#endif
}
// The lanes whose E[ka] the DC sums: L3..L0 and A0..A3.
ZW_HD inline bool i4p_value_dc_term(int l) { return l < 4 || (l >= 5 && l < 9); }

// The value-vector entry of pixel p (raster, 0..15) of a mode whose index byte
// in the single form's table (d_I4_IDX) is idx: 254 marks TrueMotion, 255 DC.
ZW_HD inline int i4p_vindex(int idx, int p)
{
    return idx == 254 ? (ZW_I4P_TMV ? ZW_I4P_V_TM + p : 3 - (p >> 2)) : (idx == 255 ? ZW_I4P_V_DC : idx);
}

// ---------------------------------------------------------------------------
// The gathered words.  A ds_bpermute of the value vector hands a lane the word
// of one entry: the entry's byte of each of the four (MB, slot) groups, group
// g = 2 hm + slot in byte g.  v_perm(a, b, sel) builds each result byte from
// selector byte n: byte n of b (n < 4), byte n - 4 of a (n < 8), zero (0x0c).
// ---------------------------------------------------------------------------
// Two words (v0, v1) to the lane's group's bytes as 16-bit values:
// v_perm(v1, v0, psel) = v0[g] | v1[g] << 16 (the candidate phase's pairs).
ZW_HD inline uint32_t i4p_psel(int hm, int slot)
{
    const uint32_t b = (uint32_t)(2 * hm + slot);
    return 0x0c000c00u | ((4u + b) << 16) | b;
}
// ... and as bytes: v_perm(v1, v0, bsel) = v0[g] | v1[g] << 8 (the ranking's rows).
ZW_HD inline uint32_t i4p_bsel(int hm, int slot)
{
    const uint32_t b = (uint32_t)(2 * hm + slot);
    return 0x0c0c0000u | ((4u + b) << 8) | b;
}
// A row's four predictions in the source row's byte order (x0 in byte 0), from
// b01 = v_perm(v1, v0, bsel) and b23 = v_perm(v3, v2, bsel).
ZW_HD inline uint32_t i4p_pack_row(uint32_t b01, uint32_t b23) { return (b23 << 16) | b01; }
// The same row from the 16-bit pairs p01 = (x0, x1) and p32 = (x3, x2):
// v_perm(p32, p01, ZW_I4P_PAIRS_TO_ROW).
#define ZW_I4P_PAIRS_TO_ROW 0x04060200u

// ---------------------------------------------------------------------------
// The ranking's sort key of mode m.  The exact key is sse << 4 | m with
// sse = sum (s - p)^2 = ss - 2 sp + pp over the block's sixteen pixels, and ss
// is the same for the ten modes of a block, so pp - 2 sp orders them alike,
// ties included (the mode stays in the low bits).  With bytes,
// pp, sp <= 16 * 255^2 = 1 040 400 < 2^20, so 2^22 + pp - 2 sp lies in
// (2^22 - 2^21, 2^22 + 2^20]: positive and below 2^23, and the key below 2^27.
// ---------------------------------------------------------------------------
#define ZW_I4P_KEY_BIAS (1u << 22)
ZW_HD inline uint32_t i4p_rank_key(uint32_t pp, uint32_t sp, int m)
{
    return ((ZW_I4P_KEY_BIAS + pp - 2u * sp) << 4) | (uint32_t)m;
}

// ---------------------------------------------------------------------------
// Candidate modes.  The ranks of a group's ten modes are a permutation of
// 0..9 (the keys sse << 4 | m are distinct), lanes m >= 10 all have rank 10.
// Lane (g, m) sends m forward to the first lane of quad `rank` of its group;
// every lane of quad k then takes the value of its quad's first lane.  Ranks
// of 4 and more go to lane 1 of the group, which no lane reads.
// ---------------------------------------------------------------------------
ZW_HD inline int i4p_inv_dest(int lane, int rank)
{
    return (lane & ~15) + (rank < ZW_I4P_KMAX ? 4 * rank : 1);
}
// The lane whose received value lane `lane` takes (a quad broadcast of lane 0).
ZW_HD inline int i4p_mode_src(int lane) { return lane & ~3; }
// Lanes of quads k >= K keep a valid mode (0) and are never eligible.
ZW_HD inline bool i4p_eligible(int lane, int K) { return ((lane >> 2) & 3) < K; }
ZW_HD inline int i4p_mode(int lane, int K, int received) { return i4p_eligible(lane, K) ? received : 0; }

// ---------------------------------------------------------------------------
// The winner of a group, as two words every lane of the winning quad holds
// alike: its u16 rate, mode cost (< 2^15) and nonzero flag, and its SSE
// (<= 16 * 255^2 < 2^24) and mode.  Every other lane of the group contributes
// 0; an OR over the group's four quads (two row rotations) leaves the words in
// every lane of the group, a swap of the 16-lane rows gives every lane of an MB
// both slots' words.
// ---------------------------------------------------------------------------
struct I4PWin {
    uint32_t pk;  // rate & 0xffff | mode cost << 16 | nonzero << 31
    uint32_t sm;  // sse | mode << 24
};
ZW_HD inline I4PWin i4p_win(uint32_t rate, uint32_t mcost, bool nz, uint32_t sse, int mode)
{
    I4PWin w;
    w.pk = (rate & 0xffffu) | (mcost << 16) | ((uint32_t)nz << 31);
    w.sm = sse | ((uint32_t)mode << 24);
    return w;
}

// ---------------------------------------------------------------------------
// The running state of one MB's search (I4State of the single form), held
// alike by every lane of the MB.  The contexts of block (bx, by) are the mode
// and the nonzero flag of the blocks above and to its left: when the
// anti-diagonal of (bx, by) is worked, the last block chosen in column bx is
// (bx, by - 1) and the last chosen in row by is (bx - 1, by), so one nibble
// per column and one per row hold every mode a later step asks for.
// ---------------------------------------------------------------------------
struct I4PState {
    uint64_t running;   // sum of the chosen blocks' rd scores (+ 211 * lambda_mode)
    uint32_t total_mc;  // header-bit cap accumulator
    uint32_t nzt;       // bits 0..15: nonzero flags by raster index; bits 16..31: last mode of column x, 4 bits each
    uint32_t lm;        // last mode of row y, 4 bits each
};

ZW_HD inline void i4p_state_init(I4PState& s, uint32_t l_mode)
{
    s.running = 211ull * l_mode;
    s.total_mc = 0;
    s.nzt = 0;
    s.lm = 0;
}

// Block (bx, by)'s winner joins its MB's state.
ZW_HD inline void i4p_state_update(I4PState& s, int bx, int by, I4PWin w, uint32_t l_mode)
{
    const uint32_t mode = w.sm >> 24, sse = w.sm & 0xffffffu;
    s.nzt |= (w.pk >> 31) << (by * 4 + bx);
    s.nzt = (s.nzt & ~(0xf0000u << (4 * bx))) | (mode << (16 + 4 * bx));
    s.lm = (s.lm & ~(0xfu << (4 * by))) | (mode << (4 * by));
    s.total_mc += (w.pk >> 16) & 0x7fffu;
    s.running += (uint64_t)sse * 256ull + (uint64_t)(w.pk & 0xffffu) * l_mode;
}

// Contexts of block (bx, by): the modes above and to the left (0 at the MB's
// border) and the count of their nonzero flags.
ZW_HD inline int i4p_tctx(const I4PState& s, int bx, int by)
{
    return by == 0 ? 0 : (int)((s.nzt >> (16 + 4 * bx)) & 15u);
}
ZW_HD inline int i4p_lctx(const I4PState& s, int bx, int by)
{
    return bx == 0 ? 0 : (int)((s.lm >> (4 * by)) & 15u);
}
ZW_HD inline int i4p_nzctx(const I4PState& s, int bx, int by)
{
    const int i = by * 4 + bx;
    return (by == 0 ? 0 : (int)((s.nzt >> ((i - 4) & 15)) & 1u)) + (bx == 0 ? 0 : (int)((s.nzt >> ((i - 1) & 15)) & 1u));
}

// The search's two early exits (vp8.rs:2018, :1839), over the blocks chosen so far.
ZW_HD inline bool i4p_exit(const I4PState& s, uint64_t i16_score)
{
    return s.running >= i16_score || s.total_mc > 256u * 16u * 16u / 4u;
}
