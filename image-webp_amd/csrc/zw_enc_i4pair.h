// zw_enc_i4pair.h -- the lane maps and the lane-form state of the paired I4
// search (i4p_step / pick_i4_pair in zw_enc_kernels.hip).
//
// Plain integers only (no HIP types): the kernels read it on the device,
// tools/i4_pair_check.cpp walks it on the host.  A wrong map makes a candidate
// lane transform another group's mode (or read a lane of another group), a
// wrong state update gives the next step another context or ends a search at
// another block than the reference does, so the tool checks both against a
// plain per-MB model.
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

#define ZW_I4P_KMAX 4  // candidates per block of the paired form (methods <= 4)

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
