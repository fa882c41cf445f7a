// zw_enc_pairfinal.h -- which (block, start context) trellis runs the final
// I16 luma transform of a macroblock needs, and how the runs of the two MBs of
// a frame pair are numbered onto the lanes of one wave.
//
// Plain integers only (no HIP types): final_luma_pair in zw_enc_kernels.hip
// reads it on the device, tools/pair_final_check.cpp walks it on the host.  A
// wrong mask makes a block gather its levels from a lane that ran another
// block (or from a lane past the wave), so the tool checks every pattern where
// nothing can go out of range.
//
// A Y1 block's start context is the number of its left and top neighbours
// with nonzero levels (capped at 2), and a neighbour inside the MB is known
// only after its own trellis.  So a block is run under every context its
// still-unknown neighbours leave possible, the raster-order chain is resolved
// afterwards, and every block takes the levels of its resolved context.
//   * A block is TRIVIALLY ZERO when the trellis can only return zeros
//     whatever the context (pf_trivial): it needs no run and its flag is 0.
//   * A neighbour's flag is KNOWN if it lies in the MB above / to the left
//     (the edge flags, final before this MB starts), or is a trivially zero
//     block of this MB (0); otherwise it is UNKNOWN.
//   * A block that is not trivially zero NEEDS the contexts min(k + t, 2),
//     t = 0 .. u, with k its known-one neighbours and u its unknown ones.
// A needed (block, context) is one task; an MB has at most 40 (block 0 needs
// one context, the six other edge blocks two, the nine interior blocks three).
#pragma once
#include <stdint.h>

#ifndef ZW_HD
#ifdef __HIPCC__
#define ZW_HD __host__ __device__
#else
#define ZW_HD
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define ZW_PF_UMUL(a, b) __umul24((a), (b))
#define ZW_PF_POPC(v) __popcll(v)
#else
#define ZW_PF_UMUL(a, b) ((uint32_t)(a) * (uint32_t)(b))
#define ZW_PF_POPC(v) __builtin_popcountll(v)
#endif

#define ZW_PF_MAX_TASKS 40  // per MB
#define ZW_PF_LANES 64      // tasks of one trellis call

// Zigzag position n -> natural index (VP8 ZIGZAG), 4 bits each.
ZW_HD inline int pf_zz(int n) { return (int)((0xfeb7adc963258410ull >> (4 * n)) & 15); }

// Trivially zero: with `last` as the trellis computes it (the highest zigzag
// position 1..15 whose coefficient has c * c > q_ac * q_ac / 4, plus one,
// capped at 15), every position 1 .. last has a threshold level of 0: the
// level of |c| + sharpen[j] under the rounding bias 0x80.  Then only level 0
// is admissible at every position, no terminating node is ever recorded and
// the result is all zero under every start context.  c: the block's 16
// coefficients in natural order (c[0], the DC, goes through Y2 and is not
// read); q_ac / iq_ac / sharpen: the segment's Y1 matrix.
ZW_HD inline bool pf_trivial(const int* c, uint32_t q_ac, uint32_t iq_ac, const uint16_t* sharpen)
{
    const uint32_t thresh = ZW_PF_UMUL(q_ac, q_ac) / 4u;
    const uint32_t tbias = ((0x80u << 17) + 128u) >> 8;
    int last = 0;
    uint32_t live = 0;  // bit n: position n has a threshold level above 0
    for (int n = 1; n < 16; n++) {
        const int j = pf_zz(n);
        const uint32_t a = (uint32_t)(c[j] < 0 ? -c[j] : c[j]);
        if (ZW_PF_UMUL(a, a) > thresh) last = n;
        const uint32_t thr = (ZW_PF_UMUL(a + sharpen[j], iq_ac) + tbias) >> 17;
        live |= (uint32_t)(thr != 0u) << n;
    }
    if (last < 15) last++;
    return (live & ((2u << last) - 1u)) == 0u;
}

// The MB's edge flags in one byte: bit x (0..3) the flag of the block above
// column x, bit 4 + y the flag of the block left of row y.
ZW_HD inline unsigned pf_edge(const int* top4, const int* left4)
{
    unsigned e = 0;
    for (int q = 0; q < 4; q++) e |= ((unsigned)(top4[q] != 0) << q) | ((unsigned)(left4[q] != 0) << (4 + q));
    return e;
}

// The contexts block b (raster 0..15) needs, bit cx; triv: bit b' set for the
// MB's trivially zero blocks.  Branch-free: k + u <= 2, so the needed
// contexts are the run k .. k + u.
ZW_HD inline unsigned pf_need(int b, unsigned triv, unsigned edge)
{
    const int bx = b & 3, by = b >> 2;
    const unsigned lt = (triv >> ((b - 1) & 15)) & 1u, tt = (triv >> ((b - 4) & 15)) & 1u;
    const unsigned kl = bx == 0 ? (edge >> (4 + by)) & 1u : 0u, ul = bx == 0 ? 0u : lt ^ 1u;
    const unsigned kt = by == 0 ? (edge >> bx) & 1u : 0u, ut = by == 0 ? 0u : tt ^ 1u;
    const unsigned k = kl + kt, u = ul + ut;
    const unsigned run = (1u << (k + u + 1u)) - (1u << k);
    return ((triv >> b) & 1u) ? 0u : run;
}

// An MB's tasks as a 48-bit mask, bit cx * 16 + b.
ZW_HD inline uint64_t pf_mask(unsigned triv, unsigned edge)
{
    uint64_t m = 0;
    for (int b = 0; b < 16; b++) {
        const unsigned nd = pf_need(b, triv, edge);
        for (int cx = 0; cx < 3; cx++) m |= (uint64_t)((nd >> cx) & 1u) << (cx * 16 + b);
    }
    return m;
}

ZW_HD inline int pf_count(uint64_t mask) { return (int)ZW_PF_POPC(mask); }

// Task numbering: a prefix count over the MB's mask, after the `base` tasks
// of the MB before it (0 for the first MB of a call, its count for the second).
ZW_HD inline int pf_task(uint64_t mask, int base, int b, int cx)
{
    return base + (int)ZW_PF_POPC(mask & ((1ull << (cx * 16 + b)) - 1ull));
}

// Both MBs' tasks fit one trellis call of the wave.  (ZW_PF_COMPACT=0, for
// A/B builds: never, the paired stage keeps one call per frame.)
#ifndef ZW_PF_COMPACT
#define ZW_PF_COMPACT 1
#endif
ZW_HD inline bool pf_one_call(uint64_t mask_a, uint64_t mask_b)
{
    return ZW_PF_COMPACT && pf_count(mask_a) + pf_count(mask_b) <= ZW_PF_LANES;
}

// The fallback's mask (one call per MB, every block under every context, as
// the per-frame final transform runs it): task cx * 16 + b.
#define ZW_PF_ALL 0xffffffffffffull
