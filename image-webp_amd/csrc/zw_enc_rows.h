// zw_enc_rows.h -- which wave of an encode workgroup works which MB row.
//
// Plain integers only (no HIP types): the kernels in zw_enc_kernels.hip read
// it on the device, tools/enc_rows_check.cpp walks it on the host.  A wave
// waits on the wave that owns the row above, so a schedule that gives a row to
// no wave, to two, or to a chain wave is a hang on the device; the tool checks
// the shipped shapes where nothing can hang.
#pragma once

#ifndef ZW_HD
#ifdef __HIPCC__
#define ZW_HD __host__ __device__
#else
#define ZW_HD
#endif
#endif

// Row k of each round of luma rows goes to wave luma_wave(k).  In pass 1 the
// luma waves that share SIMD 0 with the chroma chain (issue priority 3)
// run slowest, and every later row of a round waits on a slow row: they
// take the last rows of each round, which only the next round's first
// row follows, with a round of slack.
#ifndef ZW_P1_ORDER
#define ZW_P1_ORDER 1
#endif
// ZW_P1_SLOWSKIP (pass 1, batch shape): the luma waves on SIMD 0 (beside
// the chain) take fewer rows.  Rows go out in rounds: the nfast rows of the
// other SIMDs' waves, then the round's share of SIMD-0 rows (the SIMD-0
// waves in turn), ZW_P1_SLOW_NUM SIMD-0 rows per ZW_P1_SLOW_DEN rounds.  So
// SIMD 0 carries the chain plus fewer luma rows, and its rows keep pace
// with the rest instead of throttling every row behind them.
#ifndef ZW_P1_SLOWSKIP
#define ZW_P1_SLOWSKIP 1
#endif
#ifndef ZW_P1_SLOW_NUM
#define ZW_P1_SLOW_NUM 1  // re-tuned in round 4 (1080p, 256 frames, one lane): 1/1 28.2-28.3 ms, 3/2 28.8-29.0,
#endif                    // 2/3 29.0-29.1, 1/2 29.2, 4/3 29.8, 0/1 29.9, 2/1 31.7
#ifndef ZW_P1_SLOW_DEN
#define ZW_P1_SLOW_DEN 1
#endif

// The rows of a frame over the NW waves of its workgroup, of which waves
// 0..NCH-1 are pass 1's chroma chain (NCH 0 in pass 2) and take no row.
// PAIR (the frame-pair kernels) and pass 2 deal the rows to the luma waves in
// turn; pass 1 orders them as above.  The row-parallel kernels (ROWS) draw
// their rows from a ticket instead and only share the type.  (Pass 1 in frame
// pairs has a schedule of its own, PairRowSchedule1 below; PAIR serves pass 2.)
template <int PASS, bool ROWS, int NW, int NCH, bool PAIR = false> struct RowSchedule {
    static_assert(PASS == 1 || NCH == 0, "chain waves are pass 1's");
    static constexpr bool plain = PASS == 2 || PAIR;
    static constexpr int nrw = NW - NCH;  // waves on the luma wavefront
    static constexpr bool skip_mode = ZW_P1_SLOWSKIP && PASS == 1 && !ROWS && !PAIR && NCH == 1 && NW > 4;
    static constexpr int nslow = (NW - 1) / 4 > 0 ? (NW - 1) / 4 : 1;  // luma waves on SIMD 0: 4, 8, ..
    static constexpr int nfast = NW - NCH - (NW - 1) / 4;             // luma waves on SIMDs 1..3

    // wave v takes its row of a round before wave w
    static ZW_HD bool p1_before(int v, int w)
    {
        const bool sv = (v & 3) < NCH, sw = (w & 3) < NCH;
        return (ZW_P1_ORDER && sv != sw) ? sw : v < w;
    }
    static ZW_HD int luma_rank(int w)
    {
        if (plain) return w - NCH;
        int r = 0;
        for (int v = NCH; v < NW; v++) r += (int)p1_before(v, w);
        return r;
    }
    static ZW_HD int luma_wave(int k)
    {
        if (plain) return k + NCH;
        int w = NCH;
        for (int v = NCH; v < NW; v++)
            if (luma_rank(v) == k) w = v;
        return w;
    }
    static ZW_HD int fast_wave(int i) { return i + 1 + i / 3; }
    static ZW_HD int wave_of_row(int y)
    {
        if (!skip_mode) return luma_wave(y % (nrw > 0 ? nrw : 1));
        constexpr int L = ZW_P1_SLOW_DEN * nfast + ZW_P1_SLOW_NUM;
        int r = y % L, before = (y / L) * ZW_P1_SLOW_NUM;
        for (int k = 0; k < ZW_P1_SLOW_DEN; k++) {
            const int sk = ((k + 1) * ZW_P1_SLOW_NUM) / ZW_P1_SLOW_DEN - (k * ZW_P1_SLOW_NUM) / ZW_P1_SLOW_DEN;
            if (r < nfast) return fast_wave(r);
            r -= nfast;
            if (r < sk) return 4 * (1 + (before + r) % nslow);
            r -= sk;
            before += sk;
        }
        return 0;  // unreachable
    }
    static ZW_HD int wave_of_row(int y, int /*mbh*/) { return wave_of_row(y); }  // (as PairRowSchedule1 takes it)
    // the wave's next row after `y` (mbh or more: none)
    static ZW_HD int next_row(int wave, int y, int mbh)
    {
        if (!skip_mode) return y + nrw;
        for (y++; y < mbh; y++)
            if (wave_of_row(y) == wave) break;
        return y;
    }
    static ZW_HD int first_row(int wave, int mbh) { return skip_mode ? next_row(wave, -1, mbh) : luma_rank(wave); }
};

// ---------------------------------------------------------------------------
// Pass 1 in frame pairs (k_encode_pass1_fp): NW waves, of which waves
// 0..NCH-1 first run the chroma chains (one per frame) and then take rows too.
//
// While the chains run, the luma waves beside them (the slow waves, (w & 3) <
// NCH: 4, 5, 8, 9 of 12) lose issue slots to a chain at higher priority.  Up to
// the join row J(mbh) the rows go out in rounds as in skip mode above: the fast
// waves' rows, then the round's share of slow-wave rows (the slow waves in
// turn), ZW_P1P_SLOW_NUM slow rows per ZW_P1P_SLOW_DEN rounds.
//
// From row J on the chains are done (they end at about half of the kernel), no
// wave is slow and the chain waves are free: the rows go round all NW waves.
// The order of that round is the order in which the waves come free: the waves
// without a row above J first (the chain waves), then the others by their last
// row above J, oldest first -- a wave handed row J while it still works row
// J - 1 would hold up every row below.  A chain wave's progress word stays -1
// until it publishes, so should a chain run late, the row below just waits
// (and so does every row behind it: J too early costs more than J too late).
// J is ZW_P1P_JOIN_NUM / _DEN of the frame's rows; frames of fewer than
// ZW_P1P_JOIN_MIN rows have no join (J = mbh: the chain waves take no row).
//
// Static, so tools/enc_pair_rows_check.cpp can walk it: rows strictly
// increasing per wave and one owner per row, with row y waiting only on row
// y - 1 and the chains on nothing, is what keeps the kernel from hanging.
//
// Measured on MI355X, pass 1 of 512 1080p frames (68 rows) in one pair launch,
// ms, two runs each; plain round-robin over waves 2..11 without a join (what
// the kernel ran before): 46.62-46.80.
// ---------------------------------------------------------------------------
// The slow waves' rows per round of six fast rows.  Unlike in the one-frame
// kernel a smaller share does not pay: the chains end halfway, and the slow
// waves are slow only until then.  With the join at 5/8: 4/1 (every luma wave
// one row a round) 45.28-45.44, 2/1 46.13-46.26, 3/2 48.52, 5/1 50.4, 6/1 50.3;
// with the join at 1/2: 4/1 47.75-47.84, 3/2 47.55-47.63, 2/1 47.86-48.06,
// 1/1 48.55-48.65, 3/1 48.71-48.75.
#ifndef ZW_P1P_SLOW_NUM
#define ZW_P1P_SLOW_NUM 4
#endif
#ifndef ZW_P1P_SLOW_DEN
#define ZW_P1P_SLOW_DEN 1
#endif
// The join row as a fraction of the frame's rows.  At share 4/1: 9/16 46.01,
// 5/8 45.28-45.44, 11/16 46.05-46.14, 3/4 45.78-45.89; at share 2/1: 3/8
// 51.89-52.17 (the chains are not done: every row below waits), 1/2
// 47.86-48.06, 9/16 46.67-46.81, 5/8 46.13-46.26, 11/16 46.73-46.74, 3/4
// 47.01-47.06, no join 51.99-52.11.  (The chain waves last in the first round
// after J instead of first, J at 1/2: 45.31-45.61, the same as 5/8 with them
// first; at 5/8 45.66-45.68.  The rows above J in plain wave order 2..11
// instead of fast waves first: 45.97-46.00.)
#ifndef ZW_P1P_JOIN_NUM
#define ZW_P1P_JOIN_NUM 5
#endif
#ifndef ZW_P1P_JOIN_DEN
#define ZW_P1P_JOIN_DEN 8
#endif
// Frames of fewer rows have no join.
#ifndef ZW_P1P_JOIN_MIN
#define ZW_P1P_JOIN_MIN 24
#endif

template <int NW, int NCH> struct PairRowSchedule1 {
    static_assert(NW % 4 == 0 && NW > 4 && NW <= 16 && NCH >= 1 && NCH < 4, "chain waves on some of the four SIMDs");
    static_assert(ZW_P1P_SLOW_NUM >= 0 && ZW_P1P_SLOW_DEN >= 1, "the slow-row share");
    static_assert(ZW_P1P_JOIN_NUM >= 0 && ZW_P1P_JOIN_NUM <= ZW_P1P_JOIN_DEN && ZW_P1P_JOIN_DEN >= 1, "the join fraction");
    static constexpr int nslow = (NW / 4 - 1) * NCH;  // luma waves on a chain wave's SIMD
    static constexpr int nfast = NW - NCH - nslow;    // luma waves on the other SIMDs
    static constexpr int L = ZW_P1P_SLOW_DEN * nfast + ZW_P1P_SLOW_NUM;  // rows of ZW_P1P_SLOW_DEN rounds
    static constexpr int span = L * nslow;  // rows within which every wave that takes rows above J has one

    static ZW_HD int join_row(int mbh)
    {
        return mbh < ZW_P1P_JOIN_MIN ? mbh : (mbh * ZW_P1P_JOIN_NUM + ZW_P1P_JOIN_DEN - 1) / ZW_P1P_JOIN_DEN;
    }
    static ZW_HD int fast_wave(int i) { return (i / (4 - NCH)) * 4 + NCH + i % (4 - NCH); }  // 2, 3, 6, 7, 10, 11
    static ZW_HD int slow_wave(int i) { return 4 * (1 + i / NCH) + i % NCH; }                // 4, 5, 8, 9
    // the owner of row y above the join row
    static ZW_HD int round_wave(int y)
    {
        int r = y % L, before = (y / L) * ZW_P1P_SLOW_NUM;
        for (int k = 0; k < ZW_P1P_SLOW_DEN; k++) {
            const int sk = ((k + 1) * ZW_P1P_SLOW_NUM) / ZW_P1P_SLOW_DEN - (k * ZW_P1P_SLOW_NUM) / ZW_P1P_SLOW_DEN;
            if (r < nfast) return fast_wave(r);
            r -= nfast;
            if (r < sk) return slow_wave((before + r) % nslow);
            r -= sk;
            before += sk;
        }
        return NCH;  // unreachable
    }
    // the waves met walking up from row J - 1, nearest first, a nibble each;
    // `seen`: their bits, `n`: how many
    static ZW_HD unsigned long long join_scan(int J, unsigned& seen, int& n)
    {
        unsigned long long ord = 0;
        seen = 0;
        n = 0;
        for (int y = J - 1; y >= 0 && y >= J - span; y--) {
            const int w = round_wave(y);
            if (!((seen >> w) & 1u)) {
                seen |= 1u << w;
                ord |= (unsigned long long)w << (4 * n++);
            }
        }
        return ord;
    }
    // the wave's place in the rounds from row J on, and the wave of place k
    static ZW_HD int join_rank(int wave, int J)
    {
        unsigned seen;
        int n;
        const unsigned long long ord = join_scan(J, seen, n);
        if ((seen >> wave) & 1u) {
            int i = 0;
            while ((int)((ord >> (4 * i)) & 15u) != wave) i++;
            return NW - 1 - i;
        }
        int r = 0;
        for (int v = 0; v < wave; v++) r += (int)!((seen >> v) & 1u);
        return r;
    }
    static ZW_HD int join_wave(int k, int J)
    {
        unsigned seen;
        int n;
        const unsigned long long ord = join_scan(J, seen, n);
        if (k >= NW - n) return (int)((ord >> (4 * (NW - 1 - k))) & 15u);
        int w = 0;
        for (;; w++)
            if (!((seen >> w) & 1u) && k-- == 0) break;
        return w;
    }
    static ZW_HD int wave_of_row(int y, int mbh)
    {
        const int J = join_row(mbh);
        return y < J ? round_wave(y) : join_wave((y - J) % NW, J);
    }
    // the wave's next row after `y` (mbh or more: none)
    static ZW_HD int next_row(int wave, int y, int mbh)
    {
        const int J = join_row(mbh);
        for (y++; y < J; y++)
            if (round_wave(y) == wave) return y;
        if (y >= mbh) return y;
        const int k = join_rank(wave, J);
        return y + (k - (y - J) % NW + NW) % NW;
    }
    static ZW_HD int first_row(int wave, int mbh) { return next_row(wave, -1, mbh); }
};
