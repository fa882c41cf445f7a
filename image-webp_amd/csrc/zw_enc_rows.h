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
// their rows from a ticket instead and only share the type.
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
