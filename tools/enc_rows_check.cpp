// Host check of the encode kernels' row schedule (image-webp_amd/csrc/zw_enc_rows.h).
//
// On the device a luma wave waits on the wave that owns the row above: a row
// that no wave works, or that the schedule gives to a chain wave, hangs the
// kernel.  So the shipped shapes are walked here, where nothing can hang.  For
// every frame height from 1 to 300 MB rows:
//   - every row belongs to exactly one wave, a luma wave (never a chain wave);
//   - first_row / next_row over all luma waves visit every row once, in
//     increasing order per wave, and only rows wave_of_row gives that wave.
//
//   g++ -O2 -std=c++17 -I image-webp_amd/csrc tools/enc_rows_check.cpp -o enc_rows_check && ./enc_rows_check
#include <cstdio>
#include <vector>

#include "zw_enc_rows.h"

template <class RS, int NW, int NCH> static int check(const char* name)
{
    int bad = 0;
    auto fail = [&](int mbh, const char* what, int a, int b) {
        if (bad++ < 10) std::printf("%s mbh %d: %s (%d, %d)\n", name, mbh, what, a, b);
    };
    for (int mbh = 1; mbh <= 300; mbh++) {
        std::vector<int> visits(mbh, 0);
        for (int y = 0; y < mbh; y++) {
            const int w = RS::wave_of_row(y);
            if (w < NCH || w >= NW) fail(mbh, "row owned by a chain wave or by none", y, w);
        }
        for (int w = NCH; w < NW; w++) {
            int prev = -1;
            for (int y = RS::first_row(w, mbh); y < mbh; y = RS::next_row(w, y, mbh)) {
                if (y <= prev) {
                    fail(mbh, "rows of a wave not increasing", w, y);
                    break;  // (would not terminate)
                }
                if (RS::wave_of_row(y) != w) fail(mbh, "wave walks a row it does not own", w, y);
                visits[y]++;
                prev = y;
            }
        }
        for (int y = 0; y < mbh; y++)
            if (visits[y] != 1) fail(mbh, "row not visited exactly once", y, visits[y]);
    }
    return bad;
}

int main()
{
    int bad = 0;
    // the batch kernels: 12 waves; pass 1 with one chain wave (skip mode)
    using P1 = RowSchedule<1, false, 12, 1>;
    static_assert(ZW_P1_SLOWSKIP == 0 || P1::skip_mode, "pass 1 batch shape: the skip-mode schedule");
    bad += check<P1, 12, 1>("pass 1 batch");
    // the shipped pass-1 order itself (one SIMD-0 row per round of nine others,
    // waves 4 and 8 in turn): a consistent but different order would change the
    // pass's speed, so it is pinned
    if (ZW_P1_SLOWSKIP == 1 && ZW_P1_SLOW_NUM == 1 && ZW_P1_SLOW_DEN == 1) {
        const int want[20] = {1, 2, 3, 5, 6, 7, 9, 10, 11, 4, 1, 2, 3, 5, 6, 7, 9, 10, 11, 8};
        for (int y = 0; y < 40; y++)
            if (P1::wave_of_row(y) != want[y % 20]) {
                std::printf("pass 1 batch: row %d goes to wave %d, shipped order has %d\n", y, P1::wave_of_row(y), want[y % 20]);
                bad++;
            }
    }
    // pass 1's ordered round-robin (ZW_P1_ORDER; what skip mode off, -DZW_P1_SLOWSKIP=0, runs):
    // the waves on the chain's SIMD, 4 and 8, take the last rows of a round
    if (ZW_P1_ORDER == 1) {
        using PO = RowSchedule<1, true, 12, 1>;  // (ROWS: no skip mode)
        const int want[11] = {1, 2, 3, 5, 6, 7, 9, 10, 11, 4, 8};
        for (int k = 0; k < 11; k++)
            if (PO::luma_wave(k) != want[k] || PO::luma_rank(want[k]) != k) {
                std::printf("pass 1 order: row %d of a round goes to wave %d, shipped order has %d\n", k, PO::luma_wave(k), want[k]);
                bad++;
            }
    }
    bad += check<RowSchedule<2, false, 12, 0>, 12, 0>("pass 2 batch");
    // the frame-pair kernels: round-robin over the luma waves (pass 1: two chain waves)
    bad += check<RowSchedule<1, false, 12, 2, true>, 12, 2>("pass 1 pairs");
    bad += check<RowSchedule<2, false, 12, 0, true>, 12, 0>("pass 2 pairs");
    if (bad) {
        std::printf("FAILED: %d\n", bad);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
