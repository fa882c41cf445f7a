// Host check of pass 1's frame-pair row schedule (PairRowSchedule1 in
// image-webp_amd/csrc/zw_enc_rows.h): 12 waves, of which waves 0 and 1 run the
// chroma chains first and take rows from the join row J(mbh) on.
//
// On the device a wave waits on the wave that owns the row above, and the chain
// waves reach their rows only after their chains: a row with no owner or two,
// a wave whose rows do not increase, or a walk that differs from wave_of_row
// is a hang.  So the schedule is walked here, where nothing can hang.  For
// every frame height from 1 to 300 MB rows:
//   - every row belongs to exactly one of the 12 waves;
//   - first_row / next_row of every wave visit only rows wave_of_row gives that
//     wave, in strictly increasing order, and together every row once;
//   - no chain wave owns a row above J(mbh), and the rows above J go to the
//     luma waves in the rounds the knobs describe (each fast wave once a round);
//   - frames under the floor have no join: J = mbh, the chain waves own nothing;
//   - from J on every 12 rows in sequence have 12 different owners, and they
//     come in the order the waves come free (by their last row above J);
//   - run as the kernel runs it (a wave works its rows in order, row y needs
//     row y - 1 finished by its owner, the chains wait on nothing), every row
//     gets done.
// The shipped order at the headline height (68 rows) is pinned.
//
//   g++ -O2 -std=c++17 -I image-webp_amd/csrc tools/enc_pair_rows_check.cpp -o enc_pair_rows_check && ./enc_pair_rows_check
#include <cstdio>
#include <vector>

#include "zw_enc_rows.h"

constexpr int NW = 12, NCH = 2;
using RP = PairRowSchedule1<NW, NCH>;

static int bad = 0;
static void fail(int mbh, const char* what, int a, int b)
{
    if (bad++ < 20) std::printf("pass 1 pairs mbh %d: %s (%d, %d)\n", mbh, what, a, b);
}

static bool slow(int w) { return (w & 3) < NCH; }

static void check(int mbh)
{
    const int J = RP::join_row(mbh);
    if (J < 0 || J > mbh) fail(mbh, "join row outside the frame", J, mbh);
    if (mbh < ZW_P1P_JOIN_MIN && J != mbh) fail(mbh, "a join under the floor", J, ZW_P1P_JOIN_MIN);
    std::vector<int> owner(mbh), visits(mbh, 0);
    for (int y = 0; y < mbh; y++) {
        const int w = owner[y] = RP::wave_of_row(y, mbh);
        if (w < 0 || w >= NW) fail(mbh, "row owned by no wave", y, w);
        else if (y < J && w < NCH) fail(mbh, "chain wave owns a row above the join row", y, w);
        else if (mbh < ZW_P1P_JOIN_MIN && w < NCH) fail(mbh, "chain wave owns a row under the floor", y, w);
    }
    // the walk of every wave, chain waves included
    std::vector<std::vector<int>> rows(NW);
    for (int w = 0; w < NW; w++) {
        int prev = -1;
        for (int y = RP::first_row(w, mbh); y < mbh; y = RP::next_row(w, y, mbh)) {
            if (y <= prev) {
                fail(mbh, "rows of a wave not increasing", w, y);
                break;  // (would not terminate)
            }
            if (owner[y] != w) fail(mbh, "wave walks a row it does not own", w, y);
            visits[y]++;
            rows[w].push_back(y);
            prev = y;
        }
    }
    for (int y = 0; y < mbh; y++)
        if (visits[y] != 1) fail(mbh, "row not visited exactly once", y, visits[y]);
    // above J: rounds of the fast waves' rows, then the round's slow rows
    for (int y = 0, in_round = 0; y < J; y++) {
        if (!slow(owner[y])) {
            if (owner[y] != RP::fast_wave(in_round % RP::nfast)) fail(mbh, "fast rows of a round out of order", y, owner[y]);
            in_round++;
        } else if (in_round % RP::nfast != 0) {
            fail(mbh, "slow row inside a round's fast rows", y, owner[y]);
        }
    }
    {
        // the slow-row share: ZW_P1P_SLOW_NUM slow rows in every ZW_P1P_SLOW_DEN whole rounds
        int ns = 0;
        for (int y = 0; y < J && y < RP::L * (J / RP::L); y++) ns += (int)slow(owner[y]);
        if (ns != (J / RP::L) * ZW_P1P_SLOW_NUM) fail(mbh, "slow-row share", ns, (J / RP::L) * ZW_P1P_SLOW_NUM);
    }
    // from J on: all 12 waves in turn, in the order they come free
    for (int y = J; y < mbh; y++) {
        for (int z = y + 1; z < mbh && z < y + NW; z++)
            if (owner[z] == owner[y]) fail(mbh, "a wave twice within 12 rows after the join", y, z);
        if (y + NW < mbh && owner[y + NW] != owner[y]) fail(mbh, "rounds after the join differ", y, owner[y + NW]);
    }
    auto last_above = [&](int w) {
        for (int y = J - 1; y >= 0; y--)
            if (owner[y] == w) return y;
        return -1;
    };
    for (int k = 1; k < NW && J + k < mbh; k++)
        if (last_above(owner[J + k]) < last_above(owner[J + k - 1]))
            fail(mbh, "join order: a wave before one that comes free earlier", J + k, owner[J + k]);
    // run it: done[y] once its owner has reached it and row y - 1 is done
    std::vector<size_t> at(NW, 0);
    std::vector<char> done(mbh, 0);
    int ndone = 0;
    for (bool moved = true; moved;) {
        moved = false;
        for (int w = 0; w < NW; w++)
            while (at[w] < rows[w].size() && (rows[w][at[w]] == 0 || done[rows[w][at[w]] - 1])) {
                done[rows[w][at[w]++]] = 1;
                ndone++;
                moved = true;
            }
    }
    if (ndone != mbh) fail(mbh, "the walk stalls: rows done", ndone, mbh);
}

int main()
{
    for (int mbh = 1; mbh <= 300; mbh++) check(mbh);
    // the floor itself: the first height with a join has chain-wave rows
    {
        const int mbh = ZW_P1P_JOIN_MIN;
        int nchain = 0;
        for (int y = 0; y < mbh; y++) nchain += (int)(RP::wave_of_row(y, mbh) < NCH);
        if (RP::join_row(mbh) < mbh && nchain == 0) fail(mbh, "no join at the floor", RP::join_row(mbh), mbh);
    }
    // the shipped order at 1080p (68 rows): a consistent but different order
    // would change the pass's speed, so it is pinned
    if (ZW_P1P_SLOW_NUM == 4 && ZW_P1P_SLOW_DEN == 1 && ZW_P1P_JOIN_NUM == 5 && ZW_P1P_JOIN_DEN == 8 &&
        ZW_P1P_JOIN_MIN <= 68) {
        // four rounds of the six fast and the four slow waves, rows 40..42 of a
        // fifth, then from row 43 all twelve, the chain waves first
        const int want[68] = {2, 3, 6, 7, 10, 11, 4, 5, 8, 9, 2, 3, 6, 7, 10, 11, 4, 5, 8, 9, 2, 3, 6,
                              7, 10, 11, 4, 5, 8, 9, 2, 3, 6, 7, 10, 11, 4, 5, 8, 9, 2, 3, 6,
                              0, 1, 7, 10, 11, 4, 5, 8, 9, 2, 3, 6, 0, 1, 7, 10, 11, 4, 5, 8, 9, 2, 3, 6, 0};
        if (RP::join_row(68) != 43) fail(68, "shipped join row", RP::join_row(68), 43);
        for (int y = 0; y < 68; y++)
            if (RP::wave_of_row(y, 68) != want[y]) {
                std::printf("pass 1 pairs: row %d goes to wave %d, shipped order has %d\n", y, RP::wave_of_row(y, 68), want[y]);
                bad++;
            }
    } else {
        std::printf("(knobs differ from the shipped ones: order not pinned)\n");
    }
    if (bad) {
        std::printf("FAILED: %d\n", bad);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
