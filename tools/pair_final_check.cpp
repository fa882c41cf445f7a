// Host check of the paired final luma transform's task masks
// (image-webp_amd/csrc/zw_enc_pairfinal.h): which (block, start context)
// trellis runs an I16 MB needs, and how the runs of a frame pair's two MBs are
// numbered onto the lanes of one wave.
//
// On the device a block gathers its levels from the lane pf_task names for its
// resolved context: a context missing from the block's mask, or a numbering
// that is no bijection, reads another block's levels or a lane past the wave.
// So the masks are walked here, where nothing can go out of range:
//   - over all 2^16 trivially-zero patterns x 256 edge-flag settings, pf_need
//     equals the definition written out with branches (known neighbours: the
//     MB's edges and its trivially zero blocks; contexts min(k + t, 2), t = 0..u);
//   - an MB never needs more than ZW_PF_MAX_TASKS (40) tasks;
//   - for a seeded sample of patterns and, per pattern, 64 seeded nonzero
//     outcomes of the non-trivial blocks, the context the raster chain gives
//     every non-trivial block is in that block's mask;
//   - pf_task over two MBs' masks (the second based at the first's count) is a
//     bijection onto 0 .. n - 1, also for the fallback mask ZW_PF_ALL;
//   - pf_one_call is n <= 64.
// With arguments `trivial Q_AC` it reads coefficient blocks (16 integers a
// line, natural order) from stdin and prints pf_trivial of each under the Y1
// matrix of that AC quantiser; tests/test_enc_pair_final.py pins those against
// the oracle's trellis.
//
//   g++ -O2 -std=c++17 -I image-webp_amd/csrc tools/pair_final_check.cpp -o pair_final_check && ./pair_final_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "zw_enc_pairfinal.h"

static int bad = 0;
static void fail(const char* what, unsigned triv, unsigned edge, int a, int b)
{
    if (bad++ < 20) std::printf("triv %04x edge %02x: %s (%d, %d)\n", triv, edge, what, a, b);
}

// the definition, with branches
static unsigned need_ref(int b, unsigned triv, unsigned edge)
{
    if ((triv >> b) & 1u) return 0;
    const int bx = b & 3, by = b >> 2;
    int k = 0, u = 0;
    if (bx == 0) k += (edge >> (4 + by)) & 1u;
    else if (!((triv >> (b - 1)) & 1u)) u++;
    if (by == 0) k += (edge >> bx) & 1u;
    else if (!((triv >> (b - 4)) & 1u)) u++;
    unsigned m = 0;
    for (int t = 0; t <= u; t++) m |= 1u << (k + t < 2 ? k + t : 2);
    return m;
}

static uint64_t rng_state = 0x5EEDF17A1ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// every non-trivial block's chain context under the nonzero outcome nz is in its mask
static void check_chain(unsigned triv, unsigned edge, unsigned nz)
{
    int top[4], left[4];
    for (int q = 0; q < 4; q++) {
        top[q] = (edge >> q) & 1u;
        left[q] = (edge >> (4 + q)) & 1u;
    }
    for (int b = 0; b < 16; b++) {
        const int cx = left[b >> 2] + top[b & 3] < 2 ? left[b >> 2] + top[b & 3] : 2;
        const bool tz = (triv >> b) & 1u;
        if (!tz && !((pf_need(b, triv, edge) >> cx) & 1u)) fail("chain context not in the block's mask", triv, edge, b, cx);
        const int z = tz ? 0 : (nz >> b) & 1u;
        top[b & 3] = left[b >> 2] = z;
    }
}

static void check_numbering(uint64_t ma, uint64_t mb, unsigned triv, unsigned edge)
{
    const int na = pf_count(ma), n = na + pf_count(mb);
    if (pf_one_call(ma, mb) != (n <= ZW_PF_LANES)) fail("pf_one_call differs from the count", triv, edge, n, 0);
    unsigned char seen[96];
    std::memset(seen, 0, sizeof seen);
    for (int f = 0; f < 2; f++) {
        const uint64_t m = f ? mb : ma;
        for (int cx = 0; cx < 3; cx++)
            for (int b = 0; b < 16; b++) {
                if (!((m >> (cx * 16 + b)) & 1ull)) continue;
                const int t = pf_task(m, f ? na : 0, b, cx);
                if (t < 0 || t >= n) fail("task outside 0 .. n - 1", triv, edge, t, n);
                else if (seen[t]++) fail("two tasks with one number", triv, edge, t, n);
            }
    }
    for (int t = 0; t < n; t++)
        if (!seen[t]) fail("a number with no task", triv, edge, t, n);
}

static int trivial_filter(const char* qarg)
{
    const uint32_t q_ac = (uint32_t)std::atoi(qarg);
    if (q_ac == 0) return 2;
    static const uint8_t freq_sharpening[16] = {0, 30, 60, 90, 30, 60, 90, 90, 60, 90, 90, 90, 90, 90, 90, 90};
    uint16_t sharpen[16];
    for (int i = 0; i < 16; i++) sharpen[i] = (uint16_t)(((uint32_t)freq_sharpening[i] * q_ac) >> 11);  // (i >= 1: the AC step)
    const uint32_t iq_ac = (1u << 17) / q_ac;
    int c[16];
    for (;;) {
        for (int i = 0; i < 16; i++)
            if (std::scanf("%d", &c[i]) != 1) return 0;
        std::printf("%d\n", pf_trivial(c, q_ac, iq_ac, sharpen) ? 1 : 0);
    }
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "trivial")) return trivial_filter(argv[2]);
    int most = 0;
    for (unsigned triv = 0; triv < 65536u; triv++)
        for (unsigned edge = 0; edge < 256u; edge++) {
            int n = 0;
            uint64_t m = 0;
            for (int b = 0; b < 16; b++) {
                const unsigned nd = pf_need(b, triv, edge), ref = need_ref(b, triv, edge);
                if (nd != ref) fail("pf_need differs from the definition", triv, edge, b, (int)(nd * 8 + ref));
                n += __builtin_popcount(nd);
                for (int cx = 0; cx < 3; cx++) m |= (uint64_t)((nd >> cx) & 1u) << (cx * 16 + b);
            }
            if (n > ZW_PF_MAX_TASKS) fail("more than 40 tasks", triv, edge, n, 0);
            if (m != pf_mask(triv, edge) || pf_count(m) != n) fail("pf_mask / pf_count differ from pf_need", triv, edge, n, 0);
            most = n > most ? n : most;
        }
    if (most != ZW_PF_MAX_TASKS) fail("the largest MB is not 40 tasks", 0, 0, most, 0);
    // sampled patterns: the chain's contexts, and the numbering against a second MB
    long chains = 0, pairs = 0;
    for (int s = 0; s < 20000; s++) {
        // (sparse, dense and uniform patterns)
        unsigned triv = rnd() & 0xffffu;
        if (s % 3 == 1) triv |= rnd() & 0xffffu;
        if (s % 3 == 2) triv &= rnd() & 0xffffu;
        const unsigned edge = rnd() & 0xffu;
        for (int k = 0; k < 64; k++, chains++) check_chain(triv, edge, k == 0 ? 0u : (k == 1 ? 0xffffu : rnd() & 0xffffu));
        unsigned triv2 = rnd() & 0xffffu;
        if (s % 2) triv2 &= rnd() & 0xffffu;
        const unsigned edge2 = rnd() & 0xffu;
        check_numbering(pf_mask(triv, edge), pf_mask(triv2, edge2), triv, edge);
        check_numbering(pf_mask(triv, edge), 0, triv, edge);
        check_numbering(0, pf_mask(triv2, edge2), triv2, edge2);
        pairs += 3;
    }
    // every pattern's chain under the all-nonzero and all-zero outcomes too
    for (unsigned triv = 0; triv < 65536u; triv++)
        for (unsigned edge = 0; edge < 256u; edge += 17) {
            check_chain(triv, edge, 0xffffu);
            check_chain(triv, edge, 0u);
        }
    check_numbering(ZW_PF_ALL, 0, 0, 0);
    check_numbering(0, ZW_PF_ALL, 0, 0);
    check_numbering(0, 0, 0xffff, 0);
    if (pf_one_call(ZW_PF_ALL, ZW_PF_ALL)) fail("96 tasks in one call", 0, 0, 96, 0);
    if (bad) {
        std::printf("%d failures\n", bad);
        return 1;
    }
    std::printf("ok: 65536 x 256 masks, most %d tasks an MB, %ld chains, %ld numberings\n", most, chains, pairs);
    return 0;
}
