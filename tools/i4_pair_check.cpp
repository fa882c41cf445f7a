// Host check of the paired I4 search's lane maps and lane-form state
// (image-webp_amd/csrc/zw_enc_i4pair.h), walked where nothing can go out of
// range.  The cross-lane instructions of i4p_step (zw_enc_kernels.hip) are
// modelled here on arrays of 64 lanes: the forward permute (a lane's value
// lands in the lane it names, a lane nobody names receives 0, the highest
// sender wins a collision), the quad broadcast, the rotations within a 16-lane
// row and the swap of neighbouring rows.
//
//   - candidate modes: for ranks that are a permutation of 0..9 per group (the
//     identity, the reversal and seeded ones), both step forms (NB = 1, 2) and
//     K = 3, 4, lane (g, k, q) receives exactly the mode of rank k, from a lane
//     of its own group that exactly one lane wrote; lanes k >= K are ineligible
//     and hold a valid mode;
//   - state: over seeded sequences of winners along the ten anti-diagonal
//     steps, every lane's state equals a plain per-MB model of I4State (the
//     scalar form's update), the contexts it gives the next step's blocks are
//     the model's, the chosen modes stored are the model's, and the two exits
//     decide as the model's do.
//
//   g++ -O2 -std=c++17 -I image-webp_amd/csrc tools/i4_pair_check.cpp -o i4_pair_check && ./i4_pair_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "zw_enc_i4pair.h"

static int bad = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond) && bad++ < 20) {                      \
            std::printf("%s:%d: ", __FILE__, __LINE__);   \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static uint64_t rng_state = 0x14A9E5EEDull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// ---- the cross-lane instructions, on 64 lanes ----
static void permute_fwd(const int* dest, const int* val, int* out, int* writers)
{
    for (int l = 0; l < 64; l++) out[l] = 0, writers[l] = 0;
    for (int l = 0; l < 64; l++) {
        out[dest[l] & 63] = val[l];
        writers[dest[l] & 63]++;
    }
}
static void row_ror_or(uint32_t* v, int n)  // v |= row_ror:n (v)
{
    uint32_t t[64];
    for (int l = 0; l < 64; l++) t[l] = v[(l & ~15) | ((l - n) & 15)];
    for (int l = 0; l < 64; l++) v[l] |= t[l];
}
// permlane16_swap(v, v): [0] the even row's value in both rows of a pair, [1] the odd row's
static void row_swap(const uint32_t* v, uint32_t* r0, uint32_t* r1)
{
    for (int l = 0; l < 64; l++) {
        r0[l] = v[l & ~16];
        r1[l] = v[l | 16];
    }
}

// ---- candidate modes ----
static long n_modes = 0;
static void check_modes(const int perm[4][10], int NB, int K)
{
    int rank[64], dest[64], val[64], got[64], writers[64];
    for (int l = 0; l < 64; l++) {
        const int g = NB == 2 ? l >> 4 : (l >> 4) & ~1, m = l & 15;  // (NB = 1: slot-1 rows repeat slot 0)
        rank[l] = m < 10 ? perm[g][m] : 10;
        dest[l] = i4p_inv_dest(l, rank[l]);
        val[l] = m;
        CHECK(dest[l] >= 0 && dest[l] < 64 && (dest[l] >> 4) == (l >> 4), "lane %d sends to lane %d", l, dest[l]);
    }
    permute_fwd(dest, val, got, writers);
    for (int l = 0; l < 64; l++) {
        const int g = NB == 2 ? l >> 4 : (l >> 4) & ~1, k = (l >> 2) & 3;
        const int src = i4p_mode_src(l);
        CHECK(src >= 0 && src < 64 && (src >> 4) == (l >> 4), "lane %d reads lane %d", l, src);
        const int mode = i4p_mode(l, K, got[src]);
        CHECK(i4p_eligible(l, K) == (k < K), "lane %d eligibility", l);
        CHECK(mode >= 0 && mode < 10, "lane %d mode %d", l, mode);
        if (k < K) {
            CHECK(writers[src] == 1, "lane %d reads lane %d with %d writers", l, src, writers[src]);
            CHECK(perm[g][mode] == k, "lane %d: mode %d has rank %d, not %d", l, mode, perm[g][mode], k);
        }
        n_modes++;
    }
}

// ---- state ----
struct Model {  // I4State, and its update in the scalar form
    uint64_t running, mpack;
    uint32_t total_mc, tnz, lnz, nzm;
    uint8_t modes[16];
};

static long n_steps = 0, n_exit[2] = {0, 0};
static void check_state(int K)
{
    const uint32_t l_mode[2] = {1 + rnd() % 4000, 1 + rnd() % 4000};
    const uint32_t mc_scale = (rnd() & 1) ? 600 : 6000;  // (6000: the mode-cost cap is crossed)
    uint64_t lim[2];
    for (int mb = 0; mb < 2; mb++) lim[mb] = (uint64_t)(rnd() % 16 + 1) * (400000ull * 256 + 30000ull * l_mode[mb]) / 2;
    I4PState st[64];
    Model M[2];
    uint8_t stored[2][16] = {{0}};
    for (int l = 0; l < 64; l++) i4p_state_init(st[l], l_mode[l >> 5]);
    for (int mb = 0; mb < 2; mb++) {
        M[mb] = Model();
        M[mb].running = 211ull * l_mode[mb];
    }
    for (int s = 0; s < 10; s++) {
        const int sbyA = s < 4 ? 0 : (s - 2) >> 1, sbxA = s - 2 * sbyA;
        const int NB = s >= 2 && s <= 7 ? 2 : 1;
        const int sbx[2] = {sbxA, sbxA - 2}, sby[2] = {sbyA, sbyA + 1};
        // the lanes' contexts against the model's, before the step
        for (int l = 0; l < 64; l++) {
            const int mb = l >> 5, h = NB == 2 ? (l >> 4) & 1 : 0, bx = sbx[h], by = sby[h], i = by * 4 + bx;
            const int tc = by == 0 ? 0 : (int)((M[mb].mpack >> (4 * (i - 4))) & 15);
            const int lc = bx == 0 ? 0 : (int)((M[mb].mpack >> (4 * (i - 1))) & 15);
            const int nc = (by == 0 ? 0 : (int)((M[mb].tnz >> bx) & 1)) + (bx == 0 ? 0 : (int)((M[mb].lnz >> by) & 1));
            CHECK(i4p_tctx(st[l], bx, by) == tc, "step %d lane %d top mode", s, l);
            CHECK(i4p_lctx(st[l], bx, by) == lc, "step %d lane %d left mode", s, l);
            CHECK(i4p_nzctx(st[l], bx, by) == nc, "step %d lane %d nonzero context", s, l);
        }
        // the candidates of the four groups (NB = 1: slot-1 rows repeat slot 0) and their winners
        I4PWin cand[4][4];
        int kwin[4];
        for (int g = 0; g < 4; g++) {
            const int gs = NB == 2 ? g : g & ~1;
            if (gs != g) {
                for (int k = 0; k < 4; k++) cand[g][k] = cand[gs][k];
                kwin[g] = kwin[gs];
                continue;
            }
            for (int k = 0; k < 4; k++)
                cand[g][k] = i4p_win(rnd() & 0xffff, rnd() % mc_scale, rnd() & 1, rnd() % (16 * 255 * 255 + 1), (int)(rnd() % 10));
            kwin[g] = (int)(rnd() % K);
        }
        uint32_t w0[64], w1[64], p0[2][64], p1[2][64];
        for (int l = 0; l < 64; l++) {
            const int g = l >> 4, k = (l >> 2) & 3;
            const bool winl = k == kwin[g];
            w0[l] = winl ? cand[g][k].pk : 0;
            w1[l] = winl ? cand[g][k].sm : 0;
        }
        row_ror_or(w0, 8), row_ror_or(w1, 8), row_ror_or(w0, 4), row_ror_or(w1, 4);
        row_swap(w0, p0[0], p0[1]);
        row_swap(w1, p1[0], p1[1]);
        for (int l = 0; l < 64; l++) {
            const int mb = l >> 5;
            if (NB == 2) {
                for (int h = 0; h < 2; h++) {
                    I4PWin w = {p0[h][l], p1[h][l]};
                    i4p_state_update(st[l], sbx[h], sby[h], w, l_mode[mb]);
                }
            } else {
                I4PWin w = {w0[l], w1[l]};
                i4p_state_update(st[l], sbx[0], sby[0], w, l_mode[mb]);
            }
            if ((l & 15) == 0 && ((l >> 4) & 1) < NB) {
                const int h = (l >> 4) & 1;
                stored[mb][sby[h] * 4 + sbx[h]] = (uint8_t)(w1[l] >> 24);
            }
        }
        // the model
        for (int mb = 0; mb < 2; mb++)
            for (int h = 0; h < NB; h++) {
                const I4PWin& w = cand[2 * mb + h][kwin[2 * mb + h]];
                const uint32_t bnz = w.pk >> 31, bmode = w.sm >> 24, bsse = w.sm & 0xffffffu;
                const int i = sby[h] * 4 + sbx[h];
                Model& m = M[mb];
                m.tnz = (m.tnz & ~(1u << sbx[h])) | (bnz << sbx[h]);
                m.lnz = (m.lnz & ~(1u << sby[h])) | (bnz << sby[h]);
                m.nzm |= bnz << i;
                m.total_mc += (w.pk >> 16) & 0x7fffu;
                m.running += (uint64_t)bsse * 256ull + (uint64_t)(uint16_t)(w.pk & 0xffffu) * l_mode[mb];
                m.mpack |= (uint64_t)bmode << (4 * i);
                m.modes[i] = (uint8_t)bmode;
            }
        for (int l = 0; l < 64; l++) {
            const Model& m = M[l >> 5];
            CHECK(st[l].running == m.running, "step %d lane %d running", s, l);
            CHECK(st[l].total_mc == m.total_mc, "step %d lane %d total_mc", s, l);
            CHECK((st[l].nzt & 0xffffu) == m.nzm, "step %d lane %d nonzero flags", s, l);
            const bool ex = m.running >= lim[l >> 5] || m.total_mc > 256u * 16u * 16u / 4u;
            CHECK(i4p_exit(st[l], lim[l >> 5]) == ex, "step %d lane %d exit", s, l);
            if ((l & 31) == 0) n_exit[ex]++;
        }
        n_steps++;
    }
    for (int mb = 0; mb < 2; mb++)
        for (int i = 0; i < 16; i++) CHECK(stored[mb][i] == M[mb].modes[i], "MB %d block %d stored mode", mb, i);
}

int main()
{
    for (int NB = 1; NB <= 2; NB++)
        for (int K = 3; K <= 4; K++) {
            int perm[4][10];
            for (int g = 0; g < 4; g++)
                for (int m = 0; m < 10; m++) perm[g][m] = m;
            check_modes(perm, NB, K);
            for (int g = 0; g < 4; g++)
                for (int m = 0; m < 10; m++) perm[g][m] = 9 - m;
            check_modes(perm, NB, K);
            for (int t = 0; t < 3000; t++) {
                for (int g = 0; g < 4; g++) {
                    for (int m = 0; m < 10; m++) perm[g][m] = m;
                    for (int m = 9; m > 0; m--) {
                        const int j = (int)(rnd() % (uint32_t)(m + 1)), x = perm[g][m];
                        perm[g][m] = perm[g][j];
                        perm[g][j] = x;
                    }
                }
                check_modes(perm, NB, K);
            }
        }
    for (int K = 3; K <= 4; K++)
        for (int t = 0; t < 3000; t++) check_state(K);
    // (both outcomes of the exits occur, so the comparison is not vacuous)
    CHECK(n_exit[0] > 1000 && n_exit[1] > 1000, "exits %ld / %ld", n_exit[0], n_exit[1]);
    if (bad) {
        std::printf("FAILED: %d checks\n", bad);
        return 1;
    }
    std::printf("ok: %ld lane modes, %ld steps (exits %ld no / %ld yes)\n", n_modes, n_steps, n_exit[0], n_exit[1]);
    return 0;
}
