// Host check of the paired I4 search's value vector and of its ranking key
// (image-webp_amd/csrc/zw_enc_i4pair.h), walked where nothing can go out of
// range.
//
//   - value vector: for edge vectors E = [L3..L0, P, A0..A7] (all 0, all 255,
//     every 0/255 alternation of period 1 and 2 in both phases, single spikes
//     up and down at every position, spikes against a mid grey, and seeded
//     ones -- uniform bytes and bytes near the two ends), the 55 entries are
//     formed lane by lane as i4p_values forms them (i4p_value_map, i4p_value,
//     the DC as its reduction) and every pixel of the ten modes, read through
//     the paired index table (i4p_vindex over ZW_I4_IDX_ROWS), equals the ten
//     predictors written plainly from the VP8 rules; every edge index a lane
//     reads lies in E.  TrueMotion's L + A - P leaves 0..255 on both sides
//     (counted, so the clamp is not checked vacuously), and no other entry is
//     changed by the clamp;
//   - packing: on a model of v_perm_b32, for seeded and extreme gathered words
//     and the four (MB, slot) groups, the ranking's row (i4p_bsel,
//     i4p_pack_row) holds the group's bytes of the four words in pixel order,
//     the candidate phase's pairs (i4p_psel) are (x0, x1) and (x3, x2), and
//     ZW_I4P_PAIRS_TO_ROW makes the same row of them;
//   - key: for seeded and extreme (0 / 255) sources and predictions, and for
//     constructed ties of two, four and all ten modes, the ranks from
//     i4p_rank_key(pp, sp, m) equal the ranks from sse << 4 | m, and the key
//     lies in (0, 2^27) (rank16 takes keys in [0, 2^31)).
//
//   g++ -O2 -std=c++17 -I image-webp_amd/csrc tools/i4_rank_check.cpp -o i4_rank_check && ./i4_rank_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static const uint8_t kIdx[10][16] = {ZW_I4_IDX_ROWS};

// ---- the ten predictors, plainly (RFC 6386 section 12.3; modes in the
// bitstream's order: DC TM VE HE LD RD VR VL HD HU) ----
static int avg2(int a, int b) { return (a + b + 1) >> 1; }
static int avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
static int clip(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// E = [L3 L2 L1 L0 P A0..A7]; out[4 * row + col]
static void predict(int mode, const int* Ev, int* out)
{
    const int L[4] = {Ev[3], Ev[2], Ev[1], Ev[0]}, P = Ev[4];
    const int* A = Ev + 5;
    // the edge as one line, bottom-left to top-right: e[0] = L3 .. e[3] = L0, e[4] = P, e[5..12] = A0..A7
    const int* e = Ev;
    auto px = [&](int r, int c) -> int& { return out[4 * r + c]; };
    switch (mode) {
    case 0: {
        int s = 4;
        for (int i = 0; i < 4; i++) s += L[i] + A[i];
        for (int i = 0; i < 16; i++) out[i] = s >> 3;
        break;
    }
    case 1:
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) px(r, c) = clip(L[r] + A[c] - P);
        break;
    case 2:  // VE: the smoothed row above
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) px(r, c) = avg3(c == 0 ? P : A[c - 1], A[c], A[c + 1]);
        break;
    case 3:  // HE: the smoothed left column, the last row from (L2, L3, L3)
        for (int c = 0; c < 4; c++) {
            px(0, c) = avg3(P, L[0], L[1]);
            px(1, c) = avg3(L[0], L[1], L[2]);
            px(2, c) = avg3(L[1], L[2], L[3]);
            px(3, c) = avg3(L[2], L[3], L[3]);
        }
        break;
    case 4:  // LD: down-left along the row above
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                const int i = r + c;
                px(r, c) = i == 6 ? avg3(A[6], A[7], A[7]) : avg3(A[i], A[i + 1], A[i + 2]);
            }
        break;
    case 5:  // RD: down-right across the corner
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                const int i = 4 - r + c;  // the centre of the three edge pixels
                px(r, c) = avg3(e[i - 1], e[i], e[i + 1]);
            }
        break;
    case 6:  // VR
        px(3, 0) = avg3(L[2], L[1], L[0]);
        px(2, 0) = avg3(L[1], L[0], P);
        px(3, 1) = px(1, 0) = avg3(L[0], P, A[0]);
        px(2, 1) = px(0, 0) = avg2(P, A[0]);
        px(3, 2) = px(1, 1) = avg3(P, A[0], A[1]);
        px(2, 2) = px(0, 1) = avg2(A[0], A[1]);
        px(3, 3) = px(1, 2) = avg3(A[0], A[1], A[2]);
        px(2, 3) = px(0, 2) = avg2(A[1], A[2]);
        px(1, 3) = avg3(A[1], A[2], A[3]);
        px(0, 3) = avg2(A[2], A[3]);
        break;
    case 7:  // VL
        px(0, 0) = avg2(A[0], A[1]);
        px(1, 0) = avg3(A[0], A[1], A[2]);
        px(2, 0) = px(0, 1) = avg2(A[1], A[2]);
        px(1, 1) = px(3, 0) = avg3(A[1], A[2], A[3]);
        px(2, 1) = px(0, 2) = avg2(A[2], A[3]);
        px(3, 1) = px(1, 2) = avg3(A[2], A[3], A[4]);
        px(2, 2) = px(0, 3) = avg2(A[3], A[4]);
        px(3, 2) = px(1, 3) = avg3(A[3], A[4], A[5]);
        px(2, 3) = avg3(A[4], A[5], A[6]);
        px(3, 3) = avg3(A[5], A[6], A[7]);
        break;
    case 8:  // HD
        px(3, 0) = avg2(L[3], L[2]);
        px(3, 1) = avg3(L[3], L[2], L[1]);
        px(2, 0) = px(3, 2) = avg2(L[2], L[1]);
        px(2, 1) = px(3, 3) = avg3(L[2], L[1], L[0]);
        px(2, 2) = px(1, 0) = avg2(L[1], L[0]);
        px(2, 3) = px(1, 1) = avg3(L[1], L[0], P);
        px(1, 2) = px(0, 0) = avg2(L[0], P);
        px(1, 3) = px(0, 1) = avg3(L[0], P, A[0]);
        px(0, 2) = avg3(P, A[0], A[1]);
        px(0, 3) = avg3(A[0], A[1], A[2]);
        break;
    default:  // HU
        px(0, 0) = avg2(L[0], L[1]);
        px(0, 1) = avg3(L[0], L[1], L[2]);
        px(0, 2) = px(1, 0) = avg2(L[1], L[2]);
        px(0, 3) = px(1, 1) = avg3(L[1], L[2], L[3]);
        px(1, 2) = px(2, 0) = avg2(L[2], L[3]);
        px(1, 3) = px(2, 1) = avg3(L[2], L[3], L[3]);
        px(2, 2) = px(2, 3) = px(3, 0) = px(3, 1) = px(3, 2) = px(3, 3) = L[3];
        break;
    }
}

// ---- the value vector, lane by lane ----
static long n_vectors = 0, n_tm_low = 0, n_tm_high = 0, n_tm_in = 0;
static void check_values(const int* E)
{
    int V[64];
    int dsum = 0;
    for (int l = 0; l < 64; l++) {
        const I4PValue m = i4p_value_map(l);
        CHECK(m.ka >= 0 && m.ka < 13 && m.kb >= 0 && m.kb < 13 && m.kc >= 0 && m.kc < 13, "lane %d reads E[%d], E[%d], E[%d]",
              l, m.ka, m.kb, m.kc);
        CHECK(m.sh >= 0 && m.sh <= 2, "lane %d shift %d", l, m.sh);
        const int ea = E[m.ka % 13], eb = E[m.kb % 13], ec = E[m.kc % 13];
        V[l] = i4p_value(m, ea, eb, ec);
        CHECK(V[l] >= 0 && V[l] <= 255, "lane %d value %d is no byte", l, V[l]);
        const int raw = (ea + m.wb * eb + m.wc * ec + ((1 << m.sh) >> 1)) >> m.sh;
        if (l < ZW_I4P_V_TM) CHECK(V[l] == raw, "lane %d: the clamp changed %d", l, raw);
        else if (l < ZW_I4P_NV) (raw < 0 ? n_tm_low : raw > 255 ? n_tm_high : n_tm_in)++;
        if (i4p_value_dc_term(l)) dsum += ea;
    }
    V[ZW_I4P_V_DC] = (dsum + 4) >> 3;
    for (int mode = 0; mode < 10; mode++) {
        int want[16];
        predict(mode, E, want);
        for (int p = 0; p < 16; p++) {
            const int vi = i4p_vindex(kIdx[mode][p], p);
            CHECK(vi >= 0 && vi < ZW_I4P_NV && 4 * vi < 256, "mode %d pixel %d reads entry %d", mode, p, vi);
#if ZW_I4P_TMV
            const int got = V[vi & 63];
#else
            const int got = mode == 1 ? clip(V[vi & 63] + V[5 + (p & 3)] - V[4]) : V[vi & 63];
#endif
            CHECK(got == want[p], "mode %d pixel %d: %d, the predictor gives %d", mode, p, got, want[p]);
        }
    }
    n_vectors++;
}

static void walk_values()
{
    int E[13];
    for (int v = 0; v <= 255; v += 255) {
        for (int i = 0; i < 13; i++) E[i] = v;
        check_values(E);
    }
    for (int period = 1; period <= 2; period++)
        for (int phase = 0; phase < 2 * period; phase++) {
            for (int i = 0; i < 13; i++) E[i] = (((i + phase) / period) & 1) * 255;
            check_values(E);
        }
    const int base[3] = {0, 255, 128};
    for (int b = 0; b < 3; b++)
        for (int pos = 0; pos < 13; pos++)
            for (int s = 0; s <= 255; s += 255) {
                for (int i = 0; i < 13; i++) E[i] = base[b];
                E[pos] = s;
                check_values(E);
            }
    // the three parts of the edge at opposite ends: L, P, A each 0 or 255
    for (int c = 0; c < 8; c++) {
        for (int i = 0; i < 13; i++) E[i] = ((c >> (i < 4 ? 0 : (i == 4 ? 1 : 2))) & 1) * 255;
        check_values(E);
    }
    for (int t = 0; t < 20000; t++) {
        const int kind = t % 3;
        for (int i = 0; i < 13; i++) {
            const int r = (int)(rnd() & 255);
            E[i] = kind == 0 ? r : (kind == 1 ? ((rnd() & 1) ? r & 15 : 255 - (r & 15)) : ((rnd() & 3) ? r : (int)(rnd() & 1) * 255));
        }
        check_values(E);
    }
#if ZW_I4P_TMV
    CHECK(n_tm_low > 1000 && n_tm_high > 1000 && n_tm_in > 1000, "TrueMotion below / above / within 0..255: %ld / %ld / %ld",
          n_tm_low, n_tm_high, n_tm_in);
#endif
}

// ---- the ranking key ----
static long n_blocks = 0, n_ties = 0;
static void ranks_of(const uint32_t* key, int* rank)
{
    for (int m = 0; m < 10; m++) {
        rank[m] = 0;
        for (int o = 0; o < 10; o++) rank[m] += (int)(key[o] < key[m]);
    }
}
static void check_keys(const uint8_t* s, const uint8_t (*p)[16])
{
    uint32_t exact[10], key[10];
    for (int m = 0; m < 10; m++) {
        uint32_t sse = 0, pp = 0, sp = 0;
        // (as the lanes do: four rows of four bytes, two byte dot products each)
        for (int r = 0; r < 4; r++)
            for (int j = 0; j < 4; j++) {
                const int a = s[4 * r + j], b = p[m][4 * r + j];
                sse += (uint32_t)((a - b) * (a - b));
                pp += (uint32_t)(b * b);
                sp += (uint32_t)(a * b);
            }
        exact[m] = (sse << 4) | (uint32_t)m;
        key[m] = i4p_rank_key(pp, sp, m);
        CHECK(key[m] > 0 && key[m] < (1u << 27), "mode %d key %u out of bounds", m, key[m]);
        CHECK((key[m] & 15u) == (uint32_t)m, "mode %d in the key's low bits", m);
    }
    int r0[10], r1[10];
    ranks_of(exact, r0);
    ranks_of(key, r1);
    for (int m = 0; m < 10; m++) CHECK(r0[m] == r1[m], "mode %d: rank %d by the key, %d by the SSE", m, r1[m], r0[m]);
    for (int m = 1; m < 10; m++) n_ties += (int)((exact[m] >> 4) == (exact[0] >> 4));
    n_blocks++;
}

static void walk_keys()
{
    uint8_t s[16], p[10][16];
    // extremes: sources and predictions all 0 or all 255, every mode either
    for (int sv = 0; sv <= 255; sv += 255)
        for (int mask = 0; mask < 1024; mask++) {
            std::memset(s, sv, 16);
            for (int m = 0; m < 10; m++) std::memset(p[m], ((mask >> m) & 1) * 255, 16);
            check_keys(s, p);
        }
    for (int t = 0; t < 60000; t++) {
        const int kind = t % 6;
        for (int i = 0; i < 16; i++) s[i] = kind == 1 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)rnd();
        for (int m = 0; m < 10; m++)
            for (int i = 0; i < 16; i++)
                p[m][i] = kind == 1 ? (uint8_t)((rnd() & 1) * 255) : (kind == 2 ? (uint8_t)(s[i] + (int)(rnd() % 5) - 2) : (uint8_t)rnd());
        if (kind >= 3) {
            // ties: nt modes share one prediction (equal SSE exactly), or mirror the
            // source (s + d and s - d: equal SSE, unlike pp and sp)
            const int nt = kind == 3 ? 2 : (kind == 4 ? 4 : 10);
            int first = (int)(rnd() % 10);
            for (int k = 1; k < nt; k++) {
                const int m = (first + k * 3) % 10;  // (3 and 10 coprime: distinct modes)
                if (t & 8) {
                    for (int i = 0; i < 16; i++) {
                        const int d = (int)p[first][i] - (int)s[i], v = (int)s[i] - d;
                        p[m][i] = (uint8_t)(v < 0 || v > 255 ? p[first][i] : v);
                    }
                } else {
                    std::memcpy(p[m], p[first], 16);
                }
            }
        }
        check_keys(s, p);
    }
    CHECK(n_ties > 10000, "ties with mode 0: %ld", n_ties);
}

// ---- the byte packing of the gathered words ----
// v_perm_b32(a, b, sel): result byte i is byte n = sel byte i of the eight bytes b (0..3), a (4..7); 0x0c gives 0
static uint32_t v_perm(uint32_t a, uint32_t b, uint32_t sel)
{
    const uint64_t ab = ((uint64_t)a << 32) | b;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t n = (sel >> (8 * i)) & 255u;
        CHECK(n < 8 || n == 0x0c, "selector byte %u", n);
        if (n < 8) r |= (uint32_t)((ab >> (8 * n)) & 255u) << (8 * i);
    }
    return r;
}
static long n_rows = 0;
static void walk_packing()
{
    for (int t = 0; t < 4000; t++) {
        uint32_t v[4];
        for (int j = 0; j < 4; j++) v[j] = (t & 1) ? rnd() * 2u + (rnd() & 1u) : ((rnd() & 1) ? 0xffffffffu : 0u) ^ (0xffu << (8 * (rnd() & 3)));
        for (int g = 0; g < 4; g++) {
            const int hm = g >> 1, slot = g & 1;
            uint32_t want = 0;
            for (int j = 0; j < 4; j++) want |= ((v[j] >> (8 * g)) & 255u) << (8 * j);
            // the ranking's row, straight from the gathered words
            const uint32_t bsel = i4p_bsel(hm, slot);
            const uint32_t row = i4p_pack_row(v_perm(v[1], v[0], bsel), v_perm(v[3], v[2], bsel));
            CHECK(row == want, "group %d: packed row %08x, not %08x", g, row, want);
            // the 16-bit pairs (x0, x1), (x3, x2) and the row from them
            const uint32_t psel = i4p_psel(hm, slot);
            const uint32_t p01 = v_perm(v[1], v[0], psel), p32 = v_perm(v[2], v[3], psel);
            CHECK(p01 == ((want & 255u) | (((want >> 8) & 255u) << 16)), "group %d: pair (x0, x1) %08x", g, p01);
            CHECK(p32 == ((want >> 24) | (((want >> 16) & 255u) << 16)), "group %d: pair (x3, x2) %08x", g, p32);
            CHECK(v_perm(p32, p01, ZW_I4P_PAIRS_TO_ROW) == want, "group %d: row from the pairs", g);
            n_rows++;
        }
    }
}

int main()
{
    walk_values();
    walk_packing();
    walk_keys();
    if (bad) {
        std::printf("FAILED: %d checks\n", bad);
        return 1;
    }
    std::printf("ok: %ld edge vectors (TrueMotion below / above / within 0..255: %ld / %ld / %ld), %ld packed rows, %ld blocks' keys (%ld ties)\n",
                n_vectors, n_tm_low, n_tm_high, n_tm_in, n_rows, n_blocks, n_ties);
    return 0;
}
