// Host check of the encoder's device-tensor input (image-webp_amd/csrc/zw_ingest.h):
// the pixel rule, the vector-run predicate and the argument check.
//
// On the device a wrong rule is a wrong bitstream, and a wrong predicate or
// argument check is a load outside the caller's tensor.  So all three are
// walked here, where nothing can go out of range:
//   - the rule, for all 65 536 f16 bit patterns under several (scale, bias)
//     pairs, against an independent statement in double precision (the f16
//     value by ldexp, the product and the sum each rounded to f32 once, the
//     tie broken by the parity of the floor); and for f32 values around every
//     k + 0.5 tie (the tie, its two neighbours in f32, k +- 0.49), the clamps,
//     NaN, +-inf and denormals;
//   - the predicate: for widths 1..40, every layout x dtype x channels, base
//     offsets and strides that keep or break each alignment, every vector load
//     of every run of a tensor ing_vec_ok accepts is aligned to its size and
//     stays inside the row's own w*channels (HWC) or w (CHW) elements; and a
//     tensor it refuses does have a misaligned load (it refuses nothing else);
//   - the argument check: ing_span's *need equals the last addressed element
//     + 1 by the addressing formula for packed and padded strides, it refuses
//     each stride one below its bound and frames that overlap by one element,
//     and a capacity one short is below *need.
// With arguments `rule SCALE_BITS BIAS_BITS` it reads f32 bit patterns (decimal,
// one a line) from stdin and prints the rule's byte of each;
// tests/test_ingest_check.py pins those against numpy's float32 arithmetic, the
// statement the GPU tests take their expected images from.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I image-webp_amd/csrc tools/ingest_check.cpp -o ingest_check && ./ingest_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "zw_ingest.h"

static int bad = 0;
#define FAIL(...)                                   \
    do {                                            \
        if (bad++ < 20) std::printf(__VA_ARGS__);   \
    } while (0)

// ---- the rule, stated independently in double precision ----
static int rule_ref(double x, float scale, float bias)
{
    if (std::isnan(x)) return 0;
    // f32 x f32 is exact in double, and so is the sum of two f32 unless their
    // exponents are > 2^29 apart, where the double sum already rounds the way the
    // f32 sum does: one rounding to f32 each
    const float m = (float)(x * (double)scale);
    const float t = (float)((double)m + (double)bias);
    if (std::isnan(t)) return 0;
    double c = (double)t;
    if (c < 0.0) c = 0.0;
    if (c > 255.0) c = 255.0;
    const double fl = std::floor(c), fr = c - fl;
    int v = (int)fl;
    if (fr > 0.5 || (fr == 0.5 && (v & 1))) v++;
    return v;
}

static double f16_value(uint16_t hb)
{
    const int e = (hb >> 10) & 31, m = hb & 1023;
    double v;
    if (e == 31) v = m ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
    else if (e == 0) v = std::ldexp((double)m, -24);
    else v = std::ldexp((double)(1024 + m), e - 25);
    return (hb & 0x8000) ? -v : v;
}

static void check_rule()
{
    static const float SB[][2] = {{1.0f, 0.0f},        {255.0f, 0.0f},          {255.0f, 0.5f},  {1.0f / 0.229f, 123.675f},
                                  {58.395f, 103.53f},  {-255.0f, 255.0f},       {0.5f, 0.25f},   {1e-3f, 0.5f},
                                  {3.0e38f, -1.0f},    {127.5f, 127.5f}};
    for (const auto& sb : SB) {
        for (uint32_t hb = 0; hb < 65536; hb++) {
            const double x = f16_value((uint16_t)hb);
            const float xf = ing_f16_bits_to_f32((uint16_t)hb);
            if (std::isnan(x) ? !std::isnan(xf) : !((double)xf == x && std::signbit(xf) == std::signbit(x)))
                FAIL("f16 %04x: converts to %a, not %a\n", hb, (double)xf, x);
            const int got = ing_byte_f16((uint16_t)hb, sb[0], sb[1]), want = rule_ref(x, sb[0], sb[1]);
            if (got != want) FAIL("f16 %04x scale %a bias %a: %d, want %d\n", hb, sb[0], sb[1], got, want);
        }
    }
    // f32: around every tie, the clamps and the specials
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long n = 0;
    auto one = [&](float x, float s, float b) {
        const int got = ing_byte_f32(x, s, b), want = rule_ref((double)x, s, b);
        if (got != want) FAIL("f32 %a scale %a bias %a: %d, want %d\n", (double)x, (double)s, (double)b, got, want);
        n++;
    };
    for (int k = -2; k <= 257; k++) {
        const float tie = (float)k + 0.5f;
        const float xs[] = {tie, std::nextafterf(tie, inf), std::nextafterf(tie, -inf), (float)k + 0.49f,
                            (float)k - 0.49f, (float)k, (float)k + 0.51f};
        for (float x : xs) {
            one(x, 1.0f, 0.0f);
            one(x / 255.0f, 255.0f, 0.0f);
            one(x - 3.0f, 1.0f, 3.0f);
            one(x * 2.0f, 0.5f, 0.0f);
            one(x, 1.0f / 0.229f, -0.485f / 0.229f);
        }
    }
    const float specials[] = {nan, -nan, inf, -inf, 0.0f, -0.0f, 1e-45f, -1e-45f, 1.17549435e-38f, 3.4e38f, -3.4e38f,
                              254.5f, 255.0f, 255.5f, 256.0f, -0.5f, -0.25f, 0.5f, 1.5f, 2.5f, 1e9f, -1e9f};
    for (float x : specials)
        for (const auto& sb : SB) {
            one(x, sb[0], sb[1]);
            one(x, sb[0], inf);   // inf + -inf = NaN -> 0
            one(x, sb[0], -inf);
            one(x, sb[0], nan);
            one(x, 0.0f, sb[1]);  // inf * 0 = NaN -> 0
        }
    if (n < 9000) FAIL("f32 sample too small: %ld\n", n);
}

// ---- the predicate ----
static size_t elem_of(int layout, size_t ch, size_t fs, size_t ps, size_t rs, size_t i, size_t c, size_t y, size_t x)
{
    return layout == ZW_ING_CHW ? i * fs + c * ps + y * rs + x : i * fs + y * rs + x * ch + c;
}

static void check_predicate()
{
    long accepted = 0, refused = 0;
    for (int layout = 0; layout < 2; layout++)
        for (int dtype = 0; dtype < 3; dtype++)
            for (int ch = 3; ch <= 4; ch++) {
                const size_t es = (size_t)ing_elsize(dtype), piece = (size_t)ing_piece_bytes(layout, dtype, ch);
                const int np = ing_pieces(layout, dtype, ch);
                if ((size_t)np * piece != (layout == ZW_ING_CHW ? 8 : 8 * (size_t)ch) * es)
                    FAIL("layout %d dtype %d ch %d: %d pieces of %zu bytes do not make a run\n", layout, dtype, ch, np, piece);
                for (int w = 1; w <= 40; w++) {
                    const size_t h = 3, n = 2;
                    const size_t row0 = layout == ZW_ING_CHW ? (size_t)w : (size_t)w * ch;
                    // row / plane / frame padding and the base offset, in elements: 0 and values that
                    // break or keep each alignment
                    static const size_t PADS[] = {0, 1, 2, 3, 4, 5, 8, 16};
                    for (size_t rp : PADS)
                        for (size_t pp : PADS)
                            for (size_t fp : {(size_t)0, (size_t)1, (size_t)4, (size_t)16})
                                for (size_t off : {(size_t)0, (size_t)1, (size_t)2, (size_t)4, (size_t)8, (size_t)16}) {
                                    if (layout == ZW_ING_HWC && pp) continue;
                                    const size_t rs = row0 + rp;
                                    const size_t ps = layout == ZW_ING_CHW ? rs * h + pp : 0;
                                    const size_t fs = (layout == ZW_ING_CHW ? ps * ch : rs * h) + fp;
                                    const uintptr_t base = 4096 + off * es;  // (a 4096-aligned allocation)
                                    const bool ok = ing_vec_ok(layout, dtype, ch, base, fs, ps, rs);
                                    bool misaligned = false;
                                    for (size_t i = 0; i < n; i++)
                                        for (size_t y = 0; y < h; y++)
                                            for (size_t g = 0; ing_run_in_row((int)(8 * g), w); g++)
                                                for (size_t c = 0; c < (layout == ZW_ING_CHW ? 3u : 1u); c++) {
                                                    const size_t row = elem_of(layout, ch, fs, ps, rs, i, c, y, 0);
                                                    const size_t first = row + ing_run_first(layout, ch, g);
                                                    for (int q = 0; q < np; q++) {
                                                        const size_t b0 = first * es + (size_t)q * piece, b1 = b0 + piece;
                                                        if ((base + b0) % piece) misaligned = true;
                                                        // the row's own elements
                                                        if (ok && (b0 < row * es || b1 > (row + row0) * es))
                                                            FAIL("layout %d dtype %d ch %d w %d: load [%zu, %zu) leaves row "
                                                                 "[%zu, %zu)\n", layout, dtype, ch, w, b0, b1, row * es,
                                                                 (row + row0) * es);
                                                    }
                                                }
                                    if (ok && misaligned)
                                        FAIL("layout %d dtype %d ch %d w %d rs %zu ps %zu fs %zu off %zu: accepted, misaligned\n",
                                             layout, dtype, ch, w, rs, ps, fs, off);
                                    // (widths below 8 have no vector run; two frames of three rows and three
                                    // planes exercise every stride otherwise)
                                    if (!ok && !misaligned && w >= 8)
                                        FAIL("layout %d dtype %d ch %d w %d rs %zu ps %zu fs %zu off %zu: refused, all aligned\n",
                                             layout, dtype, ch, w, rs, ps, fs, off);
                                    ok ? accepted++ : refused++;
                                }
                }
            }
    if (accepted < 1000 || refused < 1000) FAIL("predicate walk is lopsided: %ld accepted, %ld refused\n", accepted, refused);
}

// ---- the argument check ----
static void check_span()
{
    long cases = 0;
    for (int layout = 0; layout < 2; layout++)
        for (size_t ch = 3; ch <= 4; ch++)
            for (size_t n : {(size_t)1, (size_t)2, (size_t)5})
                for (size_t w : {(size_t)1, (size_t)7, (size_t)37, (size_t)40})
                    for (size_t h : {(size_t)1, (size_t)2, (size_t)21})
                        for (size_t rp : {(size_t)0, (size_t)3})
                            for (size_t pp : {(size_t)0, (size_t)7})
                                for (size_t fp : {(size_t)0, (size_t)11}) {
                                    const bool chw = layout == ZW_ING_CHW;
                                    const size_t rs = (chw ? w : w * ch) + rp;
                                    const size_t ps = chw ? (h - 1) * rs + w + pp : 0;
                                    const size_t one = chw ? (ch - 1) * ps + (h - 1) * rs + w : (h - 1) * rs + w * ch;
                                    const size_t fs = one + fp;
                                    // the formula of tests/test_gpu_dec_device.py's span()
                                    const size_t want = (n - 1) * fs + one;
                                    // ... which is the last addressed element + 1
                                    if (elem_of(layout, ch, fs, ps, rs, n - 1, ch - 1, h - 1, w - 1) + 1 != want)
                                        FAIL("span formula != last element + 1\n");
                                    size_t need = 0;
                                    if (!ing_span(layout, n, w, h, ch, fs, ps, rs, &need) || need != want)
                                        FAIL("layout %d n %zu %zux%zu ch %zu: need %zu, want %zu\n", layout, n, w, h, ch, need, want);
                                    // a capacity one short must fail the caller's `capacity < need`
                                    if (!(want - 1 < need)) FAIL("one element short passes\n");
                                    size_t t;
                                    if (ing_span(layout, n, w, h, ch, fs, ps, rs - rp - 1, &t)) FAIL("row stride one short accepted\n");
                                    if (chw && ing_span(layout, n, w, h, ch, fs, ps - pp - 1, rs, &t))
                                        FAIL("plane stride one short accepted\n");
                                    if (n > 1 && ing_span(layout, n, w, h, ch, fs - fp - 1, ps, rs, &t))
                                        FAIL("overlapping frames accepted\n");
                                    if (n == 1 && (!ing_span(layout, n, w, h, ch, 0, ps, rs, &t) || t != want))
                                        FAIL("one frame: frame_stride must not matter\n");
                                    cases++;
                                }
    size_t t;
    const size_t big = (size_t)-1 / 2;
    if (ing_span(ZW_ING_HWC, 3, 40, 24, 3, big, 0, 120, &t)) FAIL("overflowing frame stride accepted\n");
    if (ing_span(ZW_ING_CHW, 1, 40, 24, 3, 0, big, 40, &t)) FAIL("overflowing plane stride accepted\n");
    if (ing_span(ZW_ING_HWC, 1, 40, 24, 3, 0, 0, big, &t)) FAIL("overflowing row stride accepted\n");
    if (ing_span(2, 1, 40, 24, 3, 2880, 0, 120, &t)) FAIL("layout 2 accepted\n");
    if (ing_span(ZW_ING_HWC, 0, 40, 24, 3, 2880, 0, 120, &t)) FAIL("no frames accepted\n");
    if (cases < 1000) FAIL("span walk too small\n");
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "rule")) {  // rule SCALE_BITS BIAS_BITS: f32 bit patterns on stdin -> bytes
        const uint32_t sb = (uint32_t)std::strtoul(argv[2], nullptr, 10), bb = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        float s, b, x;
        std::memcpy(&s, &sb, 4);
        std::memcpy(&b, &bb, 4);
        unsigned long xb;
        while (std::scanf("%lu", &xb) == 1) {
            const uint32_t x32 = (uint32_t)xb;
            std::memcpy(&x, &x32, 4);
            std::printf("%d\n", (int)ing_byte_f32(x, s, b));
        }
        return 0;
    }
    check_rule();
    check_predicate();
    check_span();
    if (bad) {
        std::printf("FAILED: %d\n", bad);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
