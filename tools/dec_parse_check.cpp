// dec_parse_check.cpp -- the decoder's parser of untrusted bytes
// (csrc/zw_dec_parse.cpp) on the CPU, meant to run under sanitizers: every
// .vp8 file given parses (header, modes, MB records into a worst-case buffer)
// and the CPU replay of the device token parse reproduces its records; then
// damaged variants of it (prefixes, flipped bytes) either fail with an error
// code or parse, and where both the parser and the replay succeed they agree.
// Prints "ok <files> <variants>" and exits 0 when all hold.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I image-webp_amd/csrc tools/dec_parse_check.cpp image-webp_amd/csrc/zw_dec_parse.cpp
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/zwebp.h"
#include "zw_dec_parse.h"

using namespace zwdec;

static int fail(const char* file, const char* variant, long k, const char* what, int a, int b)
{
    printf("FAILED: %s (%s %ld): %s (%d, %d)\n", file, variant, k, what, a, b);
    return 1;
}

// The flips' generator (xorshift64*, seeded per file: the variants are the same on every run).
struct Rng {
    uint64_t state;
    uint32_t operator()()
    {
        state ^= state >> 12;
        state ^= state << 25;
        state ^= state >> 27;
        return (uint32_t)((state * 0x2545F4914F6CDD1Dull) >> 32);
    }
};

struct Result {
    int rc = ZW_OK;       // parse_header, then parse_modes / parse_mbs (the records' code wins)
    int replay_rc = ZW_OK, match = -1;  // zw_dbg_tokl_frame
    bool replayable = false;            // one token partition, two or more MB columns
};

// One stream through the parser and the replay.  The bytes are copied into a
// buffer of exactly their length, so a read past the end is a sanitizer error.
static Result run(const uint8_t* bytes, size_t len)
{
    Result R;
    std::vector<uint8_t> s(bytes, bytes + len);
    DecFrame A, B;  // (parse_mbs and parse_modes each consume the first partition's reader)
    R.rc = parse_header(A, s.data(), len);
    if (R.rc == ZW_OK) {
        (void)parse_header(B, s.data(), len);
        const size_t nmb = (size_t)A.mbw * A.mbh;
        if (nmb == 0) {
            R.rc = ZW_EINVALID_DIMENSIONS;
        } else {
            std::vector<uint8_t> modes(nmb * ZW_TOK_MODE), recs(nmb * ZW_DREC_MAX);
            std::vector<uint32_t> moff(nmb + 1);
            const int rm = parse_modes(B, modes.data());
            R.rc = parse_mbs(A, recs.data(), moff.data());
            if (R.rc == ZW_OK && rm != ZW_OK) R.rc = rm;  // (the modes are a prefix of the records' decisions)
            R.replayable = A.nparts == 1 && A.mbw >= 2;
        }
    }
    R.replay_rc = zw_dbg_tokl_frame(s.data(), len, &R.match);
    return R;
}

static int check_damaged(const char* file, const char* variant, long k, const uint8_t* bytes, size_t len)
{
    const Result R = run(bytes, len);
    if (R.replay_rc != R.rc) return fail(file, variant, k, "the replay's parse code differs from the parser's", R.replay_rc, R.rc);
    if (R.rc == ZW_OK && R.match == 0) return fail(file, variant, k, "parser and replay both succeed and differ", R.rc, R.match);
    return 0;
}

// One file and its damaged variants; returns nonzero on a failure, else adds to *variants.
static int check_file(const char* file, int index, long* variants)
{
    std::vector<uint8_t> s;
    {
        FILE* f = fopen(file, "rb");
        if (!f) return fail(file, "open", 0, "cannot read", 0, 0);
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + n);
        fclose(f);
    }
    const size_t len = s.size();
    // as it is: parses, and the replay writes the same records (it declines
    // frames of several token partitions or one MB column: match -1)
    const Result R = run(s.data(), len);
    if (R.rc != ZW_OK || R.replay_rc != ZW_OK) return fail(file, "undamaged", 0, "does not parse", R.rc, R.replay_rc);
    if (R.match != (R.replayable ? 1 : -1)) return fail(file, "undamaged", 0, "replay mismatch", R.match, R.replayable);
    // every prefix of 0..12 bytes, then 24 evenly spaced over the rest
    for (size_t n = 0; n <= 12 && n <= len; n++, ++*variants)
        if (check_damaged(file, "prefix", (long)n, s.data(), n)) return 1;
    if (len > 12)
        for (size_t k = 1; k <= 24; k++, ++*variants) {
            const size_t n = 12 + (len - 12) * k / 25;
            if (check_damaged(file, "prefix", (long)n, s.data(), n)) return 1;
        }
    // 48 copies with one to three bytes flipped at positions of 10 or more
    Rng rng{0x9E3779B97F4A7C15ull + (uint64_t)index};
    if (len > 10)
        for (int k = 0; k < 48; k++, ++*variants) {
            std::vector<uint8_t> d = s;
            const int flips = 1 + (int)(rng() % 3);
            for (int j = 0; j < flips; j++) d[10 + rng() % (len - 10)] ^= (uint8_t)(1 + rng() % 255);
            if (check_damaged(file, "flip", k, d.data(), len)) return 1;
        }
    return 0;
}

// The files are independent: a few threads share them (the replay of a large
// frame under the sanitizers takes seconds).
int main(int argc, char** argv)
{
    const int nfiles = argc - 1;
    std::vector<long> variants(nfiles, 0);
    std::vector<int> bad(nfiles, 0);
    std::atomic<int> next(0);
    std::vector<std::thread> th;
    const int nt = std::max(1, std::min(nfiles, (int)std::min(8u, std::thread::hardware_concurrency())));
    for (int t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (int i; (i = next.fetch_add(1)) < nfiles;) bad[i] = check_file(argv[1 + i], i, &variants[i]);
        });
    for (auto& t : th) t.join();
    long total = 0;
    for (int i = 0; i < nfiles; i++) {
        if (bad[i]) return 1;
        total += variants[i];
    }
    printf("ok %d %ld\n", nfiles, total);
    return 0;
}
