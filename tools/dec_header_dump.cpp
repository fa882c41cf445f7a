// dec_header_dump.cpp -- what the decoder's CPU code (csrc/zw_dec_parse.cpp)
// makes of a key frame, as plain numbers for tests/test_synth_streams.py and
// tests/test_wide_coeffs.py: the header fields, the per-segment dequantisers, the loop filter's table (built
// from the header the way the decode paths build it) and, per macroblock, the
// modes and levels of the packed records.  One "frame" line, one "probs" line
// and one "mb" line per macroblock for each .vp8 file given.
//   g++ -O1 -std=c++17 -I image-webp_amd/csrc tools/dec_header_dump.cpp image-webp_amd/csrc/zw_dec_parse.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/zwebp.h"
#include "zw_dec_parse.h"

using namespace zwdec;

static int dump(const char* file)
{
    std::vector<uint8_t> s;
    FILE* f = fopen(file, "rb");
    if (!f) return 1;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + n);
    fclose(f);
    DecFrame F;
    int rc = parse_header(F, s.data(), s.size());
    if (rc != ZW_OK) return printf("error %d\n", rc), 1;
    ZwFilterParams fp;
    filter_table(fp, F.filter_type, F.filter_level, F.sharpness, F.segments_enabled, F.seg_delta_values, F.seg_lf,
                 F.lf_adj_enabled, F.ref_delta0, F.mode_delta0, F.mbw, F.mbh);
    printf("frame %d %d %d %d  %d %d %d  %d %d %d  %d %d %d  %d %d ", F.width, F.height, F.mbw, F.mbh, F.filter_type,
           F.filter_level, F.sharpness, F.segments_enabled, F.seg_update_map, F.seg_delta_values, F.lf_adj_enabled,
           F.ref_delta0, F.mode_delta0, F.nparts, F.skip_prob);
    for (int i = 0; i < 4; i++) printf(" %d", F.seg_quant[i]);
    for (int i = 0; i < 4; i++) printf(" %d", F.seg_lf[i]);
    for (int i = 0; i < 3; i++) printf(" %d", F.seg_probs[i]);
    for (int i = 0; i < 4; i++)
        printf(" %d %d %d %d %d %d", F.q[i].ydc, F.q[i].yac, F.q[i].y2dc, F.q[i].y2ac, F.q[i].uvdc, F.q[i].uvac);
    printf(" %d %d %d", fp.filter_type, fp.mbw, fp.mbh);
    for (int i = 0; i < 8; i++) printf(" %d", fp.level[i / 2][i % 2]);
    for (int i = 0; i < 8; i++) printf(" %d", fp.ilimit[i / 2][i % 2]);
    for (int i = 0; i < 8; i++) printf(" %d", fp.hev[i / 2][i % 2]);
    printf("\nprobs");
    for (size_t i = 0; i < sizeof F.probs; i++) printf(" %d", (&F.probs[0][0][0][0])[i]);
    printf("\n");
    const size_t nmb = (size_t)F.mbw * F.mbh;
    std::vector<uint8_t> recs(nmb * ZW_DREC_MAX);
    std::vector<uint32_t> moff(nmb + 1);
    rc = parse_mbs(F, recs.data(), moff.data());
    if (rc != ZW_OK) return printf("error %d\n", rc), 1;
    for (size_t m = 0; m < nmb; m++) {
        const uint8_t* rec = recs.data() + moff[m];
        uint16_t start[25];
        memcpy(start, rec + 16, sizeof start);
        const int16_t* lv = (const int16_t*)(rec + ZW_DREC_HDR);
        printf("mb %d %d %d %d ", rec[0] & 7, (rec[0] >> 3) & 3, (rec[0] >> 5) & 1, rec[1]);
        for (int i = 0; i < 16; i++) printf(" %d", (rec[8 + (i >> 1)] >> (4 * (i & 1))) & 15);
        // levels per block, 16 zigzag positions each: Y 0..15, U, V, then Y2
        for (int b = 0; b < 25; b++) {
            const int lo = b < 24 ? start[b] : 0, hi = b < 24 ? start[b + 1] : start[0];
            for (int n = 0; n < 16; n++) printf(" %d", n < hi - lo ? lv[lo + n] : 0);
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++)
        if (dump(argv[i])) return 1;
    return 0;
}
