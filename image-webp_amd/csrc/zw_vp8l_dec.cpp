// zw_vp8l_dec.cpp -- host reader of VP8L bitstreams (decoder/lossless.rs,
// decoder/huffman.rs, decoder/lossless_transform.rs of the reference) and of
// the ALPH chunk (read_alpha_chunk, decoder/extended.rs:273-334).  Plain C++.
//
// The input is untrusted: every read of the bitstream is bounds-checked (a read
// past the end is ZW_EBITSTREAM, as BitReader::consume), every table index is
// below its table's size by construction or by a check, back-references stay
// inside the pixels already decoded, and sub-image sizes follow from dimensions
// of at most 16384.  A failed allocation is ZW_ENOMEM.
#include "zw_vp8l_dec.h"

#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/zwebp.h"

namespace zwvp8l {
namespace {

// CODE_LENGTH_CODE_ORDER, DISTANCE_MAP, ALPHABET_SIZE (lossless.rs:20-54)
const uint8_t CODE_LENGTH_CODE_ORDER[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
const int8_t DISTANCE_MAP[120][2] = {
    {0, 1},  {1, 0},  {1, 1},  {-1, 1}, {0, 2},  {2, 0},  {1, 2},  {-1, 2}, {2, 1},  {-2, 1}, {2, 2},  {-2, 2},
    {0, 3},  {3, 0},  {1, 3},  {-1, 3}, {3, 1},  {-3, 1}, {2, 3},  {-2, 3}, {3, 2},  {-3, 2}, {0, 4},  {4, 0},
    {1, 4},  {-1, 4}, {4, 1},  {-4, 1}, {3, 3},  {-3, 3}, {2, 4},  {-2, 4}, {4, 2},  {-4, 2}, {0, 5},  {3, 4},
    {-3, 4}, {4, 3},  {-4, 3}, {5, 0},  {1, 5},  {-1, 5}, {5, 1},  {-5, 1}, {2, 5},  {-2, 5}, {5, 2},  {-5, 2},
    {4, 4},  {-4, 4}, {3, 5},  {-3, 5}, {5, 3},  {-5, 3}, {0, 6},  {6, 0},  {1, 6},  {-1, 6}, {6, 1},  {-6, 1},
    {2, 6},  {-2, 6}, {6, 2},  {-6, 2}, {4, 5},  {-4, 5}, {5, 4},  {-5, 4}, {3, 6},  {-3, 6}, {6, 3},  {-6, 3},
    {0, 7},  {7, 0},  {1, 7},  {-1, 7}, {5, 5},  {-5, 5}, {7, 1},  {-7, 1}, {4, 6},  {-4, 6}, {6, 4},  {-6, 4},
    {2, 7},  {-2, 7}, {7, 2},  {-7, 2}, {3, 7},  {-3, 7}, {7, 3},  {-7, 3}, {5, 6},  {-5, 6}, {6, 5},  {-6, 5},
    {8, 0},  {4, 7},  {-4, 7}, {7, 4},  {-7, 4}, {8, 1},  {8, 2},  {6, 6},  {-6, 6}, {8, 3},  {5, 7},  {-5, 7},
    {7, 5},  {-7, 5}, {8, 4},  {6, 7},  {-6, 7}, {7, 6},  {-7, 6}, {8, 5},  {7, 7},  {-7, 7}, {8, 6},  {8, 7}};
enum { GREEN = 0, RED = 1, BLUE = 2, ALPHA = 3, DIST = 4, CODES_PER_GROUP = 5 };
const uint16_t ALPHABET_SIZE[CODES_PER_GROUP] = {256 + 24, 256, 256, 256, 40};
const int MAX_CODE_LENGTH = 15, MAX_TABLE_BITS = 10;

// subsample_size (lossless.rs:57-61)
uint32_t subsample_size(uint32_t size, uint32_t bits) { return (size + (1u << bits) - 1) >> bits; }

// BitReader (lossless.rs:722-799): LSB first.  Bits past the end peek as zeros;
// taking more than the stream holds is the error.
struct BitReader {
    const uint8_t* d;
    size_t len, pos = 0;
    uint64_t buf = 0;
    unsigned nbits = 0;
    BitReader(const uint8_t* data, size_t n) : d(data), len(n) {}
    void fill()
    {
        while (nbits <= 56 && pos < len) {
            buf |= (uint64_t)d[pos++] << nbits;
            nbits += 8;
        }
    }
    // at least n (<= 32) bits in the buffer when the stream still has them
    void need(unsigned n)
    {
        if (nbits < n) fill();
    }
    uint32_t peek(unsigned n) const { return (uint32_t)(buf & (((uint64_t)1 << n) - 1)); }
    bool consume(unsigned n)
    {
        if (nbits < n) return false;
        buf >>= n;
        nbits -= n;
        return true;
    }
    // read_bits (lossless.rs:784-798), n <= 32
    bool read(unsigned n, uint32_t* v)
    {
        need(n);
        *v = peek(n);
        return consume(n);
    }
    size_t bits_left() const { return (len - pos) * 8 + nbits; }
};

// HuffmanTree (huffman.rs:10-253): a single symbol that takes no bits, or a
// complete prefix code.  Codes of up to MAX_TABLE_BITS bits resolve in one
// lookup of the next bits (entry = length << 12 | symbol); an entry of length
// 0 marks a longer code, which the canonical first-code walk resolves.
struct Huff {
    bool single = true;
    uint16_t symbol = 0;
    unsigned tbits = 0, maxlen = 0;
    std::vector<uint16_t> table, sorted;
    uint16_t count[MAX_CODE_LENGTH + 1] = {}, offset[MAX_CODE_LENGTH + 2] = {};

    void build_single(uint16_t s)  // build_single_node (huffman.rs:176-178)
    {
        single = true;
        symbol = s;
    }
    void build_two(uint16_t zero, uint16_t one)  // build_two_node (huffman.rs:180-186)
    {
        single = false;
        tbits = maxlen = 1;
        table.assign(2, 0);
        table[0] = (1u << 12) | zero;
        table[1] = (1u << 12) | one;
    }
    // build_implicit (huffman.rs:47-174); lengths[i] <= 15
    int build(const std::vector<uint16_t>& lengths)
    {
        int nsym = 0;
        memset(count, 0, sizeof count);
        for (uint16_t l : lengths) {
            if (l > MAX_CODE_LENGTH) return ZW_EHUFFMAN;
            count[l]++;
            if (l) nsym++;
        }
        if (nsym == 0) return ZW_EHUFFMAN;
        if (nsym == 1) {
            for (size_t i = 0; i < lengths.size(); i++)
                if (lengths[i]) build_single((uint16_t)i);
            return ZW_OK;
        }
        maxlen = MAX_CODE_LENGTH;
        while (maxlen > 1 && count[maxlen] == 0) maxlen--;
        uint32_t used = 0;
        for (unsigned l = 1; l <= maxlen; l++) used = (used << 1) + count[l];
        if (used != (1u << maxlen)) return ZW_EHUFFMAN;  // over- or under-subscribed
        single = false;
        count[0] = 0;
        offset[1] = 0;
        for (unsigned l = 1; l <= MAX_CODE_LENGTH; l++) offset[l + 1] = (uint16_t)(offset[l] + count[l]);
        sorted.assign((size_t)nsym, 0);
        {
            uint16_t next[MAX_CODE_LENGTH + 2];
            memcpy(next, offset, sizeof next);
            for (size_t i = 0; i < lengths.size(); i++)
                if (lengths[i]) sorted[next[lengths[i]]++] = (uint16_t)i;
        }
        tbits = maxlen < (unsigned)MAX_TABLE_BITS ? maxlen : (unsigned)MAX_TABLE_BITS;
        table.assign((size_t)1 << tbits, 0);
        uint32_t code = 0;  // canonical, MSB first
        for (unsigned l = 1; l <= tbits; l++) {
            for (unsigned k = 0; k < count[l]; k++, code++) {
                uint32_t rev = 0;
                for (unsigned b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
                const uint16_t e = (uint16_t)((l << 12) | sorted[offset[l] + k]);
                for (uint32_t i = rev; i < ((uint32_t)1 << tbits); i += (uint32_t)1 << l) table[i] = e;
            }
            code <<= 1;
        }
        return ZW_OK;
    }
    // read_symbol (huffman.rs:212-230)
    bool read(BitReader& br, uint16_t* out) const
    {
        if (single) {
            *out = symbol;
            return true;
        }
        br.need(MAX_CODE_LENGTH);
        const uint32_t v = br.peek(MAX_CODE_LENGTH);
        const uint16_t e = table[v & (((uint32_t)1 << tbits) - 1)];
        if (e >> 12) {
            *out = e & 0xfff;
            return br.consume(e >> 12);
        }
        uint32_t code = 0, first = 0;
        for (unsigned l = 1; l <= maxlen; l++) {
            code = (code << 1) | ((v >> (l - 1)) & 1u);
            if (code >= first && code - first < count[l]) {
                *out = sorted[offset[l] + (code - first)];
                return br.consume(l);
            }
            first = (first + count[l]) << 1;
        }
        return false;  // (a complete code always resolves)
    }
};

struct Group {
    Huff h[CODES_PER_GROUP];
};

// ColorCache (lossless.rs:699-719), pixels as the four bytes R, G, B, A
struct ColorCache {
    unsigned bits = 0;  // 0: none
    std::vector<uint32_t> c;
    void insert(uint32_t px)
    {
        const uint32_t r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255, a = px >> 24;
        const uint32_t argb = (a << 24) | (r << 16) | (g << 8) | b;
        c[(0x1e35a7bdu * argb) >> (32 - bits)] = px;
    }
};

// HuffmanInfo (lossless.rs:676-697)
struct HuffInfo {
    uint32_t xsize = 1, bits = 0, mask = ~0u;
    std::vector<uint16_t> image;
    std::vector<Group> groups;
    ColorCache cache;
    size_t index(uint32_t x, uint32_t y) const
    {
        return bits == 0 ? 0 : image[(size_t)(y >> bits) * xsize + (x >> bits)];
    }
};

uint32_t ld32(const uint8_t* p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
void st32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }

enum { T_PREDICTOR = 0, T_COLOR = 1, T_SUBTRACT_GREEN = 2, T_COLOR_INDEXING = 3 };
struct Transform {
    bool present = false;
    uint32_t size_bits = 0, table_size = 0;
    std::vector<uint8_t> data;
};

struct Decoder {
    BitReader br;
    uint32_t width = 0, height = 0;
    Transform tf[4];
    std::vector<uint8_t> order;
    Decoder(const uint8_t* d, size_t n) : br(d, n) {}

    // read_color_cache (lossless.rs:629-641)
    int read_color_cache(unsigned* bits)
    {
        uint32_t v;
        *bits = 0;
        if (!br.read(1, &v)) return ZW_EBITSTREAM;
        if (v) {
            if (!br.read(4, &v)) return ZW_EBITSTREAM;
            if (v < 1 || v > 11) return ZW_ECOLOR_CACHE_BITS;
            *bits = v;
        }
        return ZW_OK;
    }

    // read_huffman_code_lengths (lossless.rs:409-477)
    int read_code_lengths(const std::vector<uint16_t>& cl_lengths, uint32_t num_symbols, std::vector<uint16_t>& out)
    {
        Huff table;
        if (int r = table.build(cl_lengths)) return r;
        uint32_t v, max_symbol = num_symbols;
        if (!br.read(1, &v)) return ZW_EBITSTREAM;
        if (v) {
            if (!br.read(3, &v)) return ZW_EBITSTREAM;
            const unsigned length_nbits = 2 + 2 * v;
            if (!br.read(length_nbits, &v)) return ZW_EBITSTREAM;
            if (v > num_symbols - 2) return ZW_EBITSTREAM;
            max_symbol = 2 + v;
        }
        out.assign(num_symbols, 0);
        uint16_t prev = 8;
        uint32_t symbol = 0;
        while (symbol < num_symbols) {
            if (max_symbol == 0) break;
            max_symbol--;
            uint16_t len;
            if (!table.read(br, &len)) return ZW_EBITSTREAM;
            if (len < 16) {
                out[symbol++] = len;
                if (len) prev = len;
            } else {
                const unsigned slot = len - 16u;
                if (slot > 2) return ZW_EBITSTREAM;
                const unsigned extra = slot == 0 ? 2 : (slot == 1 ? 3 : 7), base = slot == 2 ? 11 : 3;
                if (!br.read(extra, &v)) return ZW_EBITSTREAM;
                const uint32_t repeat = v + base;
                if (symbol + repeat > num_symbols) return ZW_EBITSTREAM;
                const uint16_t fill = slot == 0 ? prev : 0;
                for (uint32_t i = 0; i < repeat; i++) out[symbol++] = fill;
            }
        }
        return ZW_OK;
    }

    // read_huffman_code (lossless.rs:370-406)
    int read_huffman_code(uint32_t alphabet, Huff& h)
    {
        uint32_t v;
        if (!br.read(1, &v)) return ZW_EBITSTREAM;
        if (v) {  // a simple code: one or two symbols
            uint32_t two, first8, zero, one;
            if (!br.read(1, &two) || !br.read(1, &first8) || !br.read(1 + 7 * first8, &zero)) return ZW_EBITSTREAM;
            if (zero >= alphabet) return ZW_EBITSTREAM;
            if (!two) {
                h.build_single((uint16_t)zero);
            } else {
                if (!br.read(8, &one)) return ZW_EBITSTREAM;
                if (one >= alphabet) return ZW_EBITSTREAM;
                h.build_two((uint16_t)zero, (uint16_t)one);
            }
            return ZW_OK;
        }
        std::vector<uint16_t> cl(19, 0), lengths;
        if (!br.read(4, &v)) return ZW_EBITSTREAM;
        const uint32_t n = 4 + v;
        for (uint32_t i = 0; i < n; i++) {
            if (!br.read(3, &v)) return ZW_EBITSTREAM;
            cl[CODE_LENGTH_CODE_ORDER[i]] = (uint16_t)v;
        }
        if (int r = read_code_lengths(cl, alphabet, lengths)) return r;
        return h.build(lengths);
    }

    // read_huffman_codes (lossless.rs:297-367)
    int read_huffman_codes(bool read_meta, uint32_t xsize, uint32_t ysize, unsigned cache_bits, HuffInfo& hi)
    {
        uint32_t v = 0, ngroups = 1;
        if (read_meta) {
            if (!br.read(1, &v)) return ZW_EBITSTREAM;
        }
        if (v) {  // the entropy image
            if (!br.read(3, &v)) return ZW_EBITSTREAM;
            hi.bits = v + 2;
            hi.xsize = subsample_size(xsize, hi.bits);
            const uint32_t hys = subsample_size(ysize, hi.bits);
            std::vector<uint8_t> data((size_t)hi.xsize * hys * 4);
            if (int r = decode_image_stream(hi.xsize, hys, false, data.data())) return r;
            hi.image.resize((size_t)hi.xsize * hys);
            for (size_t i = 0; i < hi.image.size(); i++) {
                const uint32_t code = ((uint32_t)data[i * 4] << 8) | data[i * 4 + 1];
                if (code >= ngroups) ngroups = code + 1;
                hi.image[i] = (uint16_t)code;
            }
            hi.mask = (1u << hi.bits) - 1;
        }
        // (every code takes at least one bit: a group count the stream cannot hold is refused before it is allocated)
        if ((size_t)ngroups * CODES_PER_GROUP > br.bits_left()) return ZW_EBITSTREAM;
        hi.groups.resize(ngroups);
        for (uint32_t g = 0; g < ngroups; g++)
            for (int j = 0; j < CODES_PER_GROUP; j++) {
                uint32_t alphabet = ALPHABET_SIZE[j];
                if (j == 0 && cache_bits) alphabet += 1u << cache_bits;
                if (int r = read_huffman_code(alphabet, hi.groups[g].h[j])) return r;
            }
        if (cache_bits) {
            hi.cache.bits = cache_bits;
            hi.cache.c.assign((size_t)1 << cache_bits, 0);
        }
        return ZW_OK;
    }

    // get_copy_distance (lossless.rs:644-658); prefix < 40
    bool copy_distance(uint32_t prefix, size_t* out)
    {
        if (prefix < 4) {
            *out = prefix + 1;
            return true;
        }
        const unsigned extra = (prefix - 2) >> 1;
        const size_t offset = (size_t)(2 + (prefix & 1)) << extra;
        uint32_t v;
        if (!br.read(extra, &v)) return false;
        *out = offset + v + 1;
        return true;
    }
    // plane_code_to_distance (lossless.rs:661-673); plane_code >= 1
    static size_t plane_distance(uint32_t xsize, size_t plane_code)
    {
        if (plane_code > 120) return plane_code - 120;
        const int64_t d = (int64_t)DISTANCE_MAP[plane_code - 1][0] + (int64_t)DISTANCE_MAP[plane_code - 1][1] * (int64_t)xsize;
        return d < 1 ? 1 : (size_t)d;
    }

    // decode_image_data (lossless.rs:480-626).  The reference's second cache
    // lookup (peek_symbol, :612-620) is the loop's next turn taken early.
    int decode_image_data(uint32_t w, uint32_t h, HuffInfo& hi, uint8_t* data)
    {
        const size_t num = (size_t)w * h;
        const Group* tree = &hi.groups[hi.index(0, 0)];
        size_t index = 0, next_block = 0;
        while (index < num) {
            if (index >= next_block) {
                const uint32_t x = (uint32_t)(index % w), y = (uint32_t)(index / w);
                const uint32_t xe = (x | hi.mask) < w - 1 ? (x | hi.mask) : w - 1;
                next_block = (size_t)xe + (size_t)y * w + 1;
                tree = &hi.groups[hi.index(x, y)];
                // codes of one symbol each take no bits: the block is one colour
                if (tree->h[GREEN].single && tree->h[RED].single && tree->h[BLUE].single && tree->h[ALPHA].single &&
                    tree->h[GREEN].symbol < 256) {
                    const size_t n = hi.bits == 0 ? num - index : next_block - index;
                    const uint32_t px = (uint32_t)tree->h[RED].symbol | ((uint32_t)tree->h[GREEN].symbol << 8) |
                                        ((uint32_t)(tree->h[BLUE].symbol & 255) << 16) |
                                        ((uint32_t)(tree->h[ALPHA].symbol & 255) << 24);
                    for (size_t i = 0; i < n; i++) st32(data + (index + i) * 4, px);
                    if (hi.cache.bits) hi.cache.insert(px);
                    index += n;
                    continue;
                }
            }
            uint16_t code;
            if (!tree->h[GREEN].read(br, &code)) return ZW_EBITSTREAM;
            if (code < 256) {  // a literal
                uint16_t r, b, a;
                if (!tree->h[RED].read(br, &r) || !tree->h[BLUE].read(br, &b) || !tree->h[ALPHA].read(br, &a))
                    return ZW_EBITSTREAM;
                const uint32_t px = (uint32_t)(r & 255) | ((uint32_t)code << 8) | ((uint32_t)(b & 255) << 16) |
                                    ((uint32_t)(a & 255) << 24);
                st32(data + index * 4, px);
                if (hi.cache.bits) hi.cache.insert(px);
                index++;
            } else if (code < 256 + 24) {  // a backward reference
                size_t length, dist_code;
                uint16_t ds;
                if (!copy_distance(code - 256u, &length)) return ZW_EBITSTREAM;
                if (!tree->h[DIST].read(br, &ds) || ds >= 40) return ZW_EBITSTREAM;
                if (!copy_distance(ds, &dist_code)) return ZW_EBITSTREAM;
                const size_t dist = plane_distance(w, dist_code);
                if (index < dist || num - index < length) return ZW_EBITSTREAM;
                // (the reference skips the cache for dist == 1, where every copied
                // pixel equals one the cache already holds at its slot: the same state)
                for (size_t i = 0; i < length; i++) {
                    const uint32_t px = ld32(data + (index + i - dist) * 4);
                    st32(data + (index + i) * 4, px);
                    if (hi.cache.bits) hi.cache.insert(px);
                }
                index += length;
            } else {  // a colour-cache index
                const size_t k = code - 280u;
                if (!hi.cache.bits || k >= hi.cache.c.size()) return ZW_EBITSTREAM;
                st32(data + index * 4, hi.cache.c[k]);
                index++;
            }
        }
        return ZW_OK;
    }

    // decode_image_stream (lossless.rs:184-199)
    int decode_image_stream(uint32_t xsize, uint32_t ysize, bool is_argb, uint8_t* data)
    {
        unsigned cache_bits;
        if (int r = read_color_cache(&cache_bits)) return r;
        HuffInfo hi;
        if (int r = read_huffman_codes(is_argb, xsize, ysize, cache_bits, hi)) return r;
        return decode_image_data(xsize, ysize, hi, data);
    }

    // read_transforms (lossless.rs:202-286): the width of the coded image
    int read_transforms(uint32_t* xsize_out)
    {
        uint32_t xsize = width, v;
        for (;;) {
            if (!br.read(1, &v)) return ZW_EBITSTREAM;
            if (!v) break;
            uint32_t type;
            if (!br.read(2, &type)) return ZW_EBITSTREAM;
            if (tf[type].present) return ZW_ETRANSFORM;  // one of each at most
            order.push_back((uint8_t)type);
            Transform& T = tf[type];
            if (type == T_PREDICTOR || type == T_COLOR) {
                if (!br.read(3, &v)) return ZW_EBITSTREAM;
                T.size_bits = v + 2;
                const uint32_t bx = subsample_size(xsize, T.size_bits), by = subsample_size(height, T.size_bits);
                T.data.assign((size_t)bx * by * 4, 0);
                if (int r = decode_image_stream(bx, by, false, T.data.data())) return r;
            } else if (type == T_COLOR_INDEXING) {
                if (!br.read(8, &v)) return ZW_EBITSTREAM;
                T.table_size = v + 1;
                T.data.assign((size_t)T.table_size * 4, 0);
                if (int r = decode_image_stream(T.table_size, 1, false, T.data.data())) return r;
                const uint32_t bits = T.table_size <= 2 ? 3 : (T.table_size <= 4 ? 2 : (T.table_size <= 16 ? 1 : 0));
                xsize = subsample_size(xsize, bits);
                // adjust_color_map (lossless.rs:289-293): the table is subtraction-coded
                for (size_t i = 4; i < T.data.size(); i++) T.data[i] = (uint8_t)(T.data[i] + T.data[i - 4]);
            }
            T.present = true;
        }
        *xsize_out = xsize;
        return ZW_OK;
    }
};

// --- the inverse transforms (lossless_transform.rs) -------------------------
uint8_t average2(uint8_t a, uint8_t b) { return (uint8_t)(((unsigned)a + b) / 2); }  // :582-584
uint8_t clamp_full(int a, int b, int c)                                               // :595-599
{
    const int v = a + b - c;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
uint8_t clamp_half(int a, int b)  // :602-606 (the division truncates towards zero)
{
    const int v = a + (a - b) / 2;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// apply_predictor_transform_N (lossless_transform.rs:77-353) over the bytes
// [start, end) of a row below the first, left of them already final.  L, T, TL
// and TR are 4, 4 w, 4 w + 4 and 4 w - 4 bytes back; the last pixel's TR is the
// row's own first pixel, as the flat indexing of the reference gives it.
void predict_run(uint8_t* d, size_t start, size_t end, size_t w4, unsigned mode)
{
    for (size_t p = start; p < end; p += 4) {
        const uint8_t *L = d + p - 4, *T = d + p - w4, *TL = T - 4, *TR = T + 4;
        uint8_t pred[4];
        switch (mode) {
        case 0: pred[0] = pred[1] = pred[2] = 0, pred[3] = 255; break;
        case 1: memcpy(pred, L, 4); break;
        case 2: memcpy(pred, T, 4); break;
        case 3: memcpy(pred, TR, 4); break;
        case 4: memcpy(pred, TL, 4); break;
        case 5: for (int i = 0; i < 4; i++) pred[i] = average2(average2(L[i], TR[i]), T[i]); break;
        case 6: for (int i = 0; i < 4; i++) pred[i] = average2(L[i], TL[i]); break;
        case 7: for (int i = 0; i < 4; i++) pred[i] = average2(L[i], T[i]); break;
        case 8: for (int i = 0; i < 4; i++) pred[i] = average2(TL[i], T[i]); break;
        case 9: for (int i = 0; i < 4; i++) pred[i] = average2(T[i], TR[i]); break;
        case 10: for (int i = 0; i < 4; i++) pred[i] = average2(average2(L[i], TL[i]), average2(T[i], TR[i])); break;
        case 11: {  // select (:226-283)
            int pl = 0, pt = 0;
            for (int i = 0; i < 4; i++) {
                const int predict = (int)L[i] + T[i] - TL[i];
                pl += predict > L[i] ? predict - L[i] : L[i] - predict;
                pt += predict > T[i] ? predict - T[i] : T[i] - predict;
            }
            memcpy(pred, pl < pt ? L : T, 4);
            break;
        }
        case 12: for (int i = 0; i < 4; i++) pred[i] = clamp_full(L[i], T[i], TL[i]); break;
        case 13: for (int i = 0; i < 4; i++) pred[i] = clamp_half(((int)L[i] + T[i]) / 2, TL[i]); break;
        default: return;  // (modes 14 and up leave the residual, :70)
        }
        for (int i = 0; i < 4; i++) d[p + i] = (uint8_t)(d[p + i] + pred[i]);
    }
}

// apply_predictor_transform (lossless_transform.rs:26-76)
void inverse_predictor(uint8_t* d, uint32_t width, uint32_t height, uint32_t size_bits, const uint8_t* pdata)
{
    const size_t w = width, w4 = w * 4, bxs = subsample_size(width, size_bits);
    d[3] = (uint8_t)(d[3] + 255);  // the first pixel: opaque black
    for (size_t i = 4; i < w4; i++) d[i] = (uint8_t)(d[i] + d[i - 4]);  // the first row: L
    for (size_t y = 1; y < height; y++)                               // the first column: T
        for (size_t i = 0; i < 4; i++) d[y * w4 + i] = (uint8_t)(d[y * w4 + i] + d[(y - 1) * w4 + i]);
    for (size_t y = 1; y < height; y++)
        for (size_t bx = 0; bx < bxs; bx++) {
            const unsigned mode = pdata[((y >> size_bits) * bxs + bx) * 4 + 1];
            const size_t x0 = (bx << size_bits) > 1 ? (bx << size_bits) : 1;
            const size_t x1 = ((bx + 1) << size_bits) < w ? ((bx + 1) << size_bits) : w;
            if (x0 < x1) predict_run(d, (y * w + x0) * 4, (y * w + x1) * 4, w4, mode);
        }
}

// color_transform_delta and apply_color_transform (lossless_transform.rs:355-393, :609-611)
uint32_t color_delta(int8_t t, int8_t c) { return (uint32_t)((int32_t)t * (int32_t)c) >> 5; }
void inverse_color(uint8_t* d, uint32_t width, uint32_t height, uint32_t size_bits, const uint8_t* tdata)
{
    const size_t w = width, bxs = subsample_size(width, size_bits);
    for (size_t y = 0; y < height; y++)
        for (size_t x = 0; x < w; x++) {
            const uint8_t* t = tdata + ((y >> size_bits) * bxs + (x >> size_bits)) * 4;
            uint8_t* px = d + (y * w + x) * 4;
            const uint8_t red_to_blue = t[0], green_to_blue = t[1], green_to_red = t[2];
            uint32_t red = px[0], blue = px[2];
            red += color_delta((int8_t)green_to_red, (int8_t)px[1]);
            blue += color_delta((int8_t)green_to_blue, (int8_t)px[1]);
            blue += color_delta((int8_t)red_to_blue, (int8_t)(uint8_t)red);
            px[0] = (uint8_t)red;
            px[2] = (uint8_t)blue;
        }
}

// apply_color_indexing_transform (lossless_transform.rs:402-577): the coded
// image holds table indices in green, 8 / 4 / 2 / 1 of them per pixel for tables
// of up to 2 / 4 / 16 / 256 entries; an index past the table is transparent
// black.  Rows are expanded in place from the last to the first (the packed
// row y ends before the expanded row y starts).
void inverse_color_indexing(uint8_t* d, uint32_t width, uint32_t height, uint32_t table_size, const uint8_t* table)
{
    const unsigned wbits = table_size <= 2 ? 3 : (table_size <= 4 ? 2 : (table_size <= 16 ? 1 : 0));
    const unsigned per = 1u << wbits, bpe = 8u >> wbits, mask = (1u << bpe) - 1;
    const size_t w = width, pw = subsample_size(width, wbits);
    std::vector<uint8_t> packed(pw);
    for (size_t y = height; y-- > 0;) {
        for (size_t i = 0; i < pw; i++) packed[i] = d[(y * pw + i) * 4 + 1];
        for (size_t x = 0; x < w; x++) {
            const unsigned k = (packed[x / per] >> ((x % per) * bpe)) & mask;
            st32(d + (y * w + x) * 4, k < table_size ? ld32(table + (size_t)k * 4) : 0u);
        }
    }
}

int header(BitReader& br, uint32_t* w, uint32_t* h)
{
    uint32_t v;
    if (!br.read(8, &v)) return ZW_EBITSTREAM;
    if (v != 0x2f) return ZW_ELOSSLESS_SIGNATURE;
    if (!br.read(14, w) || !br.read(14, h)) return ZW_EBITSTREAM;
    *w += 1;
    *h += 1;
    if (!br.read(1, &v)) return ZW_EBITSTREAM;  // alpha_used: a hint
    if (!br.read(3, &v)) return ZW_EBITSTREAM;
    if (v != 0) return ZW_EVERSION_NUMBER;
    return ZW_OK;
}

}  // namespace

int read_header(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height)
{
    BitReader br(data, len);
    return header(br, width, height);
}

namespace {

// px == NULL: `grow` is sized to the image once the transforms have been read
int decode_coded_impl(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims, uint8_t* px,
                      size_t cap, std::vector<uint8_t>* grow, Coded& out)
{
    Decoder D(data, len);
    if (implicit_dims) {
        D.width = width;
        D.height = height;
    } else {
        if (int r = header(D.br, &D.width, &D.height)) return r;
        if ((width || height) && (D.width != width || D.height != height)) return ZW_EINCONSISTENT_SIZES;
    }
    if (D.width == 0 || D.height == 0 || D.width > 16384 || D.height > 16384) return ZW_EINVALID_DIMENSIONS;
    out.width = D.width;
    out.height = D.height;
    out.tf.clear();
    uint32_t tw = 0;
    const int rt = D.read_transforms(&tw);
    out.tw = tw;
    for (uint8_t type : D.order) {
        CodedTransform t;
        t.type = type;
        t.bits = type == T_COLOR_INDEXING ? D.tf[type].table_size : D.tf[type].size_bits;
        t.data.swap(D.tf[type].data);
        out.tf.push_back(std::move(t));
    }
    if (rt) return rt;
    if (!px) {
        grow->assign((size_t)D.width * D.height * 4, 0);
        px = grow->data();
    } else if (cap < (size_t)D.width * D.height * 4) {  // (tw <= width: the coded image fits)
        return ZW_EINVAL;
    }
    return D.decode_image_stream(tw, D.height, true, px);
}

}  // namespace

uint32_t packed_width(uint32_t width, uint32_t table_size)
{
    return subsample_size(width, table_size <= 2 ? 3 : (table_size <= 4 ? 2 : (table_size <= 16 ? 1 : 0)));
}

bool inverse_sizes_ok(const Coded& c)
{
    if (c.width == 0 || c.height == 0 || c.width > 16384 || c.height > 16384 || c.tf.size() > 4) return false;
    uint32_t seen = 0, w = c.width;
    for (const CodedTransform& t : c.tf) {  // bitstream order: the working width shrinks at the indexing transform
        if (t.type > 3 || (seen >> t.type & 1u)) return false;
        seen |= 1u << t.type;
        if (t.type == T_PREDICTOR || t.type == T_COLOR) {
            if (t.bits < 2 || t.bits > 9) return false;
            if (t.data.size() < (size_t)subsample_size(w, t.bits) * subsample_size(c.height, t.bits) * 4) return false;
        } else if (t.type == T_COLOR_INDEXING) {
            if (t.bits < 1 || t.bits > 256 || t.data.size() < (size_t)t.bits * 4) return false;
            w = packed_width(w, t.bits);
        }
    }
    return w == c.tw;
}

void inverse_transforms(uint8_t* px, const Coded& c)
{
    uint32_t w = c.tw;
    for (size_t k = c.tf.size(); k-- > 0;) {
        const CodedTransform& T = c.tf[k];
        switch (T.type) {
        case T_PREDICTOR: inverse_predictor(px, w, c.height, T.bits, T.data.data()); break;
        case T_COLOR: inverse_color(px, w, c.height, T.bits, T.data.data()); break;
        case T_SUBTRACT_GREEN:  // apply_subtract_green_transform (lossless_transform.rs:395-400)
            for (size_t i = 0; i < (size_t)w * c.height; i++) {
                px[i * 4] = (uint8_t)(px[i * 4] + px[i * 4 + 1]);
                px[i * 4 + 2] = (uint8_t)(px[i * 4 + 2] + px[i * 4 + 1]);
            }
            break;
        default:
            w = c.width;
            inverse_color_indexing(px, w, c.height, T.bits, T.data.data());
            break;
        }
    }
}

namespace {

// decode_frame: the split read, then the host inverses
int decode_frame_impl(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims,
                      std::vector<uint8_t>& rgba, std::vector<uint8_t>* transforms)
{
    Coded c;
    const int r = decode_coded_impl(data, len, width, height, implicit_dims, nullptr, 0, &rgba, c);
    if (transforms) {
        transforms->clear();
        for (const CodedTransform& t : c.tf) transforms->push_back((uint8_t)t.type);
    }
    if (r) return r;
    inverse_transforms(rgba.data(), c);
    return ZW_OK;
}

}  // namespace

int decode_coded(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims, uint8_t* px,
                 size_t cap, Coded& out)
{
    if (!px || (!data && len)) return ZW_EINVAL;
    try {
        return decode_coded_impl(data, len, width, height, implicit_dims, px, cap, nullptr, out);
    } catch (const std::bad_alloc&) {
        return ZW_ENOMEM;
    }
}

int decode_frame(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims,
                 std::vector<uint8_t>& rgba, std::vector<uint8_t>* transforms)
{
    try {
        return decode_frame_impl(data, len, width, height, implicit_dims, rgba, transforms);
    } catch (const std::bad_alloc&) {
        return ZW_ENOMEM;
    }
}

}  // namespace zwvp8l

int zw_alph_read(const uint8_t* payload, size_t len, uint32_t width, uint32_t height, uint8_t* plane, int* filter,
                 std::vector<uint8_t>* transforms)
{
    if (!plane || !filter || (!payload && len) || width == 0 || height == 0 || width > 16384 || height > 16384)
        return ZW_EINVAL;
    if (transforms) transforms->clear();
    if (len == 0) return ZW_EBITSTREAM;
    const uint8_t info = payload[0];
    const unsigned preprocessing = (info >> 4) & 3, filtering = (info >> 2) & 3, compression = info & 3;
    if (preprocessing > 1) return ZW_EALPHA_PREPROCESSING;  // (the bit itself is not used, :328)
    if (compression > 1) return ZW_ECOMPRESSION_METHOD;
    *filter = (int)filtering;
    const size_t n = (size_t)width * height;
    if (compression == 1) {
        std::vector<uint8_t> rgba;
        if (int r = zwvp8l::decode_frame(payload + 1, len - 1, width, height, true, rgba, transforms)) return r;
        for (size_t i = 0; i < n; i++) plane[i] = rgba[i * 4 + 1];  // green
    } else {
        if (len - 1 < n) return ZW_EBITSTREAM;
        memcpy(plane, payload + 1, n);
    }
    return ZW_OK;
}

// The host-only test hooks of include/zwebp.h.
extern "C" int zw_dbg_alph_plane(const uint8_t* payload, size_t len, uint32_t width, uint32_t height, uint8_t* plane,
                                 int* filter)
{
    return zw_alph_read(payload, len, width, height, plane, filter, nullptr);
}

extern "C" int zw_dbg_vp8l_decode(const uint8_t* data, size_t len, uint32_t* argb_out, uint32_t* width,
                                  uint32_t* height)
{
    if (!width || !height || (!data && len)) return ZW_EINVAL;
    if (!argb_out) return zwvp8l::read_header(data, len, width, height);
    std::vector<uint8_t> rgba;
    if (int r = zwvp8l::read_header(data, len, width, height)) return r;
    if (int r = zwvp8l::decode_frame(data, len, 0, 0, false, rgba, nullptr)) return r;
    const size_t n = (size_t)*width * *height;
    for (size_t i = 0; i < n; i++)
        argb_out[i] = ((uint32_t)rgba[i * 4 + 3] << 24) | ((uint32_t)rgba[i * 4] << 16) |
                      ((uint32_t)rgba[i * 4 + 1] << 8) | rgba[i * 4 + 2];
    return ZW_OK;
}

// A hook image as the split reader's Coded (the data copied); false: out of range.
bool zw_vp8l_hook_image(const zw_vp8l_image& im, uint32_t width, uint32_t height, zwvp8l::Coded& c)
{
    if (!im.coded || im.ntransforms < 0 || im.ntransforms > 4) return false;
    c.width = c.tw = width;
    c.height = height;
    c.tf.clear();
    for (int k = 0; k < im.ntransforms; k++) {
        const zw_vp8l_transform& t = im.t[k];
        if (!t.data && t.len) return false;
        zwvp8l::CodedTransform ct;
        ct.type = t.type;
        ct.bits = t.bits;
        ct.data.assign(t.data, t.data + t.len);
        if (t.type == 3 && t.bits >= 1 && t.bits <= 256) c.tw = zwvp8l::packed_width(c.tw, t.bits);
        c.tf.push_back(std::move(ct));
    }
    return zwvp8l::inverse_sizes_ok(c);
}

extern "C" int zw_dbg_vp8l_inverse_host(int n, const zw_vp8l_image* images, uint32_t width, uint32_t height,
                                        uint8_t* out)
{
    if (n <= 0 || !images || !out || width == 0 || height == 0 || width > 16384 || height > 16384) return ZW_EINVAL;
    const size_t fbytes = (size_t)width * height * 4;
    try {
        for (int i = 0; i < n; i++) {
            zwvp8l::Coded c;
            if (!zw_vp8l_hook_image(images[i], width, height, c)) return ZW_EINVAL;
            uint8_t* px = out + (size_t)i * fbytes;
            memmove(px, images[i].coded, (size_t)c.tw * height * 4);
            zwvp8l::inverse_transforms(px, c);
        }
    } catch (const std::bad_alloc&) {
        return ZW_ENOMEM;
    }
    return ZW_OK;
}

extern "C" int zw_dbg_vp8l_read_coded(const uint8_t* data, size_t len, zw_bytes* out)
{
    if (!out || (!data && len)) return ZW_EINVAL;
    out->data = nullptr;
    out->len = 0;
    uint32_t w = 0, h = 0;
    if (int r = zwvp8l::read_header(data, len, &w, &h)) return r;
    try {
        std::vector<uint8_t> px((size_t)w * h * 4);
        zwvp8l::Coded c;
        if (int r = zwvp8l::decode_coded(data, len, 0, 0, false, px.data(), px.size(), c)) return r;
        std::vector<uint8_t> blob;
        auto word = [&](uint32_t v) {
            for (int k = 0; k < 4; k++) blob.push_back((uint8_t)(v >> (8 * k)));
        };
        const uint32_t head[8] = {c.width, c.height, c.tw, (uint32_t)c.tf.size(), 0, 0, 0, 0};
        for (uint32_t v : head) word(v);
        for (const zwvp8l::CodedTransform& t : c.tf) {
            word(t.type);
            word(t.bits);
            word((uint32_t)t.data.size());
            word(0);
            blob.insert(blob.end(), t.data.begin(), t.data.end());
            while (blob.size() & 3) blob.push_back(0);
        }
        blob.insert(blob.end(), px.begin(), px.begin() + (size_t)c.tw * c.height * 4);
        uint8_t* p = (uint8_t*)malloc(blob.size());
        if (!p) return ZW_ENOMEM;
        memcpy(p, blob.data(), blob.size());
        out->data = p;
        out->len = blob.size();
    } catch (const std::bad_alloc&) {
        return ZW_ENOMEM;
    }
    return ZW_OK;
}
