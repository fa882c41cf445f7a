// zw_vp8l_dec.h -- host reader of VP8L (lossless) bitstreams and of the ALPH
// chunk that carries a lossy file's alpha plane.  Plain C++, no device code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zwvp8l {

// The 5-byte header of a headered stream (decode_frame, decoder/lossless.rs:103-118):
// ZW_OK and the dimensions, or the decoder code.
int read_header(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height);

// LosslessDecoder::decode_frame (decoder/lossless.rs:92-177).  implicit_dims:
// the headerless form of an ALPH chunk, width x height given; otherwise the
// header gives them (and must match width x height unless both are 0).
// rgba: width * height pixels of 4 bytes in the reference's order R, G, B, A.
// transforms (may be NULL): the transform types in bitstream order.
// Damaged input returns a decoder code; nothing is read or written out of bounds.
int decode_frame(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims,
                 std::vector<uint8_t>& rgba, std::vector<uint8_t>* transforms);

// The same stream read up to the inverse transforms: the coded image as
// decode_image_stream leaves it and the transforms in bitstream order.
struct CodedTransform {
    uint32_t type = 0;  // 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour indexing
    uint32_t bits = 0;  // size_bits of types 0 and 1, table_size of type 3
    // types 0 and 1: the sub-image, ceil(w / 2^bits) x ceil(height / 2^bits) pixels
    // R, G, B, A with w the working width at that transform; type 3: table_size
    // entries R, G, B, A (the subtraction coding already undone)
    std::vector<uint8_t> data;
};
struct Coded {
    uint32_t width = 0, height = 0;
    uint32_t tw = 0;  // the coded image's width: `width` packed when a colour indexing transform is present
    std::vector<CodedTransform> tf;
};
// The packed width of `width` pixels under a table of table_size entries.
uint32_t packed_width(uint32_t width, uint32_t table_size);
// decode_frame up to the transforms.  px: room for width * height pixels (`cap`
// bytes; ZW_EINVAL when the header's size needs more); on ZW_OK its first
// tw * height pixels hold the coded image.
int decode_coded(const uint8_t* data, size_t len, uint32_t width, uint32_t height, bool implicit_dims, uint8_t* px,
                 size_t cap, Coded& out);
// The host inverses over px (width * height pixels, the coded image in front):
// the transforms undone in reverse order, the working width tw until the colour
// indexing inverse has run.  The data sizes must match (inverse_sizes_ok).
void inverse_transforms(uint8_t* px, const Coded& c);
// Whether c describes transforms the inverses can run: dimensions 1..16384,
// each type at most once, size_bits 2..9, table_size 1..256, tw the packed
// width, every data vector at least its sub-image's or table's size.
bool inverse_sizes_ok(const Coded& c);

}  // namespace zwvp8l

// read_alpha_chunk (decoder/extended.rs:273-334): the ALPH payload of a width x
// height image to its alpha plane before the filter is undone (width * height
// bytes at plane) and the filtering method (0 none, 1 horizontal, 2 vertical,
// 3 gradient).  transforms as above (empty for raw compression).
int zw_alph_read(const uint8_t* payload, size_t len, uint32_t width, uint32_t height, uint8_t* plane, int* filter,
                 std::vector<uint8_t>* transforms = nullptr);
