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

}  // namespace zwvp8l

// read_alpha_chunk (decoder/extended.rs:273-334): the ALPH payload of a width x
// height image to its alpha plane before the filter is undone (width * height
// bytes at plane) and the filtering method (0 none, 1 horizontal, 2 vertical,
// 3 gradient).  transforms as above (empty for raw compression).
int zw_alph_read(const uint8_t* payload, size_t len, uint32_t width, uint32_t height, uint8_t* plane, int* filter,
                 std::vector<uint8_t>* transforms = nullptr);
