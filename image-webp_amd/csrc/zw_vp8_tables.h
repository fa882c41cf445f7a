// zw_vp8_tables.h -- the VP8 constant tables (zw_tables.inc) and the mode and
// token trees, shared by the encoder's host half and the decoder's parser.
#pragma once
#include <stdint.h>

namespace zwh {

#define ZW_TABLE(T, N, D, ...) static const T N D = {__VA_ARGS__};
#include "zw_tables.inc"
#undef ZW_TABLE

static const int8_t SEGMENT_ID_TREE[6] = {2, 4, -0, -1, -2, -3};
static const int8_t YMODE_TREE[8] = {-4, 2, 4, 6, -0, -1, -2, -3};
static const int8_t BMODE_TREE[18] = {-0, 2, -1, 4, -2, 6, 8, 12, -3, 10, -5, -6, -4, 14, -7, 16, -8, -9};
static const int8_t UVMODE_TREE[6] = {-0, 2, -1, 4, -2, -3};
static const int8_t TOKEN_TREE[22] = {-11, 2, -0, 4, -1, 6, 8, 12, -2, 10, -3, -4,
                                      14, 16, -5, -6, 18, 20, -7, -8, -9, -10};

}  // namespace zwh
