// The score order shared by the nearest-row search (neighbors.hip) and the k-means step (kmeans.hip): a 64-bit key
// (order key of the score << 32) | row, smaller = better.  The order key is the usual monotone map of the float's bits
// (complemented where a higher score is better), NaN = 0xFFFFFFFE behind every number, filler = all ones behind everything.
// The score is read back out of the key: a zero comes back as +0, a NaN as the quiet NaN 0x7FC00000.
#pragma once
#include "common.h"
#include <math.h>

#define TK_KC         32          // columns per staged chunk
#define TK_LD         (TK_KC + 1) // LDS row stride of the staged chunks: a lane's 32 rows fall on 32 banks
#define TK_MAX_ROWS   0x7FFFFF00ll // rows of either matrix: a row index, rounded up to its tile, is an int
#define TK_MAX_STRIDE (1ll << 23)   // row stride in elements: a tile's offsets stay within 32 bits
#define TK_FILLER     0xFFFFFFFFFFFFFFFFull
#define TK_KEY_NAN    0xFFFFFFFEu

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t tk_order_key(float s, bool lower_better) {
    if (s != s) return TK_KEY_NAN;
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;                                  // -0 == +0
    const uint32_t m = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);  // ascending with the float
    return lower_better ? m : ~m;
}

__device__ __forceinline__ float tk_key_score(uint32_t key, bool lower_better) {
    if (key == 0xFFFFFFFFu) return lower_better ? INFINITY : -INFINITY;
    if (key == TK_KEY_NAN) return __uint_as_float(0x7FC00000u);
    const uint32_t m = lower_better ? key : ~key;
    return __uint_as_float((m >> 31) ? (m ^ 0x80000000u) : ~m);
}
