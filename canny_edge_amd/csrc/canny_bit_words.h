// canny_bit_words.h -- rows of a bit map as LSB-first 64-bit words, for the kernels that work on whole words in LDS
// (canny_morph.hip, canny_thin.hip, canny_reconstruct.hip).  Device code only.
#pragma once
#include "canny_kernels.h"

namespace canny {

// bytes MSB-first in memory order <-> LSB-first word
__device__ __forceinline__ uint64_t flip_bits(uint64_t v) { return __builtin_bswap64(__brevll(v)); }

// Columns 64 k .. 64 k + 63 of row y of frame f; whatever lies outside the frame reads as `fill` (all ones or zero).
// plane: the strong bit-plane of geometry g; otherwise a packed map of rb bytes a row, vec: its rows are whole, 8-byte
// aligned words.
__device__ __forceinline__ uint64_t morph_load(const void *__restrict__ src, bool plane, bool vec, const HystGeom &g, int rb,
                                               int f, int y, int k, uint64_t fill)
{
    if (y < 0 || y >= g.height || k < 0 || k >= g.tiles_x) return fill;
    const int left = g.width - (k << 6);
    const uint64_t in = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    uint64_t w;
    if (plane)
        w = row_word<false>(src, g, rb, f, y, k);
    else if (vec)
        w = flip_bits(*reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(src) +
                                                          ((size_t)f * g.height + y) * (size_t)rb + (size_t)k * 8));
    else
        w = row_word<true>(src, g, rb, f, y, k);
    return (w & in) | (fill & ~in);
}

// columns 64 k + d .. 64 k + d + 63 from the words left of, at and right of k; -64 < d < 64
__device__ __forceinline__ uint64_t funnel(uint64_t l, uint64_t c, uint64_t r, int d)
{
    if (d == 0) return c;
    return d > 0 ? (c >> d) | (r << (64 - d)) : (c << -d) | (l >> (64 + d));
}

// The word v of columns 64 k .. of a packed row to `row` + 8 k: one store where the rows are whole aligned words, else the
// row's own bytes only.
__device__ __forceinline__ void store_word(uint8_t *row_at_k, uint64_t v, bool vec, int rb, int k)
{
    const uint64_t raw = flip_bits(v);
    if (vec) {
        *reinterpret_cast<uint64_t *>(row_at_k) = raw;
    } else {
        const int nb = min(8, rb - k * 8);
        for (int j = 0; j < nb; j++) row_at_k[j] = (uint8_t)(raw >> (8 * j));
    }
}

} // namespace canny
