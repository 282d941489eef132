// canny_recon_words.h -- the word steps of the reconstruction by dilation (include/canny_hip.h) on 64
// pixels at once: what the kernels of canny_reconstruct.hip compute per word.  Words are LSB-first: bit i is column 64 k + i.
// Plain C++ apart from the qualifiers, so that tests/cpp/test_recon_words.cpp compiles it with the host compiler and runs it
// against the bit-by-bit loop.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CANNY_RECON_FN __device__ __forceinline__
#else
#define CANNY_RECON_FN inline
#endif

namespace canny {

// The horizontal flood within a word: every pixel of g joined to a pixel of s, or to a carry, by a run of g inside the word.
// s: the state, a subset of g; g: the pixels that conduct; carry_lo: column 64 k - 1 is in the state; carry_hi: column
// 64 k + 64 is.  The occluded Kogge-Stone fill: six doubling steps each way, `p` the runs of g that reach back 2 k columns.
CANNY_RECON_FN uint64_t recon_fill(uint64_t s, uint64_t g, bool carry_lo, bool carry_hi)
{
    s |= ((uint64_t)carry_lo | ((uint64_t)carry_hi << 63)) & g;
    uint64_t up = s, p = g; // towards higher columns
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        up |= p & (up << k);
        p &= p << k;
    }
    uint64_t down = s;      // towards lower columns
    p = g;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        down |= p & (down >> k);
        p &= p >> k;
    }
    return up | down;
}

// The neighbours above and below that reach the word's pixels in one step: u, d the words of the rows above and below, the
// *l and *r their left and right neighbour words; connectivity 4: straight steps only, 8: the diagonals too.
CANNY_RECON_FN uint64_t recon_vertical(uint64_t ul, uint64_t u, uint64_t ur, uint64_t dl, uint64_t d, uint64_t dr, bool eight)
{
    uint64_t n = u | d;
    if (eight) {
        const uint64_t b = u | d, bl = ul | dl, br = ur | dr;
        n |= (b << 1) | (bl >> 63) | (b >> 1) | (br << 63);
    }
    return n;
}

// One geodesic dilation step of the word, without the flood: s | (dilate_c(s) & g).  l, r: the state words left and right.
CANNY_RECON_FN uint64_t recon_step(uint64_t s, uint64_t g, uint64_t l, uint64_t r, uint64_t vertical)
{
    return s | ((vertical | (s << 1) | (l >> 63) | (s >> 1) | (r << 63)) & g);
}

} // namespace canny
