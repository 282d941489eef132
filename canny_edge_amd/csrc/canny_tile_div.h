// canny_tile_div.h -- exact division of a tile number by a tile count without a divide instruction (internal).
// The hysteresis sweeps turn every tile number into (frame, tile row, tile column); the divisors are fixed per call,
// so the host prepares them once (HystGeom) and a tile pays a shift, a multiply-high and a shift per quotient.
// Plain C++ apart from the function attributes: tests/cpp/test_tile_div.cpp compiles it with the host compiler alone.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CANNY_TILE_DIV_FN __host__ __device__ inline
#else
#define CANNY_TILE_DIV_FN inline
#endif

namespace canny {

// n / d == (2n * mul) >> (32 + shift) for every 0 <= n < 2^31 and every 1 <= d < 2^31, with
// shift = ceil(log2 d) and mul = ceil(2^(31 + shift) / d):
//   2^(shift-1) < d <= 2^shift gives 2^31 <= mul < 2^32, so mul fits a 32-bit word (d = 1: shift 0, mul 2^31);
//   mul * d = 2^(31+shift) + e with 0 <= e < d <= 2^shift, so n * mul / 2^(31+shift) = n / d + n * e / (d * 2^(31+shift)),
//   and the last term is below 1 / d for n < 2^31: too small to carry a quotient whose fraction is at most (d-1)/d
//   over the next integer.
// Tile numbers are ints (HystGeom::tiles()), so n < 2^31 always holds; 2n cannot overflow 32 bits.
struct TileDiv {
    uint32_t mul, shift;
};

inline TileDiv make_tile_div(int d)
{
    TileDiv v;
    v.shift = 0;
    while ((UINT32_C(1) << v.shift) < (uint32_t)d) v.shift++;
    v.mul = (uint32_t)(((UINT64_C(1) << (31 + v.shift)) + (uint32_t)d - 1) / (uint32_t)d);
    return v;
}

CANNY_TILE_DIV_FN uint32_t tile_div(uint32_t n, TileDiv v)
{
    return (uint32_t)(((uint64_t)(n << 1) * v.mul) >> 32) >> v.shift;
}

} // namespace canny
