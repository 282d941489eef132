// test_tile_div.cpp -- the reciprocal division of the hysteresis sweeps (csrc/canny_tile_div.h) against / and %.
// A stand-alone program with its own main, compiled by the host compiler alone (tests/test_tile_div.py):
//   g++ -std=c++17 -O2 -Icanny_edge_amd/csrc tests/cpp/test_tile_div.cpp -o test_tile_div
// 1. every divisor a frame of the tail route can have (tiles per frame, and tiles per row, up to 4096) with every tile
//    number below the limit of a 128-frame batch (which holds the limits of the smaller batches: 1, 2, 17 frames);
// 2. divisors over the whole int range (powers of two and their neighbours, primes, the largest) with the tile numbers
//    where a quotient steps (k * d - 1, k * d, k * d + 1 for small, large and the largest k) and the largest int.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "canny_tile_div.h"

static long long g_bad = 0;

static void check(uint32_t n, uint32_t d, canny::TileDiv v)
{
    const uint32_t q = canny::tile_div(n, v), r = n - q * d;
    if (q != n / d || r != n % d) {
        if (g_bad++ < 10) printf("MISMATCH n=%u d=%u: quotient %u remainder %u, want %u %u\n", n, d, q, r, n / d, n % d);
    }
}

int main()
{
    const uint32_t kMaxInt = 0x7fffffffu;
    long long n_checked = 0;
    for (uint32_t d = 1; d <= 4096; d++) {
        const canny::TileDiv v = canny::make_tile_div((int)d);
        for (uint32_t n = 0; n < 128u * d; n++) check(n, d, v);
        n_checked += 128ll * d;
    }
    uint32_t ds[256];
    int nd = 0;
    for (int s = 0; s < 31; s++) {
        const uint32_t p = UINT32_C(1) << s;
        ds[nd++] = p;
        if (p > 2) ds[nd++] = p - 1;
        ds[nd++] = p + 1;
    }
    for (uint32_t extra : {3u, 5u, 7u, 60u, 2040u, 4097u, 65521u, 1000003u, 16777213u, 1073741827u, 2147483629u, kMaxInt})
        ds[nd++] = extra;
    for (int i = 0; i < nd; i++) {
        const uint32_t d = ds[i];
        const canny::TileDiv v = canny::make_tile_div((int)d);
        const uint32_t kmax = kMaxInt / d;
        for (uint32_t j = 0; j <= 2000; j++) {
            for (uint32_t k : {j, kmax / 2 + j, kmax - (j <= kmax ? j : kmax)}) {
                if (k > kmax) continue;
                const uint64_t m = (uint64_t)k * d;
                for (int64_t n = (int64_t)m - 1; n <= (int64_t)m + 1; n++)
                    if (n >= 0 && n <= (int64_t)kMaxInt) check((uint32_t)n, d, v), n_checked++;
            }
        }
        check(kMaxInt, d, v);
    }
    printf("%lld quotients checked, %lld wrong\n", n_checked, g_bad);
    if (g_bad == 0) printf("tile_div ok\n");
    return g_bad == 0 ? 0 : 1;
}
