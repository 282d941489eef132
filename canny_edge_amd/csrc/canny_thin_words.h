// canny_thin_words.h -- one sub-iteration of the thinning rule (include/canny_hip.h) on 64 pixels at once:
// what the kernels of canny_thin.hip compute per staged word.  Plain C++ apart from the qualifiers, so that
// tests/cpp/test_thin_words.cpp compiles it with the host compiler and runs it over all 512 neighbourhoods.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CANNY_THIN_FN __device__ __forceinline__
#else
#define CANNY_THIN_FN inline
#endif

namespace canny {

// bit-sliced counter over 64 pixels: after the terms, `one` = an odd number of them, `two` = at least two
struct OneTwo {
    uint64_t one = 0, two = 0;
    CANNY_THIN_FN void add(uint64_t t)
    {
        two |= one & t;
        one ^= t;
    }
    CANNY_THIN_FN uint64_t exactly_one() const { return one & ~two; }
};

// The pixels of the word p1 that sub-iteration `sub` deletes; p2 .. p9: the neighbour words.
template <int METHOD>
CANNY_THIN_FN uint64_t thin_deletions(uint64_t p1, uint64_t p2, uint64_t p3, uint64_t p4, uint64_t p5, uint64_t p6,
                                                   uint64_t p7, uint64_t p8, uint64_t p9, int sub)
{
    if constexpr (METHOD == 0) { // ZHANGSUEN
        const uint64_t r[8] = {p2, p3, p4, p5, p6, p7, p8, p9};
        OneTwo a, b, z;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            a.add(~r[i] & r[(i + 1) & 7]);
            b.add(r[i]);
            z.add(~r[i]);
        }
        const uint64_t guard = sub == 0 ? (p2 & p4 & p6) | (p4 & p6 & p8) : (p2 & p4 & p8) | (p2 & p6 & p8);
        return p1 & a.exactly_one() & b.two & z.two & ~guard; // A = 1, B >= 2, at least two unset: B <= 6
    } else {                     // GUOHALL
        const uint64_t a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8; // N1's terms
        const uint64_t b1 = p2 | p3, b2 = p4 | p5, b3 = p6 | p7, b4 = p8 | p9; // N2's terms
        OneTwo c, n1, n2;
        c.add(~p2 & a2), c.add(~p4 & a3), c.add(~p6 & a4), c.add(~p8 & a1);
        n1.add(a1), n1.add(a2), n1.add(a3), n1.add(a4);
        n2.add(b1), n2.add(b2), n2.add(b3), n2.add(b4);
        const uint64_t le3 = ~(a1 & a2 & a3 & a4) | ~(b1 & b2 & b3 & b4); // not all four of N1, or not all four of N2
        const uint64_t m = sub == 0 ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
        return p1 & c.exactly_one() & n1.two & n2.two & le3 & ~m;
    }
}

} // namespace canny
