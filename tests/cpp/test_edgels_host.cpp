// test_edgels_host.cpp -- canny_hip_edgels_from_plane (csrc/canny_edgels_host.cpp) on the shapes of tests/test_edgels_rule.py,
// with every buffer allocated at its exact size: built with the host compiler's -fsanitize=address,undefined together with
// that one source file, it shows that the host rule neither reads nor writes outside its buffers and computes without
// overflow.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_edgels_host.cpp canny_edge_amd/csrc/canny_edgels_host.cpp -o test_edgels_host
// No device, no library: the program has its own main and links nothing else.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "canny_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line)
{
    if (ok) return;
    fprintf(stderr, "FAILED line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

uint32_t rng_state = 12345u;
uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Rec {
    int x_q8, y_q8;
    unsigned grad, word3;
};

// every pixel of the plane plus three indices beyond it; the invariants every record keeps
template <class T>
void run_plane(const std::vector<T> &plane, int h, int w)
{
    std::vector<unsigned> idx((size_t)h * w + 3);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (unsigned)i;
    idx[idx.size() - 1] = 0xffffffffu;
    idx[idx.size() - 2] = 0x80000000u;
    std::vector<int> out(idx.size() * CANNY_HIP_EDGEL_INTS);
    EXPECT(canny_hip_edgels_from_plane(plane.data(), sizeof(T) == 1, h, w, idx.data(), idx.size(), out.data()) == CANNY_HIP_OK);
    for (size_t i = 0; i < idx.size(); i++) {
        const Rec r{out[4 * i], out[4 * i + 1], (unsigned)out[4 * i + 2], (unsigned)out[4 * i + 3]};
        if (idx[i] >= (unsigned)(h * w)) {
            EXPECT(r.word3 == CANNY_HIP_EDGEL_INVALID && !r.x_q8 && !r.y_q8 && !r.grad);
            continue;
        }
        const int x = (int)(idx[i] % (unsigned)w), y = (int)(idx[i] / (unsigned)w);
        const int tx = r.x_q8 - 256 * x, ty = r.y_q8 - 256 * y;
        const unsigned dir = (r.word3 >> CANNY_HIP_EDGEL_DIR_SHIFT) & 3u;
        EXPECT(!(r.word3 & CANNY_HIP_EDGEL_INVALID));
        EXPECT(tx >= -128 && tx <= 128 && ty >= -128 && ty <= 128);
        EXPECT(dir != 0 || ty == 0);
        EXPECT(dir != 2 || tx == 0);
        EXPECT(dir != 1 || tx == ty);
        EXPECT(dir != 3 || tx == -ty);
        if (r.word3 & CANNY_HIP_EDGEL_REFINED) {
            const int dx = dir != 2, dy = dir == 0 ? 0 : 1;
            EXPECT(x - dx >= 0 && x + dx < w && y - dy >= 0 && y + dy < h && r.grad != 0);
        } else {
            EXPECT(tx == 0 && ty == 0);
        }
    }
}

template <class T>
void random_planes(int h, int w, int lo, int span)
{
    std::vector<T> p((size_t)h * w);
    for (auto &v : p) v = (T)(lo + (int)(rng() % (unsigned)span));
    run_plane(p, h, w);
}

} // namespace

int main()
{
    // random planes: u8, and s16 over its whole range (the wrap through short, M near 2^31, the 64-bit root)
    const int shapes[][2] = {{37, 53}, {2, 2}, {2, 70}, {70, 2}, {9, 11}};
    for (const auto &s : shapes) {
        random_planes<uint8_t>(s[0], s[1], 0, 256);
        random_planes<int16_t>(s[0], s[1], -32768, 65536);
        random_planes<int16_t>(s[0], s[1], 0, 256);
    }
    // the ends of s16 as a checkerboard and as stripes: the largest sums before the wrap
    for (int kind = 0; kind < 3; kind++) {
        std::vector<int16_t> p(9 * 11);
        for (int y = 0; y < 9; y++)
            for (int x = 0; x < 11; x++)
                p[(size_t)y * 11 + x] = (kind == 0 ? (x + y) & 1 : kind == 1 ? x & 1 : (y >> 1) & 1) ? 32767 : -32768;
        run_plane(p, 9, 11);
    }
    // designed rows: a flat plane (zero gradient), a ramp (b == a == c) and a profile with b == a > c (t_q8 = -128)
    {
        std::vector<uint8_t> flat(6 * 8, 77), ramp(6 * 8), tie(6 * 8);
        const int profile[8] = {0, 0, 10, 20, 30, 30, 30, 30};
        for (int y = 0; y < 6; y++)
            for (int x = 0; x < 8; x++) ramp[(size_t)y * 8 + x] = (uint8_t)(10 * x), tie[(size_t)y * 8 + x] = (uint8_t)profile[x];
        run_plane(flat, 6, 8);
        run_plane(ramp, 6, 8);
        run_plane(tie, 6, 8);
        const unsigned at[2] = {2 * 8 + 3, 2 * 8 + 2};
        int out[8];
        EXPECT(canny_hip_edgels_from_plane(tie.data(), 1, 6, 8, at, 2, out) == CANNY_HIP_OK);
        EXPECT(out[0] == 256 * 3 - 128 && out[1] == 256 * 2 && ((unsigned)out[3] & CANNY_HIP_EDGEL_REFINED));
        EXPECT(out[4] == 256 * 2 + 128 && out[5] == 256 * 2 && ((unsigned)out[7] & CANNY_HIP_EDGEL_REFINED));
        EXPECT(canny_hip_edgels_from_plane(ramp.data(), 1, 6, 8, at, 2, out) == CANNY_HIP_OK);
        EXPECT(out[0] == 256 * 3 && !((unsigned)out[3] & CANNY_HIP_EDGEL_REFINED) && ((unsigned)out[3] & CANNY_HIP_EDGEL_MAG_MASK) == 16u * 80u);
        EXPECT(canny_hip_edgels_from_plane(flat.data(), 1, 6, 8, at, 2, out) == CANNY_HIP_OK);
        EXPECT(out[2] == 0 && out[3] == 0);
    }
    // statuses: nothing is read or written
    {
        uint8_t px[4] = {0, 1, 2, 3};
        unsigned one = 0;
        int out[4];
        EXPECT(canny_hip_edgels_from_plane(nullptr, 1, 2, 2, &one, 1, out) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_edgels_from_plane(px, 1, 1, 4, &one, 1, out) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_edgels_from_plane(px, 1, 2, 2, nullptr, 1, out) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_edgels_from_plane(px, 1, 2, 2, &one, 1, nullptr) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_edgels_from_plane(px, 1, 2, 2, nullptr, 0, nullptr) == CANNY_HIP_OK);
    }
    if (failures) return 1;
    printf("designed planes ok\n");
    return 0;
}
