// Stand-alone check of csrc/canny_fuse_host.cpp (own main; built by tests/test_fuse_rule.py with the host compiler's address
// and undefined-behaviour sanitizers, together with that one file): the four ops against a sort written here, windows that
// slide, skip and leave a remainder, valid bit maps with dirty pad bits, pixels without a valid sample, the moving object and
// its masks, the widest sums (255 frames of 255) and refused calls -- all with buffers of exactly the needed size.
#include "canny_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

typedef std::vector<unsigned char> Bytes;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static Bytes noise(size_t n, uint32_t seed, int limit = 256)
{
    Bytes b(n);
    for (auto &v : b) v = (unsigned char)((lcg(seed) >> 16) % (uint32_t)limit);
    return b;
}

static bool bit(const Bytes &bits, int rb, int h, int f, int y, int x)
{
    return (bits[((size_t)f * h + y) * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
}

// the rule for one pixel from a sort
static int pixel(std::vector<int> v, int op, int fill, int min_count)
{
    const int c = (int)v.size();
    if (c < min_count) return fill;
    std::sort(v.begin(), v.end());
    long long s = 0;
    for (int x : v) s += x;
    if (op == CANNY_HIP_FUSE_MEAN) return (int)((2 * s + c) / (2 * c));
    return op == CANNY_HIP_FUSE_MEDIAN ? v[(c - 1) >> 1] : (op == CANNY_HIP_FUSE_MIN ? v[0] : v[c - 1]);
}

static int fuse_case(int n, int h, int w, int len, int step, int fill, int min_count, bool with_valid, uint32_t seed)
{
    const int rb = (w + 7) / 8, groups = (n - len) / step + 1;
    const Bytes frames = noise((size_t)n * h * w, seed, seed % 3 ? 256 : 3);
    Bytes valid = noise((size_t)n * h * rb, seed + 1);
    for (int op = 0; op < 4; op++) {
        Bytes fused((size_t)groups * h * w, 0xEE), count((size_t)groups * h * w, 0xEE);
        CHECK(canny_hip_fuse_frames(frames.data(), with_valid ? valid.data() : nullptr, n, h, w, len, step, op, fill, min_count,
                                    fused.data(), count.data()) == 0);
        for (int g = 0; g < groups; g++)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    std::vector<int> v;
                    for (int k = 0; k < len; k++) {
                        const int f = g * step + k;
                        if (!with_valid || bit(valid, rb, h, f, y, x)) v.push_back(frames[((size_t)f * h + y) * w + x]);
                    }
                    const size_t at = ((size_t)g * h + y) * w + x;
                    CHECK(count[at] == v.size() && fused[at] == pixel(v, op, fill, min_count));
                }
        // without the count buffer: the same frames
        Bytes again((size_t)groups * h * w, 0xEE);
        CHECK(canny_hip_fuse_frames(frames.data(), with_valid ? valid.data() : nullptr, n, h, w, len, step, op, fill, min_count,
                                    again.data(), nullptr) == 0 && again == fused);
    }
    return 0;
}

int main()
{
    // shapes around the byte of eight pixels, windows of every kind
    const int shapes[][2] = {{1, 1}, {2, 7}, {3, 8}, {5, 9}, {4, 17}, {1, 33}};
    uint32_t seed = 1;
    for (auto &s : shapes) {
        CHECK(fuse_case(1, s[0], s[1], 1, 1, 0, 1, false, seed++) == 0);
        CHECK(fuse_case(7, s[0], s[1], 3, 2, 77, 2, true, seed++) == 0);
        CHECK(fuse_case(9, s[0], s[1], 9, 9, 5, 9, true, seed++) == 0);
        CHECK(fuse_case(12, s[0], s[1], 5, 1, 0, 1, true, seed++) == 0);
        CHECK(fuse_case(11, s[0], s[1], 4, 4, 255, 1, false, seed++) == 0);
    }
    // the widest sums: 255 frames of 255 -- s = 65025, 2 s + c = 130305
    {
        const Bytes frames((size_t)255 * 2 * 3, 255);
        Bytes fused(6, 0), count(6, 0);
        for (int op = 0; op < 4; op++) {
            CHECK(canny_hip_fuse_frames(frames.data(), nullptr, 255, 2, 3, 255, 1, op, 0, 255, fused.data(), count.data()) == 0);
            for (int i = 0; i < 6; i++) CHECK(fused[i] == 255 && count[i] == 255);
        }
        CHECK(fuse_case(255, 2, 3, 255, 1, 9, 100, true, 99) == 0);
        CHECK(fuse_case(257, 1, 5, 255, 2, 9, 1, true, 98) == 0);
    }

    // the moving object: three copies of a background in 0..199, a 6 x 9 patch raised by 50 at three disjoint places
    {
        const int h = 40, w = 70, rb = 9;
        const Bytes bg = noise((size_t)h * w, 7, 200);
        Bytes frames;
        for (int f = 0; f < 3; f++) frames.insert(frames.end(), bg.begin(), bg.end());
        const int at[3][2] = {{3, 5}, {20, 30}, {31, 58}};
        for (int f = 0; f < 3; f++)
            for (int y = 0; y < 6; y++)
                for (int x = 0; x < 9; x++) frames[((size_t)f * h + at[f][0] + y) * w + at[f][1] + x] += 50;
        Bytes fused((size_t)h * w, 0xEE), count((size_t)h * w, 0xEE);
        CHECK(canny_hip_fuse_frames(frames.data(), nullptr, 3, h, w, 3, 3, CANNY_HIP_FUSE_MEDIAN, 0, 1, fused.data(),
                                    count.data()) == 0);
        CHECK(fused == bg);
        Bytes mask((size_t)3 * h * rb, 0xEE);
        std::vector<long long> changed(3, -7);
        CHECK(canny_hip_change_mask(frames.data(), nullptr, 3, h, w, fused.data(), count.data(), 3, 49, 3, mask.data(),
                                    changed.data()) == 0);
        for (int f = 0; f < 3; f++) {
            CHECK(changed[f] == 54);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < rb * 8; x++) {
                    const bool in = x < w && y >= at[f][0] && y < at[f][0] + 6 && x >= at[f][1] && x < at[f][1] + 9;
                    CHECK(bit(mask, rb, h, f, y, x) == in); // the pad bits are 0
                }
        }
        CHECK(canny_hip_change_mask(frames.data(), nullptr, 3, h, w, fused.data(), nullptr, 3, 50, 1, mask.data(),
                                    changed.data()) == 0);
        for (auto v : mask) CHECK(v == 0);
        for (auto v : changed) CHECK(v == 0);
        // counts below min_count switch the pixel off; one background per frame; no `changed`
        CHECK(canny_hip_change_mask(frames.data(), nullptr, 3, h, w, fused.data(), count.data(), 100, 49, 4, mask.data(),
                                    nullptr) == 0);
        for (auto v : mask) CHECK(v == 0);
        CHECK(canny_hip_change_mask(frames.data(), nullptr, 3, h, w, frames.data(), nullptr, 1, 0, 1, mask.data(), nullptr) == 0);
        for (auto v : mask) CHECK(v == 0);
        // valid bits switch pixels off, dirty pad bits change nothing
        Bytes valid((size_t)3 * h * rb, 0xFF);
        valid[((size_t)1 * h + 20) * rb + (30 >> 3)] = 0; // pixels 24..31 of row 20 of frame 1: two of the patch
        CHECK(canny_hip_change_mask(frames.data(), valid.data(), 3, h, w, fused.data(), count.data(), 3, 49, 1, mask.data(),
                                    changed.data()) == 0);
        CHECK(changed[0] == 54 && changed[1] == 52 && changed[2] == 54);
        for (int f = 0; f < 3; f++)
            for (int y = 0; y < h; y++)
                for (int x = w; x < rb * 8; x++) CHECK(!bit(mask, rb, h, f, y, x));
    }

    // refused calls write nothing
    {
        const Bytes frames = noise(4 * 6 * 9, 3);
        Bytes fused(2 * 6 * 9, 0xEE), count(2 * 6 * 9, 0xEE), mask(4 * 6 * 2, 0xEE);
        std::vector<long long> changed(5, -7);
        const unsigned char *F = frames.data();
        CHECK(canny_hip_fuse_frames(nullptr, nullptr, 4, 6, 9, 2, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, 0, 1, nullptr, count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 0, 6, 9, 2, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 0, 9, 2, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 0, 2, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 0, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 5, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 300, 6, 9, 256, 2, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 0, 1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 4, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, -1, 0, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, 256, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, -1, 1, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, 0, 0, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, 0, 256, fused.data(), count.data()) == 1);
        CHECK(canny_hip_fuse_frames(fused.data(), nullptr, 2, 6, 9, 2, 2, 1, 0, 1, fused.data() + 107, nullptr) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 9, 2, 2, 1, 0, 1, fused.data(), fused.data() + 50) == 1);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 32769, 9, 2, 2, 1, 0, 1, fused.data(), count.data()) == 2);
        CHECK(canny_hip_fuse_frames(F, nullptr, 4, 6, 32769, 2, 2, 1, 0, 1, fused.data(), count.data()) == 2);
        CHECK(canny_hip_fuse_frames(F, nullptr, 65536, 6, 9, 2, 2, 1, 0, 1, fused.data(), count.data()) == 2);
        CHECK(canny_hip_change_mask(nullptr, nullptr, 4, 6, 9, F, nullptr, 2, 10, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, nullptr, nullptr, 2, 10, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, 10, 1, nullptr, changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 0, 6, 9, F, nullptr, 2, 10, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 0, 10, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, -1, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, 256, 1, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, 10, 0, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, 10, 256, mask.data(), changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 6, 9, F, nullptr, 2, 10, 1, mask.data(),
                                    (long long *)((char *)changed.data() + 4)) == 1);
        CHECK(canny_hip_change_mask(F, mask.data(), 4, 6, 9, F, nullptr, 2, 10, 1, mask.data() + 47, changed.data()) == 1);
        CHECK(canny_hip_change_mask(F, nullptr, 4, 32769, 9, F, nullptr, 2, 10, 1, mask.data(), changed.data()) == 2);
        CHECK(canny_hip_change_mask(F, nullptr, 65536, 6, 9, F, nullptr, 2, 10, 1, mask.data(), changed.data()) == 2);
        for (auto v : fused) CHECK(v == 0xEE);
        for (auto v : count) CHECK(v == 0xEE);
        for (auto v : mask) CHECK(v == 0xEE);
        for (auto v : changed) CHECK(v == -7);
    }
    std::printf("fuse ok\n");
    return 0;
}
