// test_line_fits_host.cpp -- canny_hip_line_fits_from_plane and canny_hip_line_fits_finish (csrc/canny_line_fits_host.cpp) on
// the shapes of tests/test_line_fits_rule.py, with every buffer allocated at its exact size: built with the host compiler's
// -fsanitize=address,undefined together with that source file and csrc/canny_edgels_host.cpp, it shows that the host rule
// neither reads nor writes outside its buffers and computes without overflow, at the limits of the moments too.
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_line_fits_host.cpp canny_edge_amd/csrc/canny_line_fits_host.cpp \
//       canny_edge_amd/csrc/canny_edgels_host.cpp -o test_line_fits_host
// No device, no library: the program has its own main and links nothing else.
#include <cmath>
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

uint32_t rng_state = 2468u;
uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Frame {
    int h, w, numangle, numrho;
    float rho;
    std::vector<unsigned char> bits;
    std::vector<float> tc, ts;
    void set(int x, int y) { bits[(size_t)y * ((w + 7) / 8) + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7)); }
    // the accumulator cell of pixel (x, y) at angle n, as the rule votes
    unsigned base_of(int n, int x, int y) const
    {
        const float a = (float)x * tc[n], b = (float)y * ts[n];
        const int r = (int)std::nearbyintf(a + b) + (numrho - 1) / 2;
        return (unsigned)((n + 1) * (numrho + 2) + r + 1);
    }
};

Frame make_frame(int h, int w, float rho)
{
    Frame f{h, w, 180, (int)std::nearbyint((2.0 * (w + h) + 1.0) / rho), rho, {}, {}, {}};
    f.bits.assign((size_t)h * ((w + 7) / 8), 0);
    f.tc.resize(180), f.ts.resize(180);
    const float irho = 1.0f / rho, theta = (float)(M_PI / 180.0);
    float ang = 0.0f;
    for (int n = 0; n < 180; n++, ang = ang + theta) {
        f.tc[n] = (float)(std::cos((double)ang) * (double)irho);
        f.ts[n] = (float)(std::sin((double)ang) * (double)irho);
    }
    return f;
}

// every record of `seg` with options 0..3 on plane `plane`; the invariants every record keeps
template <class T>
void run(const Frame &f, const std::vector<T> &plane, const std::vector<unsigned> &bases, const std::vector<int> &seg,
         int first_invalid)
{
    const int n_seg = (int)(seg.size() / CANNY_HIP_SEGMENT_INTS);
    for (int options = 0; options < 4; options++) {
        std::vector<int> out((size_t)n_seg * CANNY_HIP_LINE_FIT_INTS);
        EXPECT(canny_hip_line_fits_from_plane(f.bits.data(), plane.data(), sizeof(T) == 1, f.h, f.w, f.rho, f.numangle,
                                              f.numrho, f.tc.data(), f.ts.data(), bases.data(), (int)bases.size(),
                                              seg.data(), n_seg, options, out.data()) == CANNY_HIP_OK);
        for (int j = 0; j < n_seg; j++) {
            const int *r = out.data() + (size_t)j * CANNY_HIP_LINE_FIT_INTS, *s = seg.data() + (size_t)j * 6;
            const unsigned flags = (unsigned)r[9];
            if (j >= first_invalid) {
                EXPECT(flags == CANNY_HIP_LINE_FIT_INVALID);
                for (int i = 0; i < 12; i++) EXPECT(i == 9 || r[i] == 0);
                continue;
            }
            EXPECT(!(flags & CANNY_HIP_LINE_FIT_INVALID) && r[8] >= 0);
            if (options == 0) EXPECT(s[5] == 1 ? r[8] >= 1 : r[8] == s[5]); // (a wide cell holds neighbours of the single pixel)
            if (flags & CANNY_HIP_LINE_FIT_DEGENERATE) {
                EXPECT(r[0] == 65536 * s[0] && r[1] == 65536 * s[1] && r[2] == 65536 * s[2] && r[3] == 65536 * s[3]);
                EXPECT(!r[6] && !r[7] && !r[10] && !r[11] && flags == CANNY_HIP_LINE_FIT_DEGENERATE);
                continue;
            }
            EXPECT(r[8] >= 2);
            const double len2 = (double)r[6] * r[6] + (double)r[7] * r[7], one = 1152921504606846976.0; // 2^60
            EXPECT(std::fabs(len2 - one) <= one / 268435456.0);
            EXPECT((long long)r[6] * (s[2] - s[0]) + (long long)r[7] * (s[3] - s[1]) >= 0);
            // the centroid lies between the two fitted end points, along the direction
            const long long p0 = (long long)(r[0] - r[4]) * r[6] + (long long)(r[1] - r[5]) * r[7];
            const long long p1 = (long long)(r[2] - r[4]) * r[6] + (long long)(r[3] - r[5]) * r[7];
            EXPECT(p0 <= (1ll << 31) && p1 >= -(1ll << 31));
        }
    }
}

template <class T>
void designed(int h, int w, float rho, int lo, int hi)
{
    Frame f = make_frame(h, w, rho);
    std::vector<T> plane((size_t)h * w);
    for (auto &v : plane) v = (T)(lo + (int)(rng() % (unsigned)(hi - lo + 1)));
    const int row = h / 2, col = w / 3, diag = h < w ? h : w;
    for (int x = 0; x < w; x++) f.set(x, row);          // a horizontal line over the whole width: from 0 to L - 1
    for (int y = 1; y < h - 1; y++) f.set(col, y);      // a vertical one
    for (int i = 0; i < diag; i++) f.set(i, i);         // the diagonal: the major-axis tie
    std::vector<unsigned> bases = {f.base_of(90, 0, row), f.base_of(0, col, 0), f.base_of(135, 0, 0), 0u,
                                   (unsigned)(f.numrho + 1), 0xffffffffu};
    // support of the three lines: the horizontal one also holds the crossing pixels of the other two
    int n_h = 0, n_v = 0, n_d = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (!(f.bits[(size_t)y * ((w + 7) / 8) + (x >> 3)] >> (7 - (x & 7)) & 1)) continue;
            n_h += f.base_of(90, x, y) == bases[0];
            n_v += f.base_of(0, x, y) == bases[1] && y >= 1 && y <= h - 2;
            n_d += f.base_of(135, x, y) == bases[2] && x < diag;
        }
    std::vector<int> seg = {0, row, w - 1, row, 0, n_h, col, 1, col, h - 2, 1, n_v, 0, 0, diag - 1, diag - 1, 2, n_d,
                            5, row, 5, row, 0, 1, // a single position: n = 1 at rho <= 1, degenerate
                            // invalid from here on: k outside the list, bases that are no cells, end points outside, ta > tb
                            0, row, w - 1, row, 6, 0, 0, row, w - 1, row, -1, 0, 0, row, w - 1, row, 3, 0, 0, row, w - 1, row, 4, 0,
                            0, row, w - 1, row, 5, 0, 0, row, w, row, 0, 0, 0, h, w - 1, row, 0, 0, -1, row, w - 1, row, 0, 0,
                            w - 1, row, 0, row, 0, 0, 2147483647, row, 2147483647, row, 0, 0};
    run(f, plane, bases, seg, 4);
    // a flat plane: no gradient anywhere, the gate removes every pixel
    std::vector<T> flat((size_t)h * w, (T)77);
    run(f, flat, bases, seg, 4);
    // no lines, no segments
    EXPECT(canny_hip_line_fits_from_plane(f.bits.data(), plane.data(), sizeof(T) == 1, h, w, rho, f.numangle, f.numrho,
                                          f.tc.data(), f.ts.data(), nullptr, 0, nullptr, 0, 0, nullptr) == CANNY_HIP_OK);
}

// the smallest frame, at the largest rho: both rows set, the top row as a segment
void tiny()
{
    Frame f = make_frame(2, 2, 8.0f);
    f.set(0, 0), f.set(1, 0), f.set(0, 1), f.set(1, 1);
    const std::vector<short> plane = {-5, 5, 300, -300};
    const std::vector<unsigned> bases = {f.base_of(90, 0, 0)};
    const std::vector<int> seg = {0, 0, 1, 0, 0, 4, 1, 0, 0, 0, 0, 0};
    std::vector<int> out(2 * CANNY_HIP_LINE_FIT_INTS);
    for (int options = 0; options < 4; options++) {
        EXPECT(canny_hip_line_fits_from_plane(f.bits.data(), plane.data(), 0, 2, 2, 8.0f, f.numangle, f.numrho, f.tc.data(),
                                              f.ts.data(), bases.data(), 1, seg.data(), 2, options, out.data()) == CANNY_HIP_OK);
        EXPECT(!((unsigned)out[9] & CANNY_HIP_LINE_FIT_INVALID) && (unsigned)out[12 + 9] == CANNY_HIP_LINE_FIT_INVALID);
        EXPECT(options || out[8] == 4); // at rho 8 all four pixels vote for the one cell
    }
}

void moments_at_the_limits()
{
    const long long n = 1ll << 18, big = (1ll << 22) + 128;
    const long long sets[][8] = {{n, 0, 0, n * big * big, n * big * big, n * big * big, 1, 1},
                                 {n, 0, 0, n * big * big, -n * big * big, n * big * big, -1, 1},
                                 {n, n * big, n * big, n * big * big, n * big * big, n * big * big, 1, 0},
                                 {n, -n * big, n * big, n * big * big, -n * big * big, n * big * big, 1, 0},
                                 {2, 0, 0, (1ll << 27) - 1, 0, 0, -16383, 16383},
                                 {2, 1, 1, 1, -((1ll << 27) - 1), 1, 16383, -16383},
                                 {0, 0, 0, 0, 0, 0, 1, 0},
                                 {1, big, -big, big * big, -big * big, big * big, 1, 0}};
    const size_t count = sizeof(sets) / sizeof(sets[0]);
    std::vector<int> out(6 * count);
    EXPECT(canny_hip_line_fits_finish(&sets[0][0], count, out.data()) == CANNY_HIP_OK);
    EXPECT(out[2] > 0 && out[3] > 0 && out[2] == out[3]);                  // the diagonal, along (1, 1)
    EXPECT(out[6 + 2] < 0 && out[6 + 3] > 0);                              // the anti-diagonal, along (-1, 1)
    EXPECT((unsigned)out[12 + 5] == CANNY_HIP_LINE_FIT_DEGENERATE);        // every point the same
    EXPECT((unsigned)out[36 + 5] == CANNY_HIP_LINE_FIT_DEGENERATE && (unsigned)out[42 + 5] == CANNY_HIP_LINE_FIT_DEGENERATE);
    EXPECT(canny_hip_line_fits_finish(nullptr, 1, out.data()) == CANNY_HIP_ERR_INVALID);
}

} // namespace

int main()
{
    designed<unsigned char>(40, 64, 1.0f, 0, 255);
    designed<short>(40, 64, 1.0f, -32768, 32767);
    designed<unsigned char>(9, 130, 2.5f, 0, 255);
    designed<short>(70, 9, 0.5f, -32768, 32767);
    tiny();
    moments_at_the_limits();
    std::vector<unsigned char> bits(8, 0), plane(64, 0);
    std::vector<float> tab(1, 1.0f);
    EXPECT(canny_hip_line_fits_from_plane(bits.data(), plane.data(), 1, 1, 8, 1.0f, 1, 19, tab.data(), tab.data(), nullptr, 0,
                                          nullptr, 0, 0, nullptr) == CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_line_fits_from_plane(bits.data(), plane.data(), 1, 2, 4, 1.0f, 1, 13, tab.data(), tab.data(), nullptr, 0,
                                          nullptr, 0, 4, nullptr) == CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_line_fits_from_plane(bits.data(), plane.data(), 1, 2, 4, 8.5f, 1, 13, tab.data(), tab.data(), nullptr, 0,
                                          nullptr, 0, 0, nullptr) == CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(canny_hip_line_fits_from_plane(bits.data(), plane.data(), 1, 2, 16385, 1.0f, 1, 13, tab.data(), tab.data(), nullptr,
                                          0, nullptr, 0, 0, nullptr) == CANNY_HIP_ERR_UNSUPPORTED);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("designed frames ok\n");
    return 0;
}
