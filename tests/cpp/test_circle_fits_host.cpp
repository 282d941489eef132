// test_circle_fits_host.cpp -- canny_hip_circle_fits_from_plane and canny_hip_circle_fits_finish
// (csrc/canny_circle_fits_host.cpp) on the shapes of tests/test_circle_fits_rule.py, with every buffer allocated at its exact
// size: built with the host compiler's -fsanitize=address,undefined together with that source file and
// csrc/canny_edgels_host.cpp, it shows that the host rule neither reads nor writes outside its buffers and computes without
// overflow, at the limits of the moments too.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_circle_fits_host.cpp canny_edge_amd/csrc/canny_circle_fits_host.cpp \
//       canny_edge_amd/csrc/canny_edgels_host.cpp -o test_circle_fits_host
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

uint32_t rng_state = 1357u;
uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Frame {
    int h, w;
    std::vector<unsigned char> bits;
    Frame(int h_, int w_) : h(h_), w(w_), bits((size_t)h_ * ((w_ + 7) / 8), 0) {}
    void set(int x, int y)
    {
        if (x >= 0 && x < w && y >= 0 && y < h) bits[(size_t)y * ((w + 7) / 8) + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7));
    }
    void ring(double cx, double cy, double r)
    {
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (std::fabs(std::hypot(x - cx, y - cy) - r) < 0.5) set(x, y);
    }
};

// every record with every band, three trims and options 0..3 on `plane`; the invariants every record keeps
template <class T>
void run(const Frame &f, const std::vector<T> &plane, const std::vector<int> &rec, int first_invalid)
{
    const int n_rec = (int)(rec.size() / CANNY_HIP_CIRCLE_INTS);
    for (int band = 0; band <= CANNY_HIP_CIRCLE_FIT_MAX_BAND; band++)
        for (int trim = 0; trim <= 128; trim += 64)
            for (int options = 0; options < 4; options++) {
                std::vector<int> out((size_t)n_rec * CANNY_HIP_CIRCLE_FIT_INTS);
                EXPECT(canny_hip_circle_fits_from_plane(f.bits.data(), plane.data(), sizeof(T) == 1, f.h, f.w, rec.data(), n_rec,
                                                        band, trim, options, out.data()) == CANNY_HIP_OK);
                for (int j = 0; j < n_rec; j++) {
                    const int *r = out.data() + (size_t)j * CANNY_HIP_CIRCLE_FIT_INTS, *s = rec.data() + (size_t)j * 6;
                    const unsigned flags = (unsigned)r[4];
                    if (j >= first_invalid) {
                        EXPECT(flags == CANNY_HIP_CIRCLE_FIT_INVALID);
                        for (int i = 0; i < 8; i++) EXPECT(i == 4 || r[i] == 0);
                        continue;
                    }
                    EXPECT(!(flags & CANNY_HIP_CIRCLE_FIT_INVALID) && r[3] >= 0);
                    if (flags & CANNY_HIP_CIRCLE_FIT_DEGENERATE) {
                        EXPECT(r[0] == 32768 * s[0] && r[1] == 32768 * s[1] && r[2] == 65536 * s[2]);
                        EXPECT(!r[5] && !r[6] && !r[7] && flags == CANNY_HIP_CIRCLE_FIT_DEGENERATE);
                        continue;
                    }
                    EXPECT(r[3] >= 3 && (r[5] & 0xffff) && !((unsigned)r[5] >> 16));
                    EXPECT(std::abs((long long)r[0] - 32768ll * s[0]) <= 65536ll * (band + 2));
                    EXPECT(std::abs((long long)r[1] - 32768ll * s[1]) <= 65536ll * (band + 2));
                    const unsigned long long sdd = (unsigned)r[6] | (unsigned long long)(unsigned)r[7] << 32;
                    const unsigned long long maxd = flags & CANNY_HIP_CIRCLE_FIT_MAXD_MASK;
                    EXPECT(maxd * maxd <= sdd && sdd <= (unsigned long long)r[3] * maxd * maxd);
                    EXPECT(trim > 0 || !(flags & CANNY_HIP_CIRCLE_FIT_TRIM_FAILED));
                }
            }
}

template <class T>
void designed(int h, int w, int lo, int hi)
{
    Frame f(h, w);
    const int s = h < w ? h : w;
    f.ring(w / 2.0 + 0.25, h / 2.0 - 0.25, s * 0.4);
    f.ring(w / 2.0 + 0.25, h / 2.0 - 0.25, s * 0.4 - 2.0);
    f.ring(1.0, 1.0, s * 0.3);         // clipped by two borders
    f.ring(w - 2.0, h - 2.0, s * 0.25); // ... and by the other two
    for (int x = 0; x < w; x++) f.set(x, h / 2);
    std::vector<T> plane((size_t)h * w);
    for (auto &v : plane) v = (T)(lo + (int)(rng() % (unsigned)(hi - lo + 1)));
    const int r0 = (int)(s * 0.4 + 0.5) > 0 ? (int)(s * 0.4 + 0.5) : 1;
    std::vector<int> rec = {w, h, r0, 0, 0, 0, w + 1, h - 1, r0 > 2 ? r0 - 2 : 1, 0, 0, 0, 2, 2, (int)(s * 0.3) + 1, 0, 0, 0,
                            2 * w - 4, 2 * h - 4, (int)(s * 0.25) + 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2 * w - 1, 2 * h - 1, 1024, 0, 0, 0,
                            w, h, 1, 0, 0, 0,
                            // invalid from here on
                            w, h, 0, 0, 0, 0, w, h, 1025, 0, 0, 0, -1, h, r0, 0, 0, 0, 2 * w, h, r0, 0, 0, 0, w, -1, r0, 0, 0, 0,
                            w, 2 * h, r0, 0, 0, 0, 2147483647, h, r0, 0, 0, 0, w, -2147483647 - 1, r0, 0, 0, 0,
                            w, h, -2147483647 - 1, 0, 0, 0};
    run(f, plane, rec, 7);
    // a flat plane: no gradient anywhere, the gate removes every pixel, every edgel is a pixel centre
    std::vector<T> flat((size_t)h * w, (T)77);
    run(f, flat, rec, 7);
    // every pixel set
    for (auto &b : f.bits) b = 0xff;
    run(f, plane, rec, 7);
    // no records
    EXPECT(canny_hip_circle_fits_from_plane(f.bits.data(), plane.data(), sizeof(T) == 1, h, w, nullptr, 0, 1, 0, 0, nullptr) ==
           CANNY_HIP_OK);
}

// the smallest frame
void tiny()
{
    Frame f(2, 2);
    f.set(0, 0), f.set(1, 0), f.set(0, 1), f.set(1, 1);
    const std::vector<short> plane = {-5, 5, 300, -300};
    const std::vector<int> rec = {1, 1, 1, 0, 0, 0, 3, 3, 1, 0, 0, 0, 4, 0, 1, 0, 0, 0};
    std::vector<int> out(3 * CANNY_HIP_CIRCLE_FIT_INTS);
    for (int options = 0; options < 4; options++) {
        EXPECT(canny_hip_circle_fits_from_plane(f.bits.data(), plane.data(), 0, 2, 2, rec.data(), 3, 4, 64, options, out.data()) ==
               CANNY_HIP_OK);
        EXPECT(!((unsigned)out[4] & CANNY_HIP_CIRCLE_FIT_INVALID) && (unsigned)out[16 + 4] == CANNY_HIP_CIRCLE_FIT_INVALID);
        EXPECT(options || out[3] == 4); // all four pixels lie in bin 1 of the centre (0.5, 0.5)
    }
}

void moments_at_the_limits()
{
    typedef __int128 i128;
    const long long U = 128 * 2057 + 128, Z = (1ll << 29) + (1ll << 28), N = (1ll << 17) - 1, q = N / 4;
    const i128 big = (i128)q * U * Z * 2;
    auto lo = [](i128 v) { return (long long)(unsigned long long)v; };
    auto hi = [](i128 v) { return (long long)(v >> 64); };
    const long long sets[][12] = {
        {4 * q, 0, 0, 0, 4 * q * U * U, 0, 4 * q * U * U, lo(big), hi(big), lo(-big / 2), hi(-big / 2), 4},
        {4 * q, 0, 0, 0, 4 * q * U * U, 0, 4 * q * U * U, lo(-big), hi(-big), lo(big / 2), hi(big / 2), 4},
        {4 * q, 0, 0, 0, 4 * q * U * U, 4 * q * U * U, 4 * q * U * U, lo(big), hi(big), lo(big), hi(big), 2}, // collinear
        {4 * q, 0, 0, 0, 4 * q * U * U, 0, 4 * q * U * U, lo(2 * big), hi(2 * big), lo(2 * big), hi(2 * big), 0}, // too far
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
        {2, 0, 0, 0, 50, 0, 50, 3, 0, 3, 0, 1},
        {3, 0, 0, 0, 4, 2, 1, 3, 0, -2, -1, 1},
        {4, 0, 0, 0, 256, 0, 256, 1, 0, -1, -1, 0}};
    const size_t count = sizeof(sets) / sizeof(sets[0]);
    std::vector<int> out(4 * count);
    EXPECT(canny_hip_circle_fits_finish(&sets[0][0], count, out.data()) == CANNY_HIP_OK);
    EXPECT(out[0] > 0 && out[1] < 0 && out[3] == 0 && std::abs(out[0] + 2 * out[1]) <= 2); // Svz = -Suz / 2
    EXPECT(out[4] == -out[0] && out[5] == -out[1] && out[4 + 3] == 0);
    EXPECT((unsigned)out[8 + 3] == CANNY_HIP_CIRCLE_FIT_DEGENERATE && (unsigned)out[12 + 3] == CANNY_HIP_CIRCLE_FIT_DEGENERATE);
    EXPECT((unsigned)out[16 + 3] == CANNY_HIP_CIRCLE_FIT_DEGENERATE && (unsigned)out[20 + 3] == CANNY_HIP_CIRCLE_FIT_DEGENERATE);
    EXPECT((unsigned)out[24 + 3] == CANNY_HIP_CIRCLE_FIT_DEGENERATE); // determinant 0
    EXPECT(out[28] == 1 && out[29] == -1 && out[28 + 3] == 0);         // halves away from zero
    EXPECT(canny_hip_circle_fits_finish(nullptr, 1, out.data()) == CANNY_HIP_ERR_INVALID);
}

} // namespace

int main()
{
    designed<unsigned char>(3, 5, 0, 255);
    designed<short>(97, 161, -32768, 32767);
    designed<unsigned char>(40, 300, 0, 255);
    designed<short>(300, 40, -32768, 32767);
    tiny();
    moments_at_the_limits();
    std::vector<unsigned char> bits(16, 0), plane(64, 0);
    std::vector<int> rec(6, 1), out(8, 0);
    EXPECT(canny_hip_circle_fits_from_plane(bits.data(), plane.data(), 1, 1, 8, rec.data(), 1, 0, 0, 0, out.data()) ==
           CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_circle_fits_from_plane(bits.data(), plane.data(), 1, 2, 4, rec.data(), 1, 0, 0, 4, out.data()) ==
           CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_circle_fits_from_plane(bits.data(), plane.data(), 1, 2, 4, rec.data(), 1, 5, 0, 0, out.data()) ==
           CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(canny_hip_circle_fits_from_plane(bits.data(), plane.data(), 1, 2, 16385, rec.data(), 1, 0, 0, 0, out.data()) ==
           CANNY_HIP_ERR_UNSUPPORTED);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("designed frames ok\n");
    return 0;
}
