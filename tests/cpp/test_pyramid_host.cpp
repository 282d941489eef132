// test_pyramid_host.cpp -- canny_hip_pyramid_layout, canny_hip_pyramid and canny_hip_pyr_up (csrc/canny_pyramid_host.cpp)
// against loops written here from the rule of include/canny_hip.h -- separated, one axis after the other, unlike the host
// rule's 25 products a pixel -- on the tiny shapes where the fold loops, with guard bytes around every output and in the pads
// between the levels, and with the refused calls.  Its own main; built with the host compiler's address and
// undefined-behaviour sanitizers by tests/test_pyramid_rule.py.  No device.
#include "canny_hip.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

typedef std::vector<unsigned char> Bytes;
const unsigned char kGuard = 0xC3;
const int kGuardBytes = 64;

unsigned rng_state = 40u;
unsigned rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int fails = 0;
void expect(bool ok, const char *what, int a = 0, int b = 0, int c = 0)
{
    if (!ok) {
        std::printf("FAIL %s (%d %d %d)\n", what, a, b, c);
        fails++;
    }
}

int fold(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// one plane h x w -> (h + 1) / 2 x (w + 1) / 2: rows first, then columns
Bytes ref_down(const Bytes &in, int h, int w)
{
    const int oh = (h + 1) / 2, ow = (w + 1) / 2, k[5] = {1, 4, 6, 4, 1};
    std::vector<int> mid((size_t)oh * w);
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int j = 0; j < 5; j++) s += k[j] * in[(size_t)fold(2 * y + j - 2, h) * w + x];
            mid[(size_t)y * w + x] = s;
        }
    Bytes out((size_t)oh * ow);
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            int s = 0;
            for (int i = 0; i < 5; i++) s += k[i] * mid[(size_t)y * w + fold(2 * x + i - 2, w)];
            out[(size_t)y * ow + x] = (unsigned char)((s + 128) >> 8);
        }
    return out;
}

// s[-1] := s[min(1, n - 1)], s[n] := s[n - 1]
int up_at(int x, int n) { return x < 0 ? (n > 1 ? 1 : 0) : (x >= n ? n - 1 : x); }

Bytes ref_up(const Bytes &in, int h, int w, int oh, int ow)
{
    std::vector<int> mid((size_t)h * ow);
    for (int y = 0; y < h; y++)
        for (int o = 0; o < ow; o++) {
            const int x = o / 2;
            const unsigned char *s = &in[(size_t)y * w];
            mid[(size_t)y * ow + o] = (o & 1) ? 4 * (s[up_at(x, w)] + s[up_at(x + 1, w)])
                                              : s[up_at(x - 1, w)] + 6 * s[up_at(x, w)] + s[up_at(x + 1, w)];
        }
    Bytes out((size_t)oh * ow);
    for (int o = 0; o < oh; o++)
        for (int x = 0; x < ow; x++) {
            const int y = o / 2;
            auto m = [&](int yy) { return mid[(size_t)up_at(yy, h) * ow + x]; };
            const int s = (o & 1) ? 4 * (m(y) + m(y + 1)) : m(y - 1) + 6 * m(y) + m(y + 1);
            out[(size_t)o * ow + x] = (unsigned char)((s + 32) >> 6);
        }
    return out;
}

int max_levels(int h, int w)
{
    int m = h > w ? h : w, l = 0;
    while ((1 << l) < m) l++;
    return l;
}

Bytes make_planes(int n, int h, int w, int kind)
{
    Bytes p((size_t)n * h * w);
    for (int f = 0; f < n; f++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int k = (kind + f) % 3;
                p[((size_t)f * h + y) * w + x] = (unsigned char)(k == 0 ? 255 : (k == 1 ? rnd() & 255 : (((x + y) & 1) ? 255 : 0)));
            }
    return p;
}

void check_pyramid(int n, int h, int w)
{
    const Bytes planes = make_planes(n, h, w, h + w);
    for (int levels = 1; levels <= max_levels(h, w); levels++) {
        long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = -1;
        expect(canny_hip_pyramid_layout(n, h, w, levels, info, &total) == CANNY_HIP_OK, "layout", h, w, levels);
        // exactly total bytes between the guards: the sanitizer sees a write behind them
        Bytes buf((size_t)total + 2 * kGuardBytes, kGuard);
        unsigned char *out = buf.data() + kGuardBytes;
        expect(canny_hip_pyramid(planes.data(), n, h, w, levels, out) == CANNY_HIP_OK, "pyramid", h, w, levels);
        std::vector<bool> level_byte((size_t)total, false);
        std::vector<Bytes> prev(n);
        int lh = h, lw = w;
        for (int f = 0; f < n; f++) prev[f].assign(planes.begin() + (size_t)f * h * w, planes.begin() + (size_t)(f + 1) * h * w);
        long long end = 0;
        for (int l = 0; l < levels; l++) {
            const int oh = (lh + 1) / 2, ow = (lw + 1) / 2;
            const long long off = info[4 * l + 2];
            expect(info[4 * l] == oh && info[4 * l + 1] == ow && info[4 * l + 3] == (long long)n * oh * ow, "level size", h, w, l);
            expect(off % 256 == 0 && off >= end && off - end < 256, "level offset", h, w, l);
            for (int f = 0; f < n; f++) {
                const Bytes want = ref_down(prev[f], lh, lw);
                for (size_t i = 0; i < want.size(); i++) {
                    const size_t at = (size_t)off + (size_t)f * oh * ow + i;
                    level_byte[at] = true;
                    if (out[at] != want[i]) {
                        expect(false, "pyrDown byte", h, w, l);
                        return;
                    }
                }
                prev[f] = want;
            }
            end = off + info[4 * l + 3];
            lh = oh, lw = ow;
        }
        expect(end == total, "total", h, w, levels);
        for (size_t i = 0; i < (size_t)total; i++)
            if (!level_byte[i] && out[i] != kGuard) {
                expect(false, "a pad byte was written", h, w, (int)i);
                return;
            }
        for (int i = 0; i < kGuardBytes; i++) expect(buf[i] == kGuard && buf[buf.size() - 1 - i] == kGuard, "guard", h, w, i);
    }
}

void check_up(int n, int h, int w)
{
    const Bytes planes = make_planes(n, h, w, h * w);
    for (int oh = 2 * h - 1; oh <= 2 * h; oh++)
        for (int ow = 2 * w - 1; ow <= 2 * w; ow++) {
            const size_t px = (size_t)oh * ow;
            Bytes buf(px * n + 2 * kGuardBytes, kGuard);
            unsigned char *out = buf.data() + kGuardBytes;
            expect(canny_hip_pyr_up(planes.data(), n, h, w, oh, ow, out) == CANNY_HIP_OK, "pyr_up", h, w, oh * 100000 + ow);
            for (int f = 0; f < n; f++) {
                const Bytes in(planes.begin() + (size_t)f * h * w, planes.begin() + (size_t)(f + 1) * h * w);
                const Bytes want = ref_up(in, h, w, oh, ow);
                for (size_t i = 0; i < px; i++)
                    if (out[f * px + i] != want[i]) {
                        expect(false, "pyrUp byte", h, w, (int)i);
                        return;
                    }
            }
            for (int i = 0; i < kGuardBytes; i++) expect(buf[i] == kGuard && buf[buf.size() - 1 - i] == kGuard, "guard", h, w, i);
        }
}

void check_refusals()
{
    const int n = 2, h = 6, w = 9;
    const Bytes planes = make_planes(n, h, w, 1);
    Bytes out(4096, kGuard);
    long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = -5;
    for (long long &v : info) v = -5;
    auto untouched = [&](const char *what) {
        for (unsigned char b : out)
            if (b != kGuard) {
                expect(false, what);
                return;
            }
        for (long long v : info) expect(v == -5, what);
        expect(total == -5, what);
    };
    const int I = CANNY_HIP_ERR_INVALID, U = CANNY_HIP_ERR_UNSUPPORTED;
    expect(canny_hip_pyramid_layout(n, h, w, 2, nullptr, &total) == I, "layout null info");
    expect(canny_hip_pyramid_layout(n, h, w, 2, info, nullptr) == I, "layout null total");
    expect(canny_hip_pyramid_layout(0, h, w, 2, info, &total) == I, "layout n 0");
    expect(canny_hip_pyramid_layout(n, 0, w, 2, info, &total) == I, "layout h 0");
    expect(canny_hip_pyramid_layout(n, h, -1, 2, info, &total) == I, "layout w -1");
    expect(canny_hip_pyramid_layout(n, h, w, 0, info, &total) == I, "layout levels 0");
    expect(canny_hip_pyramid_layout(n, h, w, 5, info, &total) == I, "layout levels 5 of 6 x 9");
    expect(canny_hip_pyramid_layout(n, h, w, 16, info, &total) == I, "layout levels 16");
    expect(canny_hip_pyramid_layout(n, 1, 1, 1, info, &total) == I, "layout of a 1 x 1 plane");
    expect(canny_hip_pyramid_layout(65536, h, w, 2, info, &total) == U, "layout frames");
    expect(canny_hip_pyramid_layout(n, 32769, w, 2, info, &total) == U, "layout h");
    expect(canny_hip_pyramid_layout(n, 32768, 65536, 2, info, &total) == U, "layout plane");
    untouched("layout refusals");
    expect(canny_hip_pyramid(nullptr, n, h, w, 2, out.data()) == I, "pyramid null in");
    expect(canny_hip_pyramid(planes.data(), n, h, w, 2, nullptr) == I, "pyramid null out");
    expect(canny_hip_pyramid(planes.data(), n, h, w, 0, out.data()) == I, "pyramid levels 0");
    expect(canny_hip_pyramid(planes.data(), n, h, w, 5, out.data()) == I, "pyramid levels 5");
    expect(canny_hip_pyramid(planes.data(), -2, h, w, 2, out.data()) == I, "pyramid n");
    expect(canny_hip_pyramid(planes.data(), n, 40000, w, 2, out.data()) == U, "pyramid h");
    expect(canny_hip_pyr_up(nullptr, n, h, w, 12, 18, out.data()) == I, "up null in");
    expect(canny_hip_pyr_up(planes.data(), n, h, w, 12, 18, nullptr) == I, "up null out");
    expect(canny_hip_pyr_up(planes.data(), n, h, w, 13, 18, out.data()) == I, "up oh");
    expect(canny_hip_pyr_up(planes.data(), n, h, w, 12, 16, out.data()) == I, "up ow");
    expect(canny_hip_pyr_up(planes.data(), n, h, w, 0, 18, out.data()) == I, "up oh 0");
    expect(canny_hip_pyr_up(planes.data(), 0, h, w, 12, 18, out.data()) == I, "up n");
    expect(canny_hip_pyr_up(planes.data(), n, 16385, w, 32770, 18, out.data()) == U, "up oh over the limit");
    expect(canny_hip_pyr_up(planes.data(), 65536, h, w, 12, 18, out.data()) == U, "up frames");
    untouched("refusals");
    // buffers that overlap: input 108 bytes, the pyramid 268, the pyrUp output 2 x 11 x 17 = 374
    Bytes both(1024, kGuard);
    expect(canny_hip_pyramid(both.data(), n, h, w, 2, both.data() + 107) == I, "pyramid overlap");
    expect(canny_hip_pyramid(both.data() + 267, n, h, w, 2, both.data()) == I, "pyramid overlap behind");
    expect(canny_hip_pyr_up(both.data() + 373, n, h, w, 11, 17, both.data()) == I, "up overlap");
    for (unsigned char b : both) expect(b == kGuard, "overlap refusals");
    expect(canny_hip_pyramid(both.data() + 268, n, h, w, 2, both.data()) == CANNY_HIP_OK, "pyramid adjacent");
    expect(canny_hip_pyr_up(both.data() + 374, n, h, w, 11, 17, both.data()) == CANNY_HIP_OK, "up adjacent");
}

} // namespace

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 3}, {3, 5}, {2, 9}, {7, 6}, {1, 7}, {5, 300}, {33, 70}};
    for (const auto &s : shapes) {
        for (int n = 1; n <= 3; n += 2) {
            check_pyramid(n, s[0], s[1]);
            check_up(n, s[0], s[1]);
        }
    }
    check_refusals();
    if (fails) {
        std::printf("%d failures\n", fails);
        return 1;
    }
    std::printf("pyramid ok\n");
    return 0;
}
