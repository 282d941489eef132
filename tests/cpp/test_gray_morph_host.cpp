// test_gray_morph_host.cpp -- canny_hip_gray_morph (csrc/canny_gray_morph_host.cpp) against a plain per-pixel loop written
// here from the rule of include/canny_hip.h, on frames smaller than the element too, with the refused calls, and the two
// selection networks of csrc/canny_gray_median.h on every input of zeros and ones.  Its own main; built with the host
// compiler's address and undefined-behaviour sanitizers by tests/test_gray_morph_rule.py.  No device.
#include "canny_gray_median.h"
#include "canny_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

typedef std::vector<unsigned char> Plane;

unsigned rng_state = 39u;
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

// kind 0 erode, 1 dilate, 2 median
Plane ref_step(const Plane &in, int h, int w, const unsigned *rows, int kw, int kh, int kind, int mode, int value)
{
    Plane out((size_t)h * w);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            std::vector<int> win;
            for (int j = 0; j < kh; j++)
                for (int i = 0; i < kw; i++) {
                    if (!((rows[j] >> i) & 1u)) continue;
                    const int dx = i - kw / 2, dy = j - kh / 2;
                    int xx = kind == 1 ? x - dx : x + dx, yy = kind == 1 ? y - dy : y + dy;
                    int v;
                    if (mode == CANNY_HIP_GRAY_BORDER_REPLICATE) {
                        xx = xx < 0 ? 0 : (xx >= w ? w - 1 : xx), yy = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
                        v = in[(size_t)yy * w + xx];
                    } else if (xx < 0 || xx >= w || yy < 0 || yy >= h) {
                        v = mode == CANNY_HIP_GRAY_BORDER_CONSTANT ? value : (kind == 0 ? 255 : 0);
                    } else {
                        v = in[(size_t)yy * w + xx];
                    }
                    win.push_back(v);
                }
            std::sort(win.begin(), win.end());
            out[(size_t)y * w + x] = (unsigned char)(kind == 0 ? win.front() : (kind == 1 ? win.back() : win[(win.size() - 1) / 2]));
        }
    return out;
}

Plane ref_chain(Plane a, int h, int w, const unsigned *rows, int kw, int kh, int kind, int mode, int value, int it)
{
    for (int i = 0; i < it; i++) a = ref_step(a, h, w, rows, kw, kh, kind, mode, value);
    return a;
}

Plane ref_sub(const Plane &a, const Plane &b)
{
    Plane r(a.size());
    for (size_t i = 0; i < a.size(); i++) r[i] = (unsigned char)(a[i] > b[i] ? a[i] - b[i] : 0);
    return r;
}

Plane ref(const Plane &in, int h, int w, int op, const unsigned *rows, int kw, int kh, int mode, int value, int it)
{
    auto e = [&](const Plane &p) { return ref_chain(p, h, w, rows, kw, kh, 0, mode, value, it); };
    auto d = [&](const Plane &p) { return ref_chain(p, h, w, rows, kw, kh, 1, mode, value, it); };
    switch (op) {
    case CANNY_HIP_GRAY_ERODE: return e(in);
    case CANNY_HIP_GRAY_DILATE: return d(in);
    case CANNY_HIP_GRAY_OPEN: return d(e(in));
    case CANNY_HIP_GRAY_CLOSE: return e(d(in));
    case CANNY_HIP_GRAY_GRADIENT: return ref_sub(d(in), e(in));
    case CANNY_HIP_GRAY_TOPHAT: return ref_sub(in, d(e(in)));
    case CANNY_HIP_GRAY_BLACKHAT: return ref_sub(e(d(in)), in);
    default: return ref_chain(in, h, w, rows, kw, kh, 2, mode, value, it);
    }
}

void compare(int n, int h, int w, int op, const unsigned *rows, int kw, int kh, int mode, int value, int it)
{
    const size_t px = (size_t)h * w;
    Plane in(px * n), out(px * n + 16, 0x5A);
    const unsigned char few[6] = {0, 1, 127, 128, 254, 255};
    for (unsigned char &v : in) v = (rnd() & 1) ? few[rnd() % 6] : (unsigned char)rnd();
    const int st = canny_hip_gray_morph(in.data(), n, h, w, op, rows, kw, kh, mode, value, it, out.data());
    expect(st == CANNY_HIP_OK, "status", st, op, kw);
    for (int f = 0; f < n; f++) {
        const Plane want = ref(Plane(in.begin() + f * px, in.begin() + (f + 1) * px), h, w, op, rows, kw, kh, mode, value, it);
        expect(std::equal(want.begin(), want.end(), out.begin() + f * px), "bytes", op, kw * 100 + kh, mode * 1000 + h * 10 + w);
    }
    for (size_t i = px * n; i < out.size(); i++) expect(out[i] == 0x5A, "guard bytes");
}

int refused(const unsigned char *in, int n, int h, int w, int op, const unsigned *rows, int kw, int kh, int mode, int value, int it,
            bool with_out = true)
{
    Plane out(256, 0x5A);
    const int st = canny_hip_gray_morph(in, n, h, w, op, rows, kw, kh, mode, value, it, with_out ? out.data() : nullptr);
    if (st != CANNY_HIP_OK)
        for (unsigned char v : out) expect(v == 0x5A, "a refused call wrote something", st);
    return st;
}

#define ZERO_ONE(a, b)                                                                                                           \
    {                                                                                                                            \
        const uint64_t lo = p[a] & p[b], hi = p[a] | p[b];                                                                       \
        p[a] = lo, p[b] = hi;                                                                                                    \
    }

// 64 inputs a word: the low six input bits are the six masks, the others come from the counter
void networks()
{
    const uint64_t base[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                              0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    long bad = 0;
    for (uint32_t v = 0; v < 512; v++) {
        uint64_t p[9];
        for (int i = 0; i < 9; i++) p[i] = (v >> i) & 1u;
        CANNY_GRAY_MED9_NET(ZERO_ONE)
        bad += p[CANNY_GRAY_MED9_OUT] != (uint64_t)(__builtin_popcount(v) >= 5);
    }
    expect(!bad, "the 3 x 3 network", (int)bad);
    bad = 0;
    for (uint32_t hi = 0; hi < (1u << 19); hi++) {
        uint64_t p[25];
        for (int i = 0; i < 6; i++) p[i] = base[i];
        for (int i = 6; i < 25; i++) p[i] = ((hi >> (i - 6)) & 1u) ? ~0ull : 0ull;
        // at least 13 ones among the 25: 13 - popcount(hi) or more among the low six
        const int need = 13 - __builtin_popcount(hi);
        uint64_t want = 0;
        for (int l = 0; l < 64; l++) want |= (uint64_t)(__builtin_popcount((unsigned)l) >= need) << l;
        CANNY_GRAY_MED25_NET(ZERO_ONE)
        bad += p[CANNY_GRAY_MED25_OUT] != want;
    }
    expect(!bad, "the 5 x 5 network", (int)bad);
}

} // namespace

int main()
{
    const unsigned rect3[3] = {7, 7, 7}, rect5[5] = {31, 31, 31, 31, 31}, ell[5] = {0x04, 0x0E, 0x1F, 0x0E, 0x04};
    const unsigned asym[3] = {0x03, 0x0E, 0x18}; // 5 x 3, no symmetry: the reflection of the dilation shows
    const unsigned far_bit[5] = {1u << 6, 0, 0, 0, 0}; // 7 x 5: the single offset (+3, -2)
    unsigned rect31[31], rand31[31];
    for (int j = 0; j < 31; j++) rect31[j] = 0x7FFFFFFFu, rand31[j] = (rnd() * 2654435761u) & 0x7FFFFFFFu;
    rand31[7] |= 1u;
    const int modes[5][2] = {{0, 0}, {1, 0}, {2, 0}, {2, 255}, {2, 77}};
    int k = 0;
    for (const auto &m : modes)
        for (int op = CANNY_HIP_GRAY_ERODE; op <= CANNY_HIP_GRAY_BLACKHAT; op++, k++) {
            compare(2, 7, 11, op, rect3, 3, 3, m[0], m[1], 1 + k % 2);
            compare(1, 9, 6, op, asym, 5, 3, m[0], m[1], 1 + k % 3);
            compare(1, 6, 9, op, ell, 5, 5, m[0], m[1], 1);
            compare(1, 8, 8, op, far_bit, 7, 5, m[0], m[1], 2);
            // frames smaller than the element
            compare(2, 1, 1, op, rect31, 31, 31, m[0], m[1], (1 + k % 2) * 8);
            compare(1, 3, 2, op, rand31, 31, 31, m[0], m[1], 2);
            compare(1, 2, 3, op, rect5, 5, 5, m[0], m[1], 16);
        }
    for (int m = 1; m < 5; m++) {
        compare(2, 7, 11, CANNY_HIP_GRAY_MEDIAN, rect3, 3, 3, modes[m][0], modes[m][1], 1);
        compare(2, 6, 9, CANNY_HIP_GRAY_MEDIAN, rect5, 5, 5, modes[m][0], modes[m][1], 2);
        compare(3, 2, 3, CANNY_HIP_GRAY_MEDIAN, rect5, 5, 5, modes[m][0], modes[m][1], 16);
        compare(1, 1, 1, CANNY_HIP_GRAY_MEDIAN, rect3, 3, 3, modes[m][0], modes[m][1], 3);
    }

    // refusals: nothing is written
    Plane in(256, 9);
    const unsigned bad_bit[3] = {7, 8, 7}, empty[3] = {0, 0, 0}, holed[3] = {7, 5, 7};
    const int I = CANNY_HIP_ERR_INVALID, U = CANNY_HIP_ERR_UNSUPPORTED;
    expect(refused(in.data(), 2, 6, 9, CANNY_HIP_GRAY_OPEN, rect3, 3, 3, 0, 0, 1) == CANNY_HIP_OK, "a good call");
    expect(refused(nullptr, 2, 6, 9, 2, rect3, 3, 3, 0, 0, 1) == I, "NULL input");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 0, 0, 1, false) == I, "NULL output");
    expect(refused(in.data(), 2, 6, 9, 2, nullptr, 3, 3, 0, 0, 1) == I, "NULL rows");
    expect(refused(in.data(), 0, 6, 9, 2, rect3, 3, 3, 0, 0, 1) == I, "no frames");
    expect(refused(in.data(), 2, 0, 9, 2, rect3, 3, 3, 0, 0, 1) == I, "h = 0");
    expect(refused(in.data(), 2, 6, 0, 2, rect3, 3, 3, 0, 0, 1) == I, "w = 0");
    expect(refused(in.data(), 2, 6, 9, -1, rect3, 3, 3, 0, 0, 1) == I, "op -1");
    expect(refused(in.data(), 2, 6, 9, 8, rect3, 3, 3, 0, 0, 1) == I, "op 8");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 3, 0, 1) == I, "mode 3");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, -1, 0, 1) == I, "mode -1");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 2, 256, 1) == I, "value 256");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 2, -1, 1) == I, "value -1");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 1, 999, 1) == CANNY_HIP_OK, "value ignored by REPLICATE");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 0, 0, 0) == I, "0 iterations");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 3, 3, 0, 0, 17) == I, "17 iterations");
    expect(refused(in.data(), 2, 6, 9, 2, bad_bit, 3, 3, 0, 0, 1) == I, "a bit at kw");
    expect(refused(in.data(), 2, 6, 9, 2, empty, 3, 3, 0, 0, 1) == I, "an empty element");
    expect(refused(in.data(), 2, 6, 9, 2, rect3, 2, 3, 0, 0, 1) == I, "even kw");
    expect(refused(in.data(), 2, 6, 9, 2, rect31, 33, 3, 0, 0, 1) == I, "kw 33");
    expect(refused(in.data(), 2, 6, 9, 7, rect3, 3, 3, 0, 0, 1) == I, "MEDIAN under NEUTRAL");
    expect(refused(in.data(), 2, 6, 9, 7, holed, 3, 3, 1, 0, 1) == I, "MEDIAN of a ring");
    expect(refused(in.data(), 2, 6, 9, 7, rect31, 7, 7, 1, 0, 1) == I, "MEDIAN 7 x 7");
    expect(refused(in.data(), 2, 6, 9, 7, rect5, 5, 3, 1, 0, 1) == I, "MEDIAN 5 x 3");
    expect(refused(in.data(), 2, 32769, 9, 2, rect3, 3, 3, 0, 0, 1) == U, "h 32769");
    expect(refused(in.data(), 2, 6, 32769, 2, rect3, 3, 3, 0, 0, 1) == U, "w 32769");
    expect(refused(in.data(), 65536, 6, 9, 2, rect3, 3, 3, 0, 0, 1) == U, "65536 frames");
    Plane buf(400, 0x5A);
    expect(canny_hip_gray_morph(buf.data(), 2, 6, 9, 2, rect3, 3, 3, 0, 0, 1, buf.data() + 107) == I, "overlap");
    expect(canny_hip_gray_morph(buf.data() + 20, 2, 6, 9, 2, rect3, 3, 3, 0, 0, 1, buf.data()) == I, "overlap");
    for (unsigned char v : buf) expect(v == 0x5A, "an overlapping call wrote something");

    networks();
    if (fails) return 1;
    std::printf("gray morph ok\n");
    return 0;
}
