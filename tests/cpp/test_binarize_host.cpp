// Stand-alone check of csrc/canny_binarize_host.cpp (own main; built by tests/test_binarize_rule.py with the host compiler's
// address and undefined-behaviour sanitizers, together with that one file): every method against a restatement written here
// straight from the definitions (the window summed pixel by pixel, the division-free comparison, Otsu with 128-bit ints),
// widths around the byte, frames smaller than the window, windows up to 255 x 255, both values of invert, NULL counts and
// thresholds, a histogram at the 2^26 limit and refused calls -- all with buffers of exactly the needed size.
#include "canny_hip.h"

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

static int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

static int otsu_of(const Bytes &img, size_t at, size_t n)
{
    unsigned long long hist[256] = {0};
    for (size_t i = 0; i < n; i++) hist[img[at + i]]++;
    __int128 N = 0, S = 0, w0 = 0, s0 = 0, best = -1;
    for (int i = 0; i < 256; i++) N += hist[i], S += (__int128)i * hist[i];
    int best_t = 0;
    for (int t = 0; t < 256; t++) {
        w0 += hist[t], s0 += (__int128)t * hist[t];
        const __int128 w1 = N - w0, s1 = S - s0, d = w1 * s0 - s1 * w0;
        const __int128 score = w0 * w1 == 0 ? 0 : d * d / (w0 * w1);
        if (score > best) best = score, best_t = t;
    }
    return best_t;
}

// one call with exact-size buffers against the restatement
static int check_case(int n, int h, int w, int method, int thr_or_c, int kw, int kh, int invert, uint32_t seed, int flat_step)
{
    const size_t plane = (size_t)h * w, rb = ((size_t)w + 7) / 8;
    Bytes img(plane * n), out(rb * h * n, 0xA5), want(rb * h * n, 0);
    for (size_t i = 0; i < img.size(); i++)
        img[i] = flat_step ? (unsigned char)(100 + (lcg(seed) >> 31) * flat_step) : (unsigned char)(lcg(seed) >> 24);
    std::vector<long long> counts((size_t)n, -1), want_counts((size_t)n, 0);
    std::vector<int> thr((size_t)n, -77), want_thr((size_t)n, 0);
    for (int f = 0; f < n; f++) {
        const int t = method == CANNY_HIP_BIN_OTSU ? otsu_of(img, plane * f, plane) : thr_or_c;
        want_thr[f] = t;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int v = img[plane * f + (size_t)y * w + x];
                bool cond;
                if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
                    long long S = 0;
                    for (int dy = -(kh / 2); dy <= kh / 2; dy++)
                        for (int dx = -(kw / 2); dx <= kw / 2; dx++)
                            S += img[plane * f + (size_t)clampi(y + dy, h - 1) * w + clampi(x + dx, w - 1)];
                    cond = 2 * S < (long long)kw * kh * (2 * (v + thr_or_c) - 1);
                } else {
                    cond = v > t;
                }
                if (cond != (invert != 0)) {
                    want[(rb * h) * f + rb * y + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7));
                    want_counts[f]++;
                }
            }
    }
    CHECK(canny_hip_binarize(img.data(), n, h, w, method, thr_or_c, kw, kh, invert, out.data(), counts.data(), thr.data()) ==
          CANNY_HIP_OK);
    CHECK(out == want);
    CHECK(counts == want_counts);
    CHECK(thr == want_thr);
    Bytes again(out.size(), 0x5A);
    CHECK(canny_hip_binarize(img.data(), n, h, w, method, thr_or_c, kw, kh, invert, again.data(), nullptr, nullptr) == CANNY_HIP_OK);
    CHECK(again == want);
    return 0;
}

int main()
{
    static const int widths[] = {1, 7, 8, 9, 15, 16, 17, 63, 65}, heights[] = {1, 2, 5, 31, 40};
    static const int windows[][2] = {{3, 3}, {3, 255}, {255, 3}, {31, 31}, {5, 9}};
    static const int cs[] = {-255, -1, 0, 1, 7, 255}, thrs[] = {-1, 0, 127, 254, 255};
    int k = 0;
    for (int w : widths)
        for (int h : heights) {
            const int n = 1 + k % 3, inv = k & 1;
            if (check_case(n, h, w, CANNY_HIP_BIN_FIXED, thrs[k % 5], 0, 0, inv, 17u + k, 0)) return 1;
            if (check_case(n, h, w, CANNY_HIP_BIN_OTSU, 12345, -1, 1 << 20, inv, 18u + k, k % 3 ? 0 : 10)) return 1;
            if (check_case(n, h, w, CANNY_HIP_BIN_ADAPTIVE_MEAN, cs[k % 6], windows[k % 5][0], windows[k % 5][1], inv, 19u + k, 0))
                return 1;
            if (check_case(n, h, w, CANNY_HIP_BIN_ADAPTIVE_MEAN, 1, 3, 3, 1 - inv, 20u + k, 1)) return 1; // {b, b + 1}
            k++;
        }
    if (check_case(1, 9, 12, CANNY_HIP_BIN_ADAPTIVE_MEAN, 3, 255, 255, 0, 5u, 0)) return 1;
    if (check_case(2, 1, 1, CANNY_HIP_BIN_ADAPTIVE_MEAN, 0, 255, 255, 1, 6u, 0)) return 1;

    // Otsu on histograms: flat, two values, a tie, the 2^26 limit
    unsigned long long hist[256] = {0};
    int t = -1;
    hist[77] = 1000;
    CHECK(canny_hip_otsu_from_histogram(hist, &t) == CANNY_HIP_OK && t == 0);
    hist[77] = 0, hist[10] = 5, hist[20] = 5;
    CHECK(canny_hip_otsu_from_histogram(hist, &t) == CANNY_HIP_OK && t == 10);
    hist[10] = hist[20] = 0, hist[100] = hist[110] = hist[120] = 10;
    CHECK(canny_hip_otsu_from_histogram(hist, &t) == CANNY_HIP_OK && t == 100);
    hist[100] = hist[110] = hist[120] = 0, hist[3] = 1ull << 25, hist[250] = 1ull << 25;
    CHECK(canny_hip_otsu_from_histogram(hist, &t) == CANNY_HIP_OK && t == 3);
    hist[250]++;
    t = -5;
    CHECK(canny_hip_otsu_from_histogram(hist, &t) == CANNY_HIP_ERR_UNSUPPORTED && t == -5);
    CHECK(canny_hip_otsu_from_histogram(nullptr, &t) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_otsu_from_histogram(hist, nullptr) == CANNY_HIP_ERR_INVALID);

    // refused calls write nothing
    Bytes img(6 * 9, 50), out(6 * 2, 0x5A);
    std::vector<long long> counts(1, -1);
    std::vector<int> thr(1, -77);
    auto refused = [&](int n, int h, int w, int method, int c, int kw, int kh, int invert, bool with_img, bool with_out) {
        const int st = canny_hip_binarize(with_img ? img.data() : nullptr, n, h, w, method, c, kw, kh, invert,
                                          with_out ? out.data() : nullptr, counts.data(), thr.data());
        for (unsigned char b : out)
            if (b != 0x5A) return -1;
        return counts[0] == -1 && thr[0] == -77 ? st : -1;
    };
    CHECK(refused(1, 6, 9, 3, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, -1, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_ADAPTIVE_MEAN, 0, 2, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_ADAPTIVE_MEAN, 0, 3, 257, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_ADAPTIVE_MEAN, 256, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, -2, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, 256, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 2, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(0, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, false, true) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, true, false) == CANNY_HIP_ERR_INVALID);
    CHECK(refused(65536, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(refused(1, 32769, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(refused(1, 8193, 8192, CANNY_HIP_BIN_OTSU, 0, 3, 3, 0, true, true) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(canny_hip_binarize(img.data(), 1, 6, 9, CANNY_HIP_BIN_FIXED, 0, 3, 3, 0, img.data() + 10, nullptr, nullptr) ==
          CANNY_HIP_ERR_INVALID);
    CHECK(refused(1, 6, 9, CANNY_HIP_BIN_FIXED, 49, 3, 3, 0, true, true) == -1); // a good call writes
    CHECK(counts[0] == 54 && thr[0] == 49);
    std::printf("binarize ok: %d shapes\n", k);
    return 0;
}
