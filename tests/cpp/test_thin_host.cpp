// Stand-alone check of csrc/canny_thin_host.cpp (own main; built by tests/test_thin_rule.py with the host compiler's address
// and undefined-behaviour sanitizers, together with that one file): both methods against a restatement written here straight
// from the definitions (a padded frame, the ring as a table), widths around the byte, frames one pixel wide or high, dirty
// pad bits, k cut below D, NULL info and refused calls -- all with buffers of exactly the needed size.
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

// One full iteration on a frame padded by one zero pixel all around; the deletions.
static long long iteration(std::vector<int> &p, int h, int w, int method)
{
    const int W = w + 2;
    static const int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dx[8] = {0, 1, 1, 1, 0, -1, -1, -1}; // P2 .. P9
    long long total = 0;
    for (int sub = 0; sub < 2; sub++) {
        std::vector<int> next = p;
        for (int y = 1; y <= h; y++)
            for (int x = 1; x <= w; x++) {
                if (!p[y * W + x]) continue;
                int r[8];
                for (int i = 0; i < 8; i++) r[i] = p[(y + dy[i]) * W + x + dx[i]];
                bool gone;
                if (method == CANNY_HIP_THIN_ZHANGSUEN) {
                    int b = 0, a = 0;
                    for (int i = 0; i < 8; i++) b += r[i], a += r[i] == 0 && r[(i + 1) % 8] == 1;
                    const int g = sub == 0 ? r[0] * r[2] * r[4] + r[2] * r[4] * r[6] : r[0] * r[2] * r[6] + r[0] * r[4] * r[6];
                    gone = b >= 2 && b <= 6 && a == 1 && g == 0;
                } else {
                    int c = 0, n1 = 0, n2 = 0;
                    for (int i = 0; i < 8; i += 2) {
                        c += !r[i] && (r[i + 1] || r[(i + 2) % 8]);
                        n1 += r[(i + 7) % 8] || r[i];
                        n2 += r[i] || r[i + 1];
                    }
                    const int m = sub == 0 ? ((r[4] || r[5] || !r[7]) && r[6]) : ((r[0] || r[1] || !r[3]) && r[2]);
                    const int n = n1 < n2 ? n1 : n2;
                    gone = c == 1 && n >= 2 && n <= 3 && !m;
                }
                if (gone) next[y * W + x] = 0, total++;
            }
        p.swap(next);
    }
    return total;
}

// one call with exact-size buffers against the restatement; density in 1/256
static int check_case(int n, int h, int w, int method, int k, uint32_t seed, unsigned density, bool with_info)
{
    const size_t rb = ((size_t)w + 7) / 8, fbytes = rb * h;
    Bytes in(fbytes * n), out(fbytes * n, 0xA5), want(fbytes * n, 0);
    for (size_t i = 0; i < in.size(); i++) { // whole bytes at the density: the pad bits are dirty
        unsigned char b = 0;
        for (int j = 0; j < 8; j++) b = (unsigned char)(b << 1 | ((lcg(seed) >> 24) < density));
        in[i] = b;
    }
    std::vector<long long> info((size_t)n * CANNY_HIP_THIN_INFO, -1), want_info((size_t)n * CANNY_HIP_THIN_INFO, 0);
    for (int f = 0; f < n; f++) {
        std::vector<int> p((size_t)(h + 2) * (w + 2), 0);
        long long in_set = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                in_set += p[(y + 1) * (w + 2) + x + 1] = (in[fbytes * f + rb * y + (x >> 3)] >> (7 - (x & 7))) & 1;
        long long it = 0, conv = 0;
        while (k == 0 || it < k) {
            std::vector<int> q = p;
            if (!iteration(q, h, w, method)) {
                conv = 1;
                break;
            }
            p.swap(q), it++;
        }
        long long set = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (p[(y + 1) * (w + 2) + x + 1]) want[fbytes * f + rb * y + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7)), set++;
        long long *r = &want_info[(size_t)f * CANNY_HIP_THIN_INFO];
        r[0] = set, r[1] = it, r[2] = in_set - set, r[3] = conv;
    }
    CHECK(canny_hip_thin_bits(in.data(), n, h, w, method, k, out.data(), with_info ? info.data() : nullptr) == CANNY_HIP_OK);
    CHECK(out == want);
    if (with_info) CHECK(info == want_info);
    return 0;
}

int main()
{
    static const int widths[] = {1, 2, 7, 8, 9, 15, 16, 17, 33, 64, 65}, heights[] = {1, 2, 3, 9, 20};
    uint32_t seed = 37;
    int cases = 0;
    for (int w : widths)
        for (int h : heights)
            for (int method = 0; method < 2; method++) {
                const int k = (w + h + method) % 4; // 0: the fixed point; 1..3: cut below D on the dense frames
                if (check_case(1 + (w + h) % 3, h, w, method, k, seed += 101, (unsigned)(120 + 30 * ((w + h) % 5)), (w + method) % 3 != 0)) return 1;
                cases++;
            }
    // thick strokes: k below, at and above D
    for (int method = 0; method < 2; method++)
        for (int k : {1, 2, 7, 8, 9, 0, CANNY_HIP_THIN_MAX_ITERATIONS})
            if (check_case(2, 19, 41, method, k, 5, 250, true)) return 1;

    // refused calls write nothing
    Bytes in(2 * 6 * 2, 0xFF), out(in.size(), 0xA5);
    std::vector<long long> info(8, -1);
    const Bytes out0 = out;
    const std::vector<long long> info0 = info;
    auto thin = [&](const unsigned char *src, int n, int h, int w, int method, int k, unsigned char *dst, long long *inf) {
        return canny_hip_thin_bits(src, n, h, w, method, k, dst, inf);
    };
    CHECK(thin(nullptr, 2, 6, 9, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 1, 0, nullptr, info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 0, 6, 9, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 0, 9, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 0, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 2, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, -1, 0, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 1, -1, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 1, CANNY_HIP_THIN_MAX_ITERATIONS + 1, out.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 1, 0, out.data(), (long long *)((char *)info.data() + 4)) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 6, 9, 1, 0, in.data(), info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 1, 6, 9, 1, 0, in.data() + 11, info.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(thin(in.data(), 2, 32769, 9, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(thin(in.data(), 2, 6, 32769, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(thin(in.data(), 65536, 6, 9, 1, 0, out.data(), info.data()) == CANNY_HIP_ERR_UNSUPPORTED);
    CHECK(out == out0 && info == info0);
    std::printf("thin ok (%d cases)\n", cases);
    return 0;
}
