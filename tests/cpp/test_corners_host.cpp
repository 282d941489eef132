// test_corners_host.cpp -- canny_hip_corners_from_plane (csrc/canny_corners_host.cpp) on the shapes of
// tests/test_corners_rule.py, with every buffer allocated at its exact size: built with the host compiler's
// -fsanitize=address,undefined together with that one source file, it shows that the host rule neither reads nor writes
// outside its buffers and computes without overflow.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_corners_host.cpp canny_edge_amd/csrc/canny_corners_host.cpp -o test_corners_host
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

uint32_t rng_state = 2929u;
uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// the 1-4-6-4-1 binomial both ways, edges replicated, floor(/256)
std::vector<unsigned char> blur(const std::vector<unsigned char> &p, int h, int w)
{
    const int k[5] = {1, 4, 6, 4, 1};
    std::vector<int> t((size_t)h * w);
    std::vector<unsigned char> out((size_t)h * w);
    auto clamp = [](int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int i = 0; i < 5; i++) s += k[i] * p[(size_t)y * w + clamp(x + i - 2, w)];
            t[(size_t)y * w + x] = s;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int i = 0; i < 5; i++) s += k[i] * t[(size_t)clamp(y + i - 2, h) * w + x];
            out[(size_t)y * w + x] = (unsigned char)(s / 256);
        }
    return out;
}

struct Result {
    std::vector<long long> rec;
    int count = -1, cands = -1;
    long long rmax = 0;
};

// one call with exact-size buffers, and the invariants every result keeps
Result run(const std::vector<unsigned char> &plane, int h, int w, int mode, int block, int k_q8, int q16, int min_dist,
           int corners_max, bool with_response)
{
    Result r;
    r.rec.assign((size_t)corners_max * CANNY_HIP_CORNER_WORDS, -1);
    std::vector<long long> resp(with_response ? (size_t)h * w : 0);
    EXPECT(canny_hip_corners_from_plane(plane.data(), h, w, mode, block, k_q8, q16, 0, min_dist, corners_max, r.rec.data(),
                                        &r.count, &r.cands, &r.rmax, with_response ? resp.data() : nullptr) == CANNY_HIP_OK);
    EXPECT(r.count >= 0 && r.count <= corners_max && r.count <= r.cands);
    long long prev_rank = -1, prev_resp = 0;
    for (int j = 0; j < r.count; j++) {
        const long long *c = &r.rec[(size_t)j * CANNY_HIP_CORNER_WORDS];
        EXPECT(c[0] >= 0 && c[0] < w && c[1] >= 0 && c[1] < h);
        EXPECT(c[2] >= 1 && c[2] <= r.rmax);
        EXPECT(c[3] > prev_rank && c[3] < corners_max && c[3] < r.cands);
        EXPECT(j == 0 || c[2] <= prev_resp);
        if (with_response) EXPECT(resp[(size_t)c[1] * w + c[0]] == c[2]);
        for (int i = 0; i < j; i++) {
            const long long dx = c[0] - r.rec[(size_t)i * 4], dy = c[1] - r.rec[(size_t)i * 4 + 1];
            EXPECT(dx * dx + dy * dy >= (long long)min_dist * min_dist);
        }
        prev_rank = c[3], prev_resp = c[2];
    }
    for (size_t i = (size_t)r.count * CANNY_HIP_CORNER_WORDS; i < r.rec.size(); i++) EXPECT(r.rec[i] == -1);
    if (with_response) {
        long long m = resp[0];
        for (long long v : resp) m = v > m ? v : m;
        EXPECT(m == r.rmax);
    }
    return r;
}

} // namespace

int main()
{
    const int modes[2][2] = {{CANNY_HIP_CORNERS_MIN_EIGEN, 0}, {CANNY_HIP_CORNERS_HARRIS, 10}};
    const int shapes[][2] = {{2, 2}, {2, 70}, {70, 2}, {9, 11}, {41, 57}};
    for (const auto &m : modes)
        for (int block = 3; block <= 7; block += 2) {
            for (const auto &s : shapes) {
                std::vector<unsigned char> p((size_t)s[0] * s[1]);
                for (auto &v : p) v = (unsigned char)rng();
                run(p, s[0], s[1], m[0], block, m[1], 3000, 5, 64, true);
                run(p, s[0], s[1], m[0], block, m[1], 0, 0, 1, false);
                // the extremes of the domain: a 0 / 255 board of single pixels
                for (size_t i = 0; i < p.size(); i++) p[i] = (unsigned char)((((i / s[1]) + (i % s[1])) & 1) ? 255 : 0);
                run(p, s[0], s[1], m[0], block, m[1], 65536, 0, 4096, true);
            }
            // a flat plane
            const Result flat = run(std::vector<unsigned char>(12 * 19, 77), 12, 19, m[0], block, m[1], 0, 0, 8, true);
            EXPECT(flat.count == 0 && flat.cands == 0 && flat.rmax == 0);
            // the square: four corners
            std::vector<unsigned char> sq(64 * 64, 0);
            for (int y = 20; y < 44; y++)
                for (int x = 20; x < 44; x++) sq[(size_t)y * 64 + x] = 200;
            const Result four = run(blur(sq, 64, 64), 64, 64, m[0], block, m[1], 655, 0, 256, true);
            EXPECT(four.count == 4 && four.cands == 4);
            for (int j = 0; j < four.count; j++)
                for (int a = 0; a < 2; a++) {
                    const long long v = four.rec[(size_t)j * 4 + a];
                    EXPECT(llabs(v - 20) <= 2 || llabs(v - 43) <= 2);
                }
        }
    // the checkerboard: 196 candidates in two groups of 98 equal responses
    std::vector<unsigned char> board(64 * 64);
    for (int y = 0; y < 64; y++)
        for (int x = 0; x < 64; x++) board[(size_t)y * 64 + x] = (unsigned char)((((y / 8) + (x / 8)) & 1) * 200);
    board = blur(board, 64, 64);
    for (const auto &m : modes) {
        const int cuts[] = {50, 98, 99, 150, 4096};
        for (int cmax : cuts)
            for (int md : {0, 6, 9}) {
                const Result r = run(board, 64, 64, m[0], 5, m[1], 655, md, cmax, false);
                EXPECT(r.cands == 196);
                if (md == 0) EXPECT(r.count == (cmax < 196 ? cmax : 196));
                else EXPECT(r.count > 0 && r.count < (cmax < 196 ? cmax : 196)); // four candidates round a crossing, 5 px apart
                if (cmax == 4096 && md == 0) EXPECT(r.rec[97 * 4 + 2] > r.rec[98 * 4 + 2] && r.rec[98 * 4 + 2] == r.rec[195 * 4 + 2]);
            }
    }
    // refused calls write nothing
    long long rec[4] = {-1, -1, -1, -1};
    int count = -7;
    const unsigned char tiny[4] = {0, 255, 255, 0};
    EXPECT(canny_hip_corners_from_plane(tiny, 1, 4, 0, 3, 0, 0, 0, 0, 1, rec, &count, nullptr, nullptr, nullptr) == CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_corners_from_plane(tiny, 2, 2, 0, 4, 0, 0, 0, 0, 1, rec, &count, nullptr, nullptr, nullptr) == CANNY_HIP_ERR_INVALID);
    EXPECT(canny_hip_corners_from_plane(tiny, 2, 2, 0, 3, 0, 0, 0, 0, 4097, rec, &count, nullptr, nullptr, nullptr) == CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(canny_hip_corners_from_plane(tiny, 65536, 32768, 0, 3, 0, 0, 0, 0, 1, rec, &count, nullptr, nullptr, nullptr) == CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(count == -7 && rec[0] == -1 && rec[3] == -1);
    long long r = 0;
    EXPECT(canny_hip_corner_response_of(CANNY_HIP_CORNERS_MAX_SUM, CANNY_HIP_CORNERS_MAX_SUM, -CANNY_HIP_CORNERS_MAX_SUM, 1, 64, &r) == CANNY_HIP_OK);
    EXPECT(canny_hip_corner_response_of(0, CANNY_HIP_CORNERS_MAX_SUM, CANNY_HIP_CORNERS_MAX_SUM, 0, 0, &r) == CANNY_HIP_OK);
    EXPECT(canny_hip_corner_response_of(0, CANNY_HIP_CORNERS_MAX_SUM + 1, 0, 0, 0, &r) == CANNY_HIP_ERR_INVALID);
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("designed planes ok\n");
    return 0;
}
