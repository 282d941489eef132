// test_chamfer_host.cpp -- canny_hip_chamfer_from_dist2 and canny_hip_chamfer_cost_of (csrc/canny_chamfer_host.cpp) on
// designed frames, with every buffer allocated at exactly the size the header promises, so that the host compiler's
// address and undefined-behaviour sanitizers see any access past an end.  Has its own main; compiled together with
// canny_chamfer_host.cpp alone (tests/test_chamfer_rule.py): no device, nothing loaded into an interpreter.
#include "canny_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

int fails = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            fails++;                                                   \
        }                                                              \
    } while (0)

uint64_t isqrt_slow(uint64_t v)
{
    uint64_t r = 0;
    for (uint64_t bit = 1ull << 31; bit; bit >>= 1)
        if ((r + bit) * (r + bit) <= v) r += bit;
    return r;
}

// exact-size heap copies: the sanitizer's red zones start right behind the last element
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

std::vector<int> dist2_of(const std::vector<int> &mask, int h, int w)
{
    std::vector<int> d((size_t)h * w, CANNY_HIP_EDT_NONE);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int yy = 0; yy < h; yy++)
                for (int xx = 0; xx < w; xx++)
                    if (mask[(size_t)yy * w + xx])
                        d[(size_t)y * w + x] = std::min(d[(size_t)y * w + x], (y - yy) * (y - yy) + (x - xx) * (x - xx));
    return d;
}

void frame(int h, int w, unsigned seed, int density_pct, const std::vector<int> &offsets, const std::vector<short> &points,
           int trunc, int max_mean, int min_dist, int matches_max, bool with_scores, bool with_matches)
{
    std::vector<int> mask((size_t)h * w);
    for (auto &m : mask) {
        seed = seed * 1664525u + 1013904223u;
        m = (int)((seed >> 16) % 100u) < density_pct;
    }
    const int T = (int)offsets.size() - 1;
    auto d2 = exact(dist2_of(mask, h, w));
    auto off = exact(offsets);
    auto pts = exact(points);
    std::unique_ptr<int[]> rec(new int[(size_t)matches_max * CANNY_HIP_MATCH_INTS]);
    std::fill(rec.get(), rec.get() + (size_t)matches_max * CANNY_HIP_MATCH_INTS, -7);
    std::unique_ptr<unsigned[]> S(new unsigned[(size_t)T * h * w]);
    int count = -1, cands = -1;
    const int rc = canny_hip_chamfer_from_dist2(d2.get(), h, w, off.get(), pts.get(), T, trunc, max_mean, min_dist,
                                                matches_max, with_matches ? rec.get() : nullptr, &count, &cands,
                                                with_scores ? S.get() : nullptr);
    CHECK(rc == CANNY_HIP_OK);
    CHECK(count >= 0 && count <= matches_max && cands >= count);
    if (with_scores) // the sums, by the definition
        for (int t = 0; t < T; t++)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    unsigned sum = 0;
                    for (int k = offsets[t]; k < offsets[t + 1]; k++) {
                        const int px = x + points[2 * k], py = y + points[2 * k + 1];
                        const bool in = px >= 0 && px < w && py >= 0 && py < h;
                        sum += in ? (unsigned)std::min<uint64_t>(isqrt_slow((uint64_t)(unsigned)d2[(size_t)py * w + px] * 256u),
                                                                 (uint64_t)trunc)
                                  : (unsigned)trunc;
                    }
                    CHECK(S[((size_t)t * h + y) * w + x] == sum);
                }
    if (with_matches) {
        for (int j = 0; j < count; j++) {
            const int *r = rec.get() + (size_t)j * CANNY_HIP_MATCH_INTS;
            CHECK(r[0] >= 0 && r[0] < w && r[1] >= 0 && r[1] < h && r[2] >= 0 && r[2] < T);
            CHECK(r[5] == (r[2] * h + r[1]) * w + r[0]);
            const int K = offsets[r[2] + 1] - offsets[r[2]];
            CHECK(r[3] <= max_mean * K && r[4] == (int)((int64_t)r[3] * 256 / K));
            if (with_scores) CHECK((unsigned)r[3] == S[(size_t)r[5]]);
            if (j) {
                const int *q = r - CANNY_HIP_MATCH_INTS;
                CHECK(q[4] < r[4] || (q[4] == r[4] && q[5] < r[5]));
            }
            for (int i = 0; i < j; i++) {
                const int *q = rec.get() + (size_t)i * CANNY_HIP_MATCH_INTS;
                CHECK((q[0] - r[0]) * (q[0] - r[0]) + (q[1] - r[1]) * (q[1] - r[1]) >= min_dist * min_dist);
            }
        }
        for (size_t i = (size_t)count * CANNY_HIP_MATCH_INTS; i < (size_t)matches_max * CANNY_HIP_MATCH_INTS; i++)
            CHECK(rec[i] == -7); // later slots are not written
    }
}

} // namespace

int main()
{
    // cost: boundaries of the root, the truncation, the "no edge pixel" value
    for (int q = 1; q <= 5000; q++) {
        const int64_t up = ((int64_t)q * q + 255) / 256;
        for (int64_t d2 = std::max<int64_t>(0, up - 1); d2 <= up; d2++)
            CHECK(canny_hip_chamfer_cost_of((int)d2, 4095) == (int)std::min<uint64_t>(isqrt_slow((uint64_t)d2 * 256u), 4095));
    }
    CHECK(canny_hip_chamfer_cost_of(CANNY_HIP_EDT_NONE, 160) == 160);
    CHECK(canny_hip_chamfer_cost_of(0, 1) == 0 && canny_hip_chamfer_cost_of(1, 1) == 1);
    CHECK(canny_hip_chamfer_cost_of(-1, 160) == -1 && canny_hip_chamfer_cost_of(4, 0) == -1 &&
          canny_hip_chamfer_cost_of(4, 4096) == -1);

    const std::vector<int> one_off{0, 1};
    const std::vector<short> one_pts{0, 0};
    // three templates: a single point, an L with a duplicate and negative offsets, one that reaches the extent limit
    const std::vector<int> off3{0, 1, 7, 11};
    const std::vector<short> pts3{0, 0, /**/ -2, -1, -2, 0, -2, 1, -1, 1, 0, 1, 0, 1, /**/ -255, 0, 255, 0, 0, -255, 0, 255};
    frame(1, 1, 1u, 100, one_off, one_pts, 1, 0, 0, 1, true, true);
    frame(1, 1, 2u, 0, one_off, one_pts, 4095, 4094, 0, 1, true, true);
    frame(1, 9, 3u, 30, off3, pts3, 160, 100, 2, 4, true, true);
    frame(9, 1, 4u, 30, off3, pts3, 160, 100, 0, 4096, true, true);
    frame(12, 17, 5u, 10, off3, pts3, 160, 120, 3, 5, true, true);
    frame(12, 17, 6u, 10, off3, pts3, 255, 200, 3, 5, false, true);
    frame(11, 13, 7u, 50, off3, pts3, 256, 128, 1, 7, true, false);
    frame(7, 5, 8u, 0, off3, pts3, 33, 32, 1, 7, true, true);
    frame(7, 5, 9u, 100, off3, pts3, 33, 32, 100, 7, true, true);

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("designed frames ok\n");
    return 0;
}
