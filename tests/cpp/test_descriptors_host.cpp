// Stand-alone check of csrc/canny_descriptors_host.cpp (own main; built by tests/test_descriptors_rule.py with the host
// compiler's address and undefined-behaviour sanitizers, together with that one file): the pattern's bounds, planes whose
// descriptors are known, records on and outside the frame's border with buffers of exactly the needed size, the matcher on
// designed sets, and refused calls.
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

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main()
{
    // the pattern: bounded, both ends distinct
    std::vector<signed char> pat(CANNY_HIP_DESC_BITS * 4);
    for (int k = 0; k < CANNY_HIP_DESC_ROTATIONS; k++) {
        CHECK(canny_hip_descriptor_pattern(k, pat.data()) == CANNY_HIP_OK);
        for (int t = 0; t < CANNY_HIP_DESC_BITS; t++) {
            const signed char *p = &pat[(size_t)t * 4];
            for (int c = 0; c < 4; c++) CHECK(p[c] >= -13 && p[c] <= 13);
            CHECK(p[0] != p[2] || p[1] != p[3]);
        }
    }
    CHECK(canny_hip_descriptor_pattern(-1, pat.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_descriptor_pattern(32, pat.data()) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_descriptor_pattern(0, nullptr) == CANNY_HIP_ERR_INVALID);

    // descriptors: frames from 2 x 2, records in every corner and outside, exact-size buffers
    const int shapes[][2] = {{2, 2}, {2, 70}, {70, 2}, {16, 31}, {40, 52}};
    uint32_t seed = 12345;
    for (const auto &sh : shapes) {
        const int h = sh[0], w = sh[1];
        std::vector<unsigned char> plane((size_t)h * w);
        for (auto &v : plane) v = (unsigned char)(lcg(seed) >> 24);
        const long long xs[] = {0, w - 1, w / 2, -1, w, 1ll << 40}, ys[] = {0, h - 1, h / 2, -1, h, -(1ll << 40)};
        std::vector<long long> rec;
        for (long long y : ys)
            for (long long x : xs) rec.insert(rec.end(), {x, y, 0, 0});
        const int n = (int)rec.size() / 4;
        for (int options = 0; options < 2; options++) {
            std::vector<unsigned long long> desc((size_t)n * 4, 0x5a5a5a5a5a5a5a5aull);
            std::vector<int> meta((size_t)n, -7);
            CHECK(canny_hip_corner_descriptors_from_plane(plane.data(), h, w, rec.data(), n, options, desc.data(),
                                                          meta.data()) == CANNY_HIP_OK);
            for (int c = 0; c < n; c++) {
                const long long x = rec[(size_t)c * 4], y = rec[(size_t)c * 4 + 1];
                const bool inside = x >= 0 && x < w && y >= 0 && y < h;
                if (!inside) {
                    CHECK(meta[c] == -1 && !desc[c * 4] && !desc[c * 4 + 1] && !desc[c * 4 + 2] && !desc[c * 4 + 3]);
                    continue;
                }
                const bool border = x < 15 || y < 15 || x + 15 > w - 1 || y + 15 > h - 1;
                CHECK(meta[c] >= 0 && (meta[c] >> 8) == (border ? 1 : 0) && (meta[c] & 255) < 32);
                if (!options) CHECK((meta[c] & 255) == 0);
            }
            // a flat plane: k = 0 and all-zero words
            std::vector<unsigned char> flat((size_t)h * w, 77);
            CHECK(canny_hip_corner_descriptors_from_plane(flat.data(), h, w, rec.data(), n, options, desc.data(),
                                                          meta.data()) == CANNY_HIP_OK);
            for (int c = 0; c < n; c++) {
                CHECK(meta[c] == -1 || (meta[c] & 255) == 0);
                CHECK(!desc[c * 4] && !desc[c * 4 + 1] && !desc[c * 4 + 2] && !desc[c * 4 + 3]);
            }
        }
    }
    // a vertical step edge, upright: a test's bit is set iff its first end lies left of the edge and its second does not
    {
        const int h = 40, w = 40;
        std::vector<unsigned char> plane((size_t)h * w);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) plane[(size_t)y * w + x] = x < 20 ? 10 : 200;
        const long long rec[4] = {20, 20, 0, 0};
        unsigned long long desc[4];
        int meta = -7;
        CHECK(canny_hip_corner_descriptors_from_plane(plane.data(), h, w, rec, 1, 0, desc, &meta) == CANNY_HIP_OK);
        CHECK(meta == 0);
        CHECK(canny_hip_descriptor_pattern(0, pat.data()) == CANNY_HIP_OK);
        for (int t = 0; t < CANNY_HIP_DESC_BITS; t++) {
            const bool want = pat[(size_t)t * 4] < 0 && pat[(size_t)t * 4 + 2] >= 0;
            CHECK(((desc[t / 64] >> (t % 64)) & 1) == (want ? 1u : 0u));
        }
        // steered: the centroid lies to the right (+x): k = 0; the transposed plane: +y, k = 8
        CHECK(canny_hip_corner_descriptors_from_plane(plane.data(), h, w, rec, 1, CANNY_HIP_DESC_STEERED, desc, &meta) ==
              CANNY_HIP_OK);
        CHECK(meta == 0);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) plane[(size_t)y * w + x] = y < 20 ? 10 : 200;
        CHECK(canny_hip_corner_descriptors_from_plane(plane.data(), h, w, rec, 1, CANNY_HIP_DESC_STEERED, desc, &meta) ==
              CANNY_HIP_OK);
        CHECK(meta == 8);
    }
    // refused: nothing written
    {
        unsigned char plane[4] = {1, 2, 3, 4};
        const long long rec[4] = {0, 0, 0, 0};
        unsigned long long desc[4] = {9, 9, 9, 9};
        int meta = -7;
        CHECK(canny_hip_corner_descriptors_from_plane(nullptr, 2, 2, rec, 1, 0, desc, &meta) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_corner_descriptors_from_plane(plane, 1, 2, rec, 1, 0, desc, &meta) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_corner_descriptors_from_plane(plane, 2, 2, rec, 1, 2, desc, &meta) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_corner_descriptors_from_plane(plane, 2, 2, rec, 4097, 0, desc, &meta) == CANNY_HIP_ERR_UNSUPPORTED);
        CHECK(desc[0] == 9 && desc[3] == 9 && meta == -7);
    }

    // the matcher: exact-size buffers, counts on both sides of 64 and 256
    const int sizes[] = {0, 1, 2, 63, 64, 65, 257, 300};
    for (int nq : sizes)
        for (int nt : sizes) {
            std::vector<unsigned long long> q((size_t)nq * 4), t((size_t)nt * 4);
            for (auto &v : q) v = ((unsigned long long)lcg(seed) << 32) | lcg(seed);
            for (size_t i = 0; i < t.size(); i++) {
                if (q.empty()) t[i] = lcg(seed);
                else t[i] = i < q.size() ? q[i] ^ (1ull << (i % 64)) : ~q[i % q.size()];
            }
            std::vector<int> m((size_t)nq * 4, -7);
            int acc = -7;
            CHECK(canny_hip_match_descriptors(nq ? q.data() : nullptr, nq, nt ? t.data() : nullptr, nt, 64, 205,
                                              CANNY_HIP_MATCH_CROSS_CHECK, nq ? m.data() : nullptr, &acc) == CANNY_HIP_OK);
            int n_acc = 0;
            for (int i = 0; i < nq; i++) {
                const int *r = &m[(size_t)i * 4];
                if (!nt) CHECK(r[0] == -1 && r[1] == 257 && r[2] == 257 && !(r[3] & 4));
                else CHECK(r[0] >= 0 && r[0] < nt && r[1] <= r[2] && r[1] <= 256);
                if (i < nt) CHECK(r[0] == i && r[1] == 4 && (r[3] & 5) == 5); // its own copy with four bits flipped
                if (nt == 1) CHECK(r[2] == 257);
                n_acc += r[3] >> 3 & 1;
            }
            CHECK(acc == n_acc);
        }
    {   // duplicates: the smaller index, d2 == d1
        const unsigned long long t[12] = {1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8}, q[8] = {1, 2, 3, 4, 1, 2, 3, 4};
        int m[8], acc = -7;
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 256, 205, 1, m, &acc) == CANNY_HIP_OK);
        CHECK(m[0] == 0 && m[1] == 0 && m[2] == 0 && m[3] == (1 | 4) && m[4] == 0 && m[7] == 1 && acc == 0);
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 256, 0, 1, m, &acc) == CANNY_HIP_OK);
        CHECK(m[3] == 15 && m[7] == 3 && acc == 1);
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 256, 0, 0, m, &acc) == CANNY_HIP_OK && acc == 2);
        int keep[8];
        for (int i = 0; i < 8; i++) keep[i] = m[i];
        acc = -7;
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 257, 0, 0, m, &acc) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 64, 257, 0, m, &acc) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_match_descriptors(q, 2, t, 3, 64, 0, 2, m, &acc) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_match_descriptors(q, 2, nullptr, 3, 64, 0, 0, m, &acc) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_match_descriptors(q, 4097, t, 3, 64, 0, 0, m, &acc) == CANNY_HIP_ERR_UNSUPPORTED);
        for (int i = 0; i < 8; i++) CHECK(keep[i] == m[i]);
        CHECK(acc == -7);
    }
    std::printf("descriptors ok\n");
    return 0;
}
