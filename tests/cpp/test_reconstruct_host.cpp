// test_reconstruct_host.cpp -- canny_hip_reconstruct_bits (csrc/canny_reconstruct_host.cpp) on its own, for the host compiler's
// sanitizers: random maps of awkward shapes against an iterated geodesic dilation written here, guard bytes around every
// buffer, the documented numbers of the diamond ring, and the refused calls.  Compiled by tests/test_reconstruct_rule.py; no
// device, nothing of the library but that one file.
#include "canny_hip.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond) && fails++ < 20) printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

typedef std::vector<unsigned char> Px;

static Px propagate(const Px &start, const Px &g, int h, int w, int c)
{
    Px s(start.size());
    for (size_t i = 0; i < s.size(); i++) s[i] = start[i] && g[i];
    for (bool moved = true; moved;) {
        moved = false;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                if (s[(size_t)y * w + x] || !g[(size_t)y * w + x]) continue;
                bool any = false;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if ((!dy && !dx) || (c == 4 && dy && dx)) continue;
                        const int yy = y + dy, xx = x + dx;
                        if (yy >= 0 && yy < h && xx >= 0 && xx < w && s[(size_t)yy * w + xx]) any = true;
                    }
                if (any) s[(size_t)y * w + x] = 1, moved = true;
            }
    }
    return s;
}

static Px rule(const Px *marker, const Px &m, int h, int w, int op, int c, long long *info)
{
    Px start(m.size()), g(m.size()), out(m.size());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const bool b = y == 0 || y == h - 1 || x == 0 || x == w - 1;
            g[i] = op == CANNY_HIP_RECON_FILL_HOLES ? !m[i] : m[i];
            start[i] = (op == CANNY_HIP_RECON_SEEDED ? (*marker)[i] : b) && g[i];
        }
    const Px r = propagate(start, g, h, w, op == CANNY_HIP_RECON_FILL_HOLES ? 12 - c : c);
    info[0] = info[1] = info[2] = 0;
    for (size_t i = 0; i < m.size(); i++) {
        out[i] = op == CANNY_HIP_RECON_SEEDED ? r[i] : (op == CANNY_HIP_RECON_FILL_HOLES ? !r[i] : m[i] && !r[i]);
        info[0] += out[i], info[1] += m[i], info[2] += start[i];
    }
    return out;
}

// rows MSB-first, pad bits set: they must be ignored
static std::vector<unsigned char> pack_dirty(const Px &px, int h, int w)
{
    const size_t rb = ((size_t)w + 7) / 8;
    std::vector<unsigned char> b(rb * h, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < (int)rb * 8; x++)
            if (x >= w || px[(size_t)y * w + x]) b[(size_t)y * rb + (x >> 3)] |= (unsigned char)(0x80u >> (x & 7));
    return b;
}

int main()
{
    const int kGuard = 32;
    std::mt19937 rng(38);
    const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {3, 5}, {7, 8}, {12, 13}, {17, 64}, {20, 65}, {33, 70}};
    for (const auto &sh : shapes)
        for (int n_frames = 1; n_frames <= 2; n_frames++)
            for (int op = 0; op <= 2; op++)
                for (int c = 4; c <= 8; c += 4) {
                    const int h = sh[0], w = sh[1];
                    const size_t rb = ((size_t)w + 7) / 8, fbytes = rb * h;
                    std::vector<unsigned char> kb, mb;
                    std::vector<Px> want;
                    std::vector<long long> want_info;
                    for (int f = 0; f < n_frames; f++) {
                        Px m((size_t)h * w), k((size_t)h * w);
                        for (auto &v : m) v = rng() % 100 < 55;
                        for (auto &v : k) v = rng() % 100 < 5;
                        long long inf[3];
                        want.push_back(rule(&k, m, h, w, op, c, inf));
                        want_info.insert(want_info.end(), inf, inf + 3);
                        const auto a = pack_dirty(k, h, w), b = pack_dirty(m, h, w);
                        kb.insert(kb.end(), a.begin(), a.end()), mb.insert(mb.end(), b.begin(), b.end());
                    }
                    std::vector<unsigned char> out(fbytes * n_frames + 2 * kGuard, 0x5A);
                    std::vector<long long> info(3 * n_frames + 2, 0x5A5A5A5A5A5A5A5All);
                    const int st = canny_hip_reconstruct_bits(op == CANNY_HIP_RECON_SEEDED ? kb.data() : nullptr, mb.data(), n_frames, h,
                                                              w, op, c, out.data() + kGuard, info.data() + 1);
                    CHECK(st == CANNY_HIP_OK);
                    for (int i = 0; i < kGuard; i++) CHECK(out[i] == 0x5A && out[out.size() - 1 - i] == 0x5A);
                    CHECK(info.front() == 0x5A5A5A5A5A5A5A5All && info.back() == 0x5A5A5A5A5A5A5A5All);
                    for (int f = 0; f < n_frames; f++) {
                        const unsigned char *o = out.data() + kGuard + (size_t)f * fbytes;
                        for (int y = 0; y < h; y++)
                            for (int x = 0; x < (int)rb * 8; x++) {
                                const int got = (o[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
                                CHECK(got == (x < w ? want[f][(size_t)y * w + x] : 0));
                            }
                        for (int j = 0; j < 3; j++) CHECK(info[1 + 3 * f + j] == want_info[3 * f + j]);
                    }
                }
    // the diamond ring closed only by diagonal steps: 13 pixels filled at c = 8, none at c = 4
    {
        Px d(9 * 9, 0);
        for (int i = 0; i < 4; i++) d[(4 - i) * 9 + 1 + i] = d[(4 + i) * 9 + 1 + i] = d[(4 - i) * 9 + 7 - i] = d[(4 + i) * 9 + 7 - i] = 1;
        const auto b = pack_dirty(d, 9, 9);
        std::vector<unsigned char> out(b.size());
        long long info[3];
        CHECK(canny_hip_reconstruct_bits(nullptr, b.data(), 1, 9, 9, CANNY_HIP_RECON_FILL_HOLES, 8, out.data(), info) == 0);
        CHECK(info[0] - info[1] == 13 && info[1] == 12);
        CHECK(canny_hip_reconstruct_bits(nullptr, b.data(), 1, 9, 9, CANNY_HIP_RECON_FILL_HOLES, 4, out.data(), info) == 0);
        CHECK(info[0] - info[1] == 0);
    }
    // refused calls write nothing
    {
        std::vector<unsigned char> m(16, 0xFF), out(16, 0x5A);
        long long info[4] = {7, 7, 7, 7};
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 4, 9, CANNY_HIP_RECON_SEEDED, 8, out.data(), info) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(m.data(), m.data(), 1, 4, 9, CANNY_HIP_RECON_FILL_HOLES, 8, out.data(), info) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 4, 9, CANNY_HIP_RECON_CLEAR_BORDER, 6, out.data(), info) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 4, 9, 3, 8, out.data(), info) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 4, 9, CANNY_HIP_RECON_CLEAR_BORDER, 8, m.data() + 4, info) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 4, 9, CANNY_HIP_RECON_CLEAR_BORDER, 8, out.data(),
                                         (long long *)((char *)info + 4)) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_reconstruct_bits(nullptr, m.data(), 1, 32769, 9, CANNY_HIP_RECON_CLEAR_BORDER, 8, out.data(), info) ==
              CANNY_HIP_ERR_UNSUPPORTED);
        for (auto v : out) CHECK(v == 0x5A);
        for (auto v : m) CHECK(v == 0xFF);
        for (auto v : info) CHECK(v == 7);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("reconstruct ok\n");
    return 0;
}
