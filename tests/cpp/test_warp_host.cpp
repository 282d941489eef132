// Stand-alone check of csrc/canny_warp_host.cpp (own main; built by tests/test_warp_rule.py with the host compiler's address
// and undefined-behaviour sanitizers, together with that one file): the identity, an integer shift, the quarter turn and a
// mirror against their known answers, negative positions, footprints outside the source, the magnitude limits with the widest
// sums (no signed overflow), chains that break, source indices out of range and refused calls -- all with buffers of exactly
// the needed size.
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
typedef std::vector<long long> Words;

static const long long ONE = 65536, LIM_A = 1ll << 24, LIM_T = 1ll << 36;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static Bytes noise(int n, uint32_t seed)
{
    Bytes b((size_t)n);
    for (auto &v : b) v = (unsigned char)(lcg(seed) >> 24);
    return b;
}

static Words record(long long a11, long long a12, long long tx, long long a21, long long a22, long long ty, long long src = 0,
                    long long flags = 1)
{
    return Words{flags, src, a11, a12, tx, a21, a22, ty};
}

static Words motion(long long a11, long long a12, long long tx, long long a21, long long a22, long long ty, long long flags = 3)
{
    Words m(CANNY_HIP_MOTION_WORDS, 0);
    m[0] = flags, m[4] = a11, m[5] = a12, m[6] = tx, m[7] = a21, m[8] = a22, m[9] = ty;
    return m;
}

struct Result {
    int status;
    Bytes out, valid;
    bool bit(int w, int x, int y, int frame = 0, int h = 0) const
    {
        const size_t rb = ((size_t)w + 7) / 8;
        return (valid[((size_t)frame * h + y) * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
    }
};

static Result warp(const Bytes &src, int n_src, int sh, int sw, const Words &x, int oh, int ow, int interp, int border)
{
    const int n_out = (int)(x.size() / CANNY_HIP_XFORM_WORDS);
    Result r;
    r.out.assign((size_t)n_out * oh * ow, 0xEE);
    r.valid.assign((size_t)n_out * oh * ((ow + 7) / 8), 0xEE);
    r.status = canny_hip_warp_frames(src.data(), n_src, sh, sw, x.data(), n_out, oh, ow, interp, border, r.out.data(),
                                     r.valid.data());
    return r;
}

int main()
{
    const int H = 19, W = 37;
    const Bytes P = noise(H * W, 1);
    for (int interp = 0; interp < 2; interp++) {
        // the identity
        Result r = warp(P, 1, H, W, record(ONE, 0, 0, 0, ONE, 0), H, W, interp, 9);
        CHECK(r.status == 0 && r.out == P);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W + 3; x++) CHECK(r.bit(W, x, y, 0, H) == (x < W)); // pad bits are 0
        // an integer shift: output (x, y) reads (x + 5, y - 3)
        r = warp(P, 1, H, W, record(ONE, 0, 5 * ONE, 0, ONE, -3 * ONE), H, W, interp, 200);
        CHECK(r.status == 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const bool in = x + 5 < W && y - 3 >= 0;
                CHECK(r.out[(size_t)y * W + x] == (in ? P[(size_t)(y - 3) * W + x + 5] : 200) && r.bit(W, x, y, 0, H) == in);
            }
        // the quarter turn: R holds P's (x, y) at (y, W - 1 - x); R is W rows of H
        Bytes R((size_t)H * W);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) R[(size_t)(W - 1 - x) * H + y] = P[(size_t)y * W + x];
        r = warp(R, 1, W, H, record(0, ONE, 0, -ONE, 0, (W - 1) * ONE), H, W, interp, 0);
        CHECK(r.status == 0 && r.out == P);
        // a mirror
        r = warp(P, 1, H, W, record(-ONE, 0, (W - 1) * ONE, 0, ONE, 0), H, W, interp, 0);
        CHECK(r.status == 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) CHECK(r.out[(size_t)y * W + x] == P[(size_t)y * W + W - 1 - x]);
        // negative positions: -1 stays on the grid under both rules
        r = warp(P, 1, H, W, record(ONE, 0, -1, 0, ONE, -1), H, W, interp, 77);
        CHECK(r.status == 0 && r.out == P && r.bit(W, 0, 0, 0, H));
        r = warp(P, 1, H, W, record(ONE, 0, -129, 0, ONE, -129), H, W, interp, 77);
        CHECK(r.status == 0 && r.bit(W, 0, 0, 0, H) == (interp == 0) && r.bit(W, 1, 1, 0, H));
        // wholly outside, on every side and far away
        const long long far[][2] = {{-100, 0}, {100, 0}, {0, -100}, {0, 100}, {LIM_T / ONE, -LIM_T / ONE}};
        for (auto &f : far) {
            r = warp(P, 1, H, W, record(ONE, 0, f[0] * ONE, 0, ONE, f[1] * ONE), H, W, interp, 13);
            CHECK(r.status == 0);
            for (auto v : r.out) CHECK(v == 13);
            for (auto v : r.valid) CHECK(v == 0);
        }
        // the limits: the widest sums, at the largest output dimension (one row of 32768, one column of 32768)
        r = warp(P, 1, H, W, record(-LIM_A, LIM_A, LIM_T, LIM_A, -LIM_A, -LIM_T), 1, 32768, interp, 3);
        CHECK(r.status == 0);
        r = warp(P, 1, H, W, record(LIM_A, LIM_A, -LIM_T, -LIM_A, -LIM_A, LIM_T), 32768, 1, interp, 3);
        CHECK(r.status == 0);
        r = warp(P, 1, H, W, record(LIM_A, 0, 0, 0, LIM_A, 0), 2, 2, interp, 3);
        CHECK(r.status == 0 && r.out[0] == P[0] && r.out[1] == 3 && r.bit(2, 0, 0, 0, 2) && !r.bit(2, 1, 0, 0, 2));
        // one past a limit, a source index out of range, a cleared flag: the border and no valid bit
        Words bad;
        for (const Words &w : {record(LIM_A + 1, 0, 0, 0, ONE, 0), record(ONE, 0, 0, 0, -LIM_A - 1, 0),
                               record(ONE, 0, LIM_T + 1, 0, ONE, 0), record(ONE, 0, 0, 0, ONE, -LIM_T - 1),
                               record(ONE, 0, 0, 0, ONE, 0, 1), record(ONE, 0, 0, 0, ONE, 0, -1),
                               record(ONE, 0, 0, 0, ONE, 0, 0, 2), record(ONE, 0, 0, 0, ONE, 0, 1ll << 40)})
            bad.insert(bad.end(), w.begin(), w.end());
        r = warp(P, 1, H, W, bad, 5, 9, interp, 44);
        CHECK(r.status == 0);
        for (auto v : r.out) CHECK(v == 44);
        for (auto v : r.valid) CHECK(v == 0);
        // a random affine map: every read stays inside the source buffer (the sanitizer is the judge)
        uint32_t s = 5 + interp;
        for (int k = 0; k < 20; k++) {
            Words w = record((long long)(lcg(s) >> 14) - 131072, (long long)(lcg(s) >> 14) - 131072,
                             ((long long)(lcg(s) >> 8) - (1 << 23)), (long long)(lcg(s) >> 14) - 131072,
                             (long long)(lcg(s) >> 14) - 131072, ((long long)(lcg(s) >> 8) - (1 << 23)));
            r = warp(P, 1, H, W, w, 23, 41, interp, 1);
            CHECK(r.status == 0);
        }
    }

    // chains
    {
        Words m, x;
        for (int k = 0; k < 4; k++) {
            const Words q = motion(0, ONE, 0, -ONE, 0, 49 * ONE);
            m.insert(m.end(), q.begin(), q.end());
        }
        x.assign(5 * CANNY_HIP_XFORM_WORDS, -7);
        CHECK(canny_hip_compose_motion(m.data(), 4, 3, x.data()) == 0);
        CHECK(x[0] == 1 && x[1] == 3 && x[2] == ONE && x[3] == 0 && x[4] == 0 && x[5] == 0 && x[6] == ONE && x[7] == 0);
        CHECK(x[32] == 1 && x[33] == 7 && x[34] == ONE && x[35] == 0 && x[36] == 0 && x[37] == 0 && x[38] == ONE && x[39] == 0);
        CHECK(x[16 + 2] == -ONE && x[16 + 4] == 49 * ONE && x[16 + 6] == -ONE && x[16 + 7] == 49 * ONE);
        // broken in the middle by a record without the refit bit, and by the limit
        for (int how = 0; how < 2; how++) {
            Words c = m;
            if (how == 0) c[2 * CANNY_HIP_MOTION_WORDS] = 1;
            else c[2 * CANNY_HIP_MOTION_WORDS + 4] = LIM_A + 1;
            x.assign(5 * CANNY_HIP_XFORM_WORDS, -7);
            CHECK(canny_hip_compose_motion(c.data(), 4, 0, x.data()) == 0);
            for (int k = 0; k < 5; k++) {
                CHECK(x[8 * k] == (k < 3) && x[8 * k + 1] == k);
                if (k >= 3)
                    for (int i = 2; i < 8; i++) CHECK(x[8 * k + i] == 0);
            }
        }
        // the widest sums: every coefficient at its limit, three times over
        Words e;
        for (int k = 0; k < 3; k++) {
            const Words q = motion(-LIM_A, LIM_A, LIM_T, LIM_A, -LIM_A, -LIM_T);
            e.insert(e.end(), q.begin(), q.end());
        }
        x.assign(4 * CANNY_HIP_XFORM_WORDS, -7);
        CHECK(canny_hip_compose_motion(e.data(), 3, 0, x.data()) == 0 && x[8] == 1 && x[16] == 0 && x[24] == 0);
        x.assign(CANNY_HIP_XFORM_WORDS, -7);
        CHECK(canny_hip_compose_motion(nullptr, 0, 9, x.data()) == 0 && x[0] == 1 && x[1] == 9 && x[2] == ONE);
    }

    // refused calls write nothing
    {
        Bytes out(6 * 9, 0xEE), valid(6 * 2, 0xEE);
        const Words x = record(ONE, 0, 0, 0, ONE, 0);
        Words chain(2 * CANNY_HIP_XFORM_WORDS, -7);
        const Words m = motion(ONE, 0, 0, 0, ONE, 0);
        CHECK(canny_hip_warp_frames(nullptr, 1, H, W, x.data(), 1, 6, 9, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, nullptr, 1, 6, 9, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 9, 0, 0, nullptr, valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 0, H, W, x.data(), 1, 6, 9, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 0, 6, 9, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, 0, W, x.data(), 1, 6, 9, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 0, 0, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 9, 2, 0, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 9, 0, 256, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 9, 0, -1, out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, (const long long *)((const char *)x.data() + 4), 1, 6, 9, 0, 0,
                                    out.data(), valid.data()) == 1);
        CHECK(canny_hip_warp_frames(out.data(), 1, 3, 9, x.data(), 1, 3, 9, 0, 0, out.data() + 26, valid.data()) == 1);
        CHECK(canny_hip_warp_frames(P.data(), 1, 32769, W, x.data(), 1, 6, 9, 0, 0, out.data(), valid.data()) == 2);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 32769, 0, 0, out.data(), valid.data()) == 2);
        CHECK(canny_hip_warp_frames(P.data(), 65536, H, W, x.data(), 1, 6, 9, 0, 0, out.data(), valid.data()) == 2);
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 65536, 6, 9, 0, 0, out.data(), valid.data()) == 2);
        CHECK(canny_hip_compose_motion(nullptr, 1, 0, chain.data()) == 1);
        CHECK(canny_hip_compose_motion(m.data(), 1, 0, nullptr) == 1);
        CHECK(canny_hip_compose_motion(m.data(), -1, 0, chain.data()) == 1);
        CHECK(canny_hip_compose_motion(m.data(), 1, -1, chain.data()) == 1);
        CHECK(canny_hip_compose_motion(m.data(), 65536, 0, chain.data()) == 2);
        for (auto v : out) CHECK(v == 0xEE);
        for (auto v : valid) CHECK(v == 0xEE);
        for (auto v : chain) CHECK(v == -7);
        // without the valid buffer
        CHECK(canny_hip_warp_frames(P.data(), 1, H, W, x.data(), 1, 6, 9, 1, 0, out.data(), nullptr) == 0);
        CHECK(out[0] == P[0] && out[53] == P[5 * W + 8]);
    }
    std::printf("warp ok\n");
    return 0;
}
