// Stand-alone check of csrc/canny_motion_host.cpp (own main; built by tests/test_motion_rule.py with the host compiler's
// address and undefined-behaviour sanitizers, together with that one file): exact integer motions with wrong matches, sets
// too small for a model, coincident and collinear points, 4096 correspondences with coordinates spread to 0 and 65535 (the
// width bounds), skipped slots and refused calls -- all with buffers of exactly the needed size.
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

struct Set {
    std::vector<long long> q, t;
    std::vector<int> m;
    int n = 0;
    void add(long long x, long long y, long long u, long long v, int flags = 15)
    {
        q.insert(q.end(), {x, y, 0, n});
        t.insert(t.end(), {u, v, 0, n});
        m.insert(m.end(), {n, 0, 0, flags});
        n++;
    }
};

static int run(const Set &s, int model, int thr, int hyp, unsigned seed, long long *rec, std::vector<int> &flags)
{
    flags.assign((size_t)s.n, -7);
    return canny_hip_estimate_motion(s.n ? s.q.data() : nullptr, s.n, s.n ? s.t.data() : nullptr, s.n,
                                     s.n ? s.m.data() : nullptr, model, thr, hyp, seed, rec, s.n ? flags.data() : nullptr);
}

int main()
{
    std::vector<long long> rec(CANNY_HIP_MOTION_WORDS);
    std::vector<int> flags;
    uint32_t seed = 777;

    // exact integer motions, a third of the matches wrong: the refit is the motion, the residuals are zero
    const long long motions[][7] = {{0, 1, 0, 0, 1, 5, -3 + 40}, {1, 0, -1, 1, 0, 700, 20}, {1, 2, 0, 0, 2, 3, 4}, {2, 1, 1, 0, 1, 7, 9}};
    for (const auto &mo : motions) {
        Set s;
        for (int i = 0; i < 90; i++) {
            const long long x = lcg(seed) % 600, y = lcg(seed) % 600;
            if (i % 3 == 2)
                s.add(x, y, lcg(seed) % 1800, lcg(seed) % 1800);
            else
                s.add(x, y, mo[1] * x + mo[2] * y + mo[5], mo[3] * x + mo[4] * y + mo[6]);
        }
        CHECK(run(s, (int)mo[0], 16, 64, 5, rec.data(), flags) == CANNY_HIP_OK);
        CHECK(rec[0] == 3 && rec[1] == 90 && rec[2] >= 60);
        CHECK(rec[4] == 65536 * mo[1] && rec[5] == 65536 * mo[2] && rec[7] == 65536 * mo[3] && rec[8] == 65536 * mo[4]);
        CHECK(rec[6] == 65536 * mo[5] && rec[9] == 65536 * mo[6] && rec[10] == 0 && rec[11] == 0);
        int n_in = 0;
        for (int i = 0; i < 90; i++) {
            CHECK(flags[i] == 0 || flags[i] == 1);
            CHECK(i % 3 == 2 || flags[i] == 1);
            n_in += flags[i];
        }
        CHECK(n_in == rec[2]);
    }

    // m = 0..3 against each model's sample size; all query points equal; collinear points under AFFINE
    for (int m = 0; m <= 3; m++)
        for (int model = 0; model < 3; model++) {
            Set s;
            for (int i = 0; i < m; i++) s.add(10 + 7 * i, 20 + 3 * i * i, 15 + 7 * i, 18 + 3 * i * i);
            CHECK(run(s, model, 16, 8, 1, rec.data(), flags) == CANNY_HIP_OK);
            CHECK(rec[1] == m && (rec[0] & 1) == (m > model) && rec[3] == (m > model ? 0 : -1));
            if (m <= model) {
                for (int w = 4; w < 12; w++) CHECK(rec[w] == 0);
                CHECK(rec[2] == 0 && rec[12] == -1 && rec[13] == -1 && rec[14] == -1 && rec[15] == 0);
                for (int i = 0; i < m; i++) CHECK(flags[i] == 0);
            }
        }
    {
        Set s;
        for (int i = 0; i < 12; i++) s.add(33, 44, 10 * i, 3 * i);
        for (int model = 1; model < 3; model++) {
            CHECK(run(s, model, 4095, 32, 2, rec.data(), flags) == CANNY_HIP_OK);
            CHECK(rec[0] == 0 && rec[1] == 12 && rec[3] == -1);
        }
        CHECK(run(s, 0, 0, 32, 2, rec.data(), flags) == CANNY_HIP_OK);
        CHECK(rec[0] == 3 && rec[2] == 1);
        Set line;
        for (int i = 0; i < 12; i++) line.add(5 * i, 10 * i, 5 * i + 1, 10 * i);
        line.add(3, 100, 900, 900);
        CHECK(run(line, 2, 16, 64, 3, rec.data(), flags) == CANNY_HIP_OK);
        CHECK(rec[1] == 13 && (rec[0] == 1 || rec[0] == 3));
    }

    // the width bounds: 4096 correspondences, coordinates spread to 0 and 65535, the widest threshold
    {
        Set s;
        const long long e = 65535;
        const long long ext[][4] = {{0, 0, e, e}, {e, e, 0, 0}, {0, e, e, 0}, {e, 0, 0, e}, {0, 0, 0, e}, {e, e, e, 0}, {0, e, 0, 0}, {e, 0, e, e}};
        for (const auto &c : ext) s.add(c[0], c[1], c[2], c[3]);
        for (int model = 0; model < 3; model++) {
            CHECK(run(s, model, 4095, 256, 9, rec.data(), flags) == CANNY_HIP_OK);
            CHECK(rec[1] == 8 && (rec[0] & 1));
        }
        while (s.n < 4096) {
            const long long x = lcg(seed) >> 16, y = lcg(seed) >> 16;
            if (s.n % 2)
                s.add(x, y, e - x, e - y);
            else
                s.add(x, y, lcg(seed) >> 16, lcg(seed) >> 16);
        }
        for (int model = 0; model < 3; model++) {
            CHECK(run(s, model, 4095, 64, 9, rec.data(), flags) == CANNY_HIP_OK);
            CHECK(rec[1] == 4096 && (rec[0] & 1) && rec[2] >= 1);
        }
    }

    // skipped slots: not accepted, a train index outside the count, coordinates outside [0, 65535]
    {
        Set s;
        for (int i = 0; i < 20; i++) s.add(10 * i, i * i, 10 * i + 2, i * i + 1);
        s.m[4 * 3 + 3] = 7, s.m[4 * 5] = 20, s.m[4 * 6] = -1, s.q[4 * 8] = -1, s.t[4 * 9 + 1] = 65536, s.q[4 * 11 + 1] = 1ll << 40;
        CHECK(run(s, 0, 16, 8, 4, rec.data(), flags) == CANNY_HIP_OK);
        CHECK(rec[0] == 3 && rec[1] == 14 && rec[2] == 14 && rec[6] == 2 * 65536 && rec[9] == 65536);
        for (int i = 0; i < 20; i++) {
            const bool skipped = i == 3 || i == 5 || i == 6 || i == 8 || i == 9 || i == 11;
            CHECK(flags[i] == (skipped ? -1 : 1));
        }
        // no inlier buffer
        CHECK(canny_hip_estimate_motion(s.q.data(), s.n, s.t.data(), s.n, s.m.data(), 1, 16, 8, 4, rec.data(), nullptr) == CANNY_HIP_OK);
        CHECK(rec[0] == 3 && rec[1] == 14);
    }

    // refused calls write nothing
    {
        Set s;
        for (int i = 0; i < 5; i++) s.add(i, 2 * i, i + 1, 2 * i);
        std::vector<long long> r(CANNY_HIP_MOTION_WORDS, 0x5a5a5a5a5a5a5a5all);
        std::vector<int> f(5, -7);
        const long long *q = s.q.data(), *t = s.t.data();
        const int *m = s.m.data();
        CHECK(canny_hip_estimate_motion(nullptr, 5, t, 5, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, nullptr, 5, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, nullptr, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 0, 16, 8, 1, nullptr, f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, -1, t, 5, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, -1, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 3, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, -1, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 0, 4096, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 0, -1, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 0, 16, 0, 1, r.data(), f.data()) == CANNY_HIP_ERR_INVALID);
        CHECK(canny_hip_estimate_motion(q, 5, t, 5, m, 0, 16, 4097, 1, r.data(), f.data()) == CANNY_HIP_ERR_UNSUPPORTED);
        CHECK(canny_hip_estimate_motion(q, 4097, t, 5, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_UNSUPPORTED);
        CHECK(canny_hip_estimate_motion(q, 5, t, 4097, m, 0, 16, 8, 1, r.data(), f.data()) == CANNY_HIP_ERR_UNSUPPORTED);
        for (long long v : r) CHECK(v == 0x5a5a5a5a5a5a5a5all);
        for (int v : f) CHECK(v == -7);
    }
    std::printf("motion ok\n");
    return 0;
}
