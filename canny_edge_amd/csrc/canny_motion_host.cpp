// canny_motion_host.cpp -- canny_hip_estimate_motion: the frame-to-frame motion rule of include/canny_hip.h (DESIGN.md
// section 31) in plain C++ on host buffers, one pair of frames.  No device, no HIP: what the CPU tests pin against
// tests/motion_rule.py, and what tests/cpp/test_motion_host.cpp compiles under the host compiler's sanitizers.  The kernels
// of canny_motion.hip are written separately from this file on purpose; the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

typedef __int128 i128;
typedef unsigned __int128 u128;
typedef long long i64;

struct Corr {
    int x, y, u, v; // query (x, y) -> train (u, v)
};

struct Hyp {
    i64 D, m11, m12, m21, m22;
    int i[3];
};

unsigned draw(unsigned &s, unsigned n)
{
    s = s * 1664525u + 1013904223u;
    return (s >> 16) % n;
}

// false: D == 0
bool build(const std::vector<Corr> &c, int model, unsigned seed, int h, Hyp &o)
{
    const unsigned m = (unsigned)c.size();
    unsigned s = seed + 0x9E3779B9u * (unsigned)(h + 1);
    o.i[0] = (int)draw(s, m), o.i[1] = o.i[2] = -1;
    if (model == CANNY_HIP_MOTION_TRANSLATION) {
        o.D = 1, o.m11 = o.m22 = 1, o.m12 = o.m21 = 0;
        return true;
    }
    int i2 = (int)draw(s, m - 1);
    i2 += i2 >= o.i[0];
    o.i[1] = i2;
    const Corr &a = c[o.i[0]], &b = c[i2];
    const i64 dx = b.x - a.x, dy = b.y - a.y, du = b.u - a.u, dv = b.v - a.v;
    if (model == CANNY_HIP_MOTION_SIMILARITY) {
        const i64 A = dx * du + dy * dv, B = dx * dv - dy * du;
        o.D = dx * dx + dy * dy;
        o.m11 = A, o.m12 = -B, o.m21 = B, o.m22 = A;
        return o.D != 0;
    }
    int i3 = (int)draw(s, m - 2);
    const int lo = o.i[0] < i2 ? o.i[0] : i2, hi = o.i[0] < i2 ? i2 : o.i[0];
    i3 += i3 >= lo;
    i3 += i3 >= hi;
    o.i[2] = i3;
    const Corr &f = c[i3];
    const i64 fx = f.x - a.x, fy = f.y - a.y, fu = f.u - a.u, fv = f.v - a.v;
    o.D = dx * fy - dy * fx;
    o.m11 = du * fy - fu * dy, o.m12 = fu * dx - du * fx;
    o.m21 = dv * fy - fv * dy, o.m22 = fv * dx - dv * fx;
    return o.D != 0;
}

// 256 (rx^2 + ry^2) <= thr^2 D^2, exactly: |r| < 2^53, so the left side stays under 2^116 and the right under 2^90
bool inlier(const Corr &c, const Corr &q1, const Hyp &h, u128 rhs)
{
    const i64 dx = c.x - q1.x, dy = c.y - q1.y, du = c.u - q1.u, dv = c.v - q1.v;
    const i64 rx = h.D * du - (h.m11 * dx + h.m12 * dy), ry = h.D * dv - (h.m21 * dx + h.m22 * dy);
    const u128 ax = (u128)(uint64_t)(rx < 0 ? -rx : rx), ay = (u128)(uint64_t)(ry < 0 ? -ry : ry);
    return ((ax * ax + ay * ay) << 8) <= rhs;
}

i128 floor_div(i128 n, i128 d) // d > 0
{
    i128 q = n / d;
    if (n % d != 0 && n < 0) q--;
    return q;
}

i64 floor_div64(i64 n, i64 d) // d > 0
{
    i64 q = n / d;
    if (n % d != 0 && n < 0) q--;
    return q;
}

const i64 kLimit = 1ll << 24;

} // namespace

extern "C" int canny_hip_estimate_motion(const long long *q_corners, int n_q, const long long *t_corners, int n_t,
                                         const int *matches, int model, int thr_q4, int hypotheses, unsigned seed,
                                         long long *motion, int *inlier_flags)
{
    if (n_q < 0 || n_t < 0 || !motion || (n_q > 0 && (!q_corners || !matches)) || (n_t > 0 && !t_corners) ||
        model < CANNY_HIP_MOTION_TRANSLATION || model > CANNY_HIP_MOTION_AFFINE || thr_q4 < 0 || thr_q4 > 4095 ||
        hypotheses < 1 || ((uintptr_t)q_corners & 7) || ((uintptr_t)t_corners & 7) || ((uintptr_t)motion & 7))
        return CANNY_HIP_ERR_INVALID;
    if (n_q > CANNY_HIP_HOUGH_MAX_LINES || n_t > CANNY_HIP_HOUGH_MAX_LINES || hypotheses > CANNY_HIP_MOTION_MAX_HYPOTHESES)
        return CANNY_HIP_ERR_UNSUPPORTED;

    std::vector<Corr> c;
    std::vector<int> slot;
    for (int i = 0; i < n_q; i++) {
        const int j = matches[4 * i], flags = matches[4 * i + 3];
        bool is = (flags & 8) && j >= 0 && j < n_t;
        if (is) {
            const i64 x = q_corners[4 * (size_t)i], y = q_corners[4 * (size_t)i + 1];
            const i64 u = t_corners[4 * (size_t)j], v = t_corners[4 * (size_t)j + 1];
            is = x >= 0 && x <= 65535 && y >= 0 && y <= 65535 && u >= 0 && u <= 65535 && v >= 0 && v <= 65535;
            if (is) {
                c.push_back(Corr{(int)x, (int)y, (int)u, (int)v});
                slot.push_back(i);
            }
        }
        if (inlier_flags) inlier_flags[i] = is ? 0 : -1;
    }
    const int m = (int)c.size(), k = model + 1;
    long long rec[CANNY_HIP_MOTION_WORDS];
    std::memset(rec, 0, sizeof rec);
    rec[1] = m, rec[3] = -1, rec[12] = rec[13] = rec[14] = -1;

    Hyp best{};
    int best_h = -1, best_n = -1;
    if (m >= k) {
        for (int h = 0; h < hypotheses; h++) {
            Hyp hy;
            if (!build(c, model, seed, h, hy)) continue;
            const u128 rhs = (u128)((uint64_t)thr_q4 * (uint64_t)thr_q4) * ((u128)(uint64_t)(hy.D < 0 ? -hy.D : hy.D) *
                                                                          (uint64_t)(hy.D < 0 ? -hy.D : hy.D));
            const Corr &q1 = c[hy.i[0]];
            int n = 0;
            for (int e = 0; e < m; e++) n += inlier(c[e], q1, hy, rhs);
            if (n > best_n) best_n = n, best_h = h, best = hy;
        }
    }
    if (best_h < 0) {
        std::memcpy(motion, rec, sizeof rec);
        return CANNY_HIP_OK;
    }

    // the inliers of the best hypothesis and the eleven sums over them
    const uint64_t aD = (uint64_t)(best.D < 0 ? -best.D : best.D);
    const u128 rhs = (u128)((uint64_t)thr_q4 * (uint64_t)thr_q4) * ((u128)aD * aD);
    std::vector<char> in((size_t)m);
    i64 n = 0, sx = 0, sy = 0, su = 0, sv = 0, sxx = 0, sxy = 0, syy = 0, sxu = 0, sxv = 0, syu = 0, syv = 0;
    for (int e = 0; e < m; e++) {
        in[e] = inlier(c[e], c[best.i[0]], best, rhs);
        if (inlier_flags) inlier_flags[slot[e]] = in[e];
        if (!in[e]) continue;
        const i64 x = c[e].x, y = c[e].y, u = c[e].u, v = c[e].v;
        n++, sx += x, sy += y, su += u, sv += v;
        sxx += x * x, sxy += x * y, syy += y * y, sxu += x * u, sxv += x * v, syu += y * u, syv += y * v;
    }
    rec[0] = 1, rec[2] = n, rec[3] = best_h, rec[15] = best.D;
    for (int s = 0; s < k; s++) rec[12 + s] = slot[best.i[s]];

    const i64 cxx = n * sxx - sx * sx, cxy = n * sxy - sx * sy, cyy = n * syy - sy * sy;
    const i64 cxu = n * sxu - sx * su, cxv = n * sxv - sx * sv, cyu = n * syu - sy * su, cyv = n * syv - sy * sv;
    i128 a11 = 65536, a12 = 0, a21 = 0, a22 = 65536;
    bool ok = true;
    if (model == CANNY_HIP_MOTION_SIMILARITY) {
        const i128 dn = (i128)cxx + cyy;
        ok = dn > 0;
        if (ok) {
            a11 = a22 = floor_div(((i128)cxu + cyv) * 65536, dn);
            a21 = floor_div(((i128)cxv - cyu) * 65536, dn);
            a12 = -a21;
        }
    } else if (model == CANNY_HIP_MOTION_AFFINE) {
        const i128 det = (i128)cxx * cyy - (i128)cxy * cxy;
        ok = det > 0;
        if (ok) {
            a11 = floor_div(((i128)cxu * cyy - (i128)cyu * cxy) * 65536, det);
            a12 = floor_div(((i128)cyu * cxx - (i128)cxu * cxy) * 65536, det);
            a21 = floor_div(((i128)cxv * cyy - (i128)cyv * cxy) * 65536, det);
            a22 = floor_div(((i128)cyv * cxx - (i128)cxv * cxy) * 65536, det);
        }
    }
    if (ok)
        for (i128 a : {a11, a12, a21, a22})
            if (a > kLimit || a < -kLimit) ok = false;
    if (ok) {
        const i64 b11 = (i64)a11, b12 = (i64)a12, b21 = (i64)a21, b22 = (i64)a22;
        const i64 tx = floor_div64(65536 * su - b11 * sx - b12 * sy, n), ty = floor_div64(65536 * sv - b21 * sx - b22 * sy, n);
        i64 total = 0, worst = 0;
        for (int e = 0; e < m; e++) {
            if (!in[e]) continue;
            i64 gx = (65536ll * c[e].u - (b11 * c[e].x + b12 * c[e].y + tx)) >> 8;
            i64 gy = (65536ll * c[e].v - (b21 * c[e].x + b22 * c[e].y + ty)) >> 8;
            gx = gx < -kLimit ? -kLimit : gx > kLimit ? kLimit : gx;
            gy = gy < -kLimit ? -kLimit : gy > kLimit ? kLimit : gy;
            const i64 g = gx * gx + gy * gy;
            total += g;
            if (g > worst) worst = g;
        }
        rec[0] |= 2;
        rec[4] = b11, rec[5] = b12, rec[6] = tx, rec[7] = b21, rec[8] = b22, rec[9] = ty, rec[10] = total, rec[11] = worst;
    }
    std::memcpy(motion, rec, sizeof rec);
    return CANNY_HIP_OK;
}
