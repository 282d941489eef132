// canny_line_fits_host.cpp -- canny_hip_line_fits_from_plane: the line-fit rule of include/canny_hip.h (DESIGN.md section
// 24) in plain C++ on one host frame: bit map, plane, line list and segment records.  No device, no HIP: what the CPU
// tests pin against tests/line_fits_rule.py, and what tests/cpp/test_line_fits_host.cpp compiles under the host compiler's
// sanitizers together with canny_edgels_host.cpp, whose canny_hip_edgels_from_plane supplies the edgel of every pixel.
// The support is found on the FULL plane (every set pixel's vote): there is no search window here.  The kernel of
// canny_line_fits.hip is written separately from this file on purpose; the GPU tests compare both with the Python rule.
// Built with -ffp-contract=off: the vote is three float roundings.
#include "canny_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

typedef __int128 i128;

int host_vote(int x, int y, float c, float s, int half)
{
    const float a = (float)x * c, b = (float)y * s;
    const float v = a + b;
    return (int)std::nearbyintf(v) + half;
}

// floor(sqrt(v)), exact, v < 2^63
uint64_t isqrt64(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// a / b to nearest, halves away from zero; b > 0, 2 |a| + b < 2^63
int64_t rdiv(int64_t a, int64_t b)
{
    const int64_t m = a < 0 ? -a : a, q = (2 * m + b) / (2 * b);
    return a < 0 ? -q : q;
}

int bitlength(i128 v) // v >= 0
{
    int n = 0;
    while (v) v >>= 1, n++;
    return n;
}

struct Moments {
    int64_t n = 0, su = 0, sv = 0, suu = 0, suv = 0, svv = 0;
};

struct Finish {
    int64_t mu, mv, dx, dy;
    bool degenerate;
};

Finish finish(const Moments &m, int ddx, int ddy)
{
    Finish f{0, 0, 0, 0, true};
    if (m.n) f.mu = rdiv(256 * m.su, m.n), f.mv = rdiv(256 * m.sv, m.n);
    i128 A = (i128)m.n * m.suu - (i128)m.su * m.su;
    i128 B = (i128)m.n * m.suv - (i128)m.su * m.sv;
    i128 C = (i128)m.n * m.svv - (i128)m.sv * m.sv;
    i128 top = B < 0 ? -B : B;
    if (A > top) top = A;
    if (C > top) top = C;
    const int s = bitlength(top) > 28 ? bitlength(top) - 28 : 0;
    const int64_t a = (int64_t)(A >> s), b = (int64_t)(B >> s), c = (int64_t)(C >> s); // arithmetic: floor
    const int64_t D = a - c, E = 2 * b;
    const int64_t h = (int64_t)isqrt64((uint64_t)(D * D) + (uint64_t)(E * E));
    if (m.n < 2 || h == 0) return f;
    int64_t wx, wy;
    if (D >= 0)
        wx = h + D, wy = E;
    else
        wx = E < 0 ? -E : E, wy = E < 0 ? -(h - D) : h - D;
    if (wx * ddx + wy * ddy < 0) wx = -wx, wy = -wy;
    // the larger component to exactly 31 bits (|w| < 2^30.3, so k >= 1): len >= 2^30 and the squares stay below 2^62
    const int64_t ax = wx < 0 ? -wx : wx, ay = wy < 0 ? -wy : wy;
    const int k = 31 - bitlength(ax > ay ? ax : ay);
    wx *= (int64_t)1 << k, wy *= (int64_t)1 << k;
    const int64_t len = (int64_t)isqrt64((uint64_t)(wx * wx) + (uint64_t)(wy * wy));
    f.dx = rdiv(wx * (1ll << 30), len);
    f.dy = rdiv(wy * (1ll << 30), len);
    f.degenerate = false;
    return f;
}

int64_t along(int64_t p, int64_t q) { return (p * q + (1ll << 29)) >> 30; }

} // namespace

extern "C" int canny_hip_line_fits_from_plane(const unsigned char *bits, const void *plane, int plane_is_u8, int height,
                                              int width, float rho, int numangle, int numrho, const float *tab_cos,
                                              const float *tab_sin, const unsigned int *bases, int n_lines,
                                              const int *segments, int n_segments, int options, int *fits)
{
    if (!bits || !plane || !tab_cos || !tab_sin || n_lines < 0 || (n_lines && !bases) || n_segments < 0 ||
        (n_segments && (!segments || !fits)) || numangle < 1 || numrho < 1 || (options & ~3) || height < 2 || width < 2 ||
        !(rho > 0.0f))
        return CANNY_HIP_ERR_INVALID;
    if (height > CANNY_HIP_LINE_FIT_MAX_AXIS || width > CANNY_HIP_LINE_FIT_MAX_AXIS || rho > CANNY_HIP_LINE_FIT_MAX_RHO)
        return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t row_bytes = ((size_t)width + 7) / 8;
    std::vector<unsigned> px; // the set pixels of E as indices, raster order
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7)) & 1) px.push_back((unsigned)(y * width + x));
    const unsigned stride = (unsigned)numrho + 2u;
    const int half = (numrho - 1) / 2;
    std::vector<unsigned> sup;
    std::vector<int> edgels;
    std::vector<int64_t> us, vs;
    for (int j = 0; j < n_segments; j++) {
        const int *rec = segments + (size_t)j * CANNY_HIP_SEGMENT_INTS;
        int *out = fits + (size_t)j * CANNY_HIP_LINE_FIT_INTS;
        std::memset(out, 0, CANNY_HIP_LINE_FIT_INTS * sizeof(int));
        out[9] = (int)CANNY_HIP_LINE_FIT_INVALID;
        const int x0 = rec[0], y0 = rec[1], x1 = rec[2], y1 = rec[3], k = rec[4];
        if (k < 0 || k >= n_lines) continue;
        const int n = (int)(bases[k] / stride) - 1, r = (int)(bases[k] % stride) - 1;
        if (n < 0 || n >= numangle || r < 0 || r >= numrho) continue;
        if (x0 < 0 || x0 >= width || x1 < 0 || x1 >= width || y0 < 0 || y0 >= height || y1 < 0 || y1 >= height) continue;
        const float c = tab_cos[n], s = tab_sin[n];
        const bool major_x = std::fabs(s) >= std::fabs(c);
        const int ta = major_x ? x0 : y0, tb = major_x ? x1 : y1;
        if (ta > tb) continue;
        // step 2: the support inside the segment's extent
        sup.clear();
        for (unsigned p : px) {
            const int y = (int)(p / (unsigned)width), x = (int)(p % (unsigned)width), t = major_x ? x : y;
            if (t >= ta && t <= tb && host_vote(x, y, c, s, half) == r) sup.push_back(p);
        }
        // step 3: their edgels, gated
        edgels.resize(sup.size() * CANNY_HIP_EDGEL_INTS + 1);
        const int rc = canny_hip_edgels_from_plane(plane, plane_is_u8, height, width, sup.data(), sup.size(), edgels.data());
        if (rc) return rc;
        const int ddx = x1 - x0, ddy = y1 - y0;
        us.clear(), vs.clear();
        Moments m;
        for (size_t i = 0; i < sup.size(); i++) {
            const int *e = edgels.data() + i * CANNY_HIP_EDGEL_INTS;
            const int gx = (int16_t)((uint32_t)e[2] & 0xffffu), gy = (int16_t)((uint32_t)e[2] >> 16);
            if (options & CANNY_HIP_LINE_FIT_GATE) {
                const int64_t dot = (int64_t)gx * ddx + (int64_t)gy * ddy;
                const int64_t g2 = (int64_t)gx * gx + (int64_t)gy * gy, d2 = (int64_t)ddx * ddx + (int64_t)ddy * ddy;
                if (!(gx | gy) || 4 * dot * dot > g2 * d2) continue;
            }
            if ((options & CANNY_HIP_LINE_FIT_REFINED_ONLY) && !((uint32_t)e[3] & CANNY_HIP_EDGEL_REFINED)) continue;
            const int64_t u = (int64_t)e[0] - 256 * x0, v = (int64_t)e[1] - 256 * y0;
            us.push_back(u), vs.push_back(v);
            m.n++, m.su += u, m.sv += v, m.suu += u * u, m.suv += u * v, m.svv += v * v;
        }
        const Finish f = finish(m, ddx, ddy);
        const int64_t cx = 65536ll * x0 + f.mu, cy = 65536ll * y0 + f.mv;
        out[4] = (int)cx, out[5] = (int)cy, out[8] = (int)m.n;
        if (f.degenerate) {
            out[0] = 65536 * x0, out[1] = 65536 * y0, out[2] = 65536 * x1, out[3] = 65536 * y1;
            out[9] = (int)CANNY_HIP_LINE_FIT_DEGENERATE;
            continue;
        }
        uint64_t sdd = 0;
        int64_t maxd = 0, pmin = 0, pmax = 0;
        for (size_t i = 0; i < us.size(); i++) {
            const int64_t U = 256 * us[i] - f.mu, V = 256 * vs[i] - f.mv;
            const int64_t d = (V * f.dx - U * f.dy + (1ll << 37)) >> 38;
            const int64_t p = (U * f.dx + V * f.dy + (1ll << 29)) >> 30;
            sdd += (uint64_t)(d * d);
            const int64_t ad = d < 0 ? -d : d;
            if (ad > maxd) maxd = ad;
            if (!i || p < pmin) pmin = p;
            if (!i || p > pmax) pmax = p;
        }
        out[0] = (int)(cx + along(pmin, f.dx)), out[1] = (int)(cy + along(pmin, f.dy));
        out[2] = (int)(cx + along(pmax, f.dx)), out[3] = (int)(cy + along(pmax, f.dy));
        out[6] = (int)f.dx, out[7] = (int)f.dy;
        out[9] = (int)((uint32_t)maxd & CANNY_HIP_LINE_FIT_MAXD_MASK);
        out[10] = (int)(uint32_t)sdd, out[11] = (int)(uint32_t)(sdd >> 32);
    }
    return CANNY_HIP_OK;
}

// Host-only test hook: steps 4 to 6 on moment sets, outputs as canny_hip_dev_line_fits_arith.
extern "C" int canny_hip_line_fits_finish(const long long *moments, size_t n_sets, int *out)
{
    if (!n_sets || !moments || !out) return CANNY_HIP_ERR_INVALID;
    for (size_t i = 0; i < n_sets; i++) {
        const long long *p = moments + 8 * i;
        Moments m;
        m.n = p[0], m.su = p[1], m.sv = p[2], m.suu = p[3], m.suv = p[4], m.svv = p[5];
        const Finish f = finish(m, (int)p[6], (int)p[7]);
        int *o = out + 6 * i;
        o[0] = (int)f.mu, o[1] = (int)f.mv, o[2] = (int)f.dx, o[3] = (int)f.dy, o[4] = (int)m.n;
        o[5] = f.degenerate ? (int)CANNY_HIP_LINE_FIT_DEGENERATE : 0;
    }
    return CANNY_HIP_OK;
}
