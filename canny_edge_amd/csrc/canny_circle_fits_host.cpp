// canny_circle_fits_host.cpp -- canny_hip_circle_fits_from_plane: the circle-fit rule of include/canny_hip.h (DESIGN.md
// section 25) in plain C++ on one host frame: bit map, plane and circle records.  No device, no HIP: what the CPU tests
// pin against tests/circle_fits_rule.py, and what tests/cpp/test_circle_fits_host.cpp compiles under the host compiler's
// sanitizers together with canny_edgels_host.cpp, whose canny_hip_edgels_from_plane supplies the edgel of every pixel.
// The pixels of a record are found by testing every set pixel of the map against the band: there is no row walk here.
// The kernel of canny_circle_fits.hip is written separately from this file on purpose; the GPU tests compare both with
// the Python rule.
#include "canny_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

typedef __int128 i128;

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
    int64_t n = 0, su = 0, sv = 0, sz = 0, suu = 0, suv = 0, svv = 0;
    i128 suz = 0, svz = 0;
    void add(int64_t u, int64_t v, int64_t z)
    {
        n++, su += u, sv += v, sz += z, suu += u * u, suv += u * v, svv += v * v;
        suz += (i128)u * z, svz += (i128)v * z;
    }
};

struct Move {
    int64_t mx, my; // the centre's move, 1/65536 px
    bool degenerate;
};

// |num| * 2^e / det to nearest, halves away from zero, for a quotient of at most `limit` < 2^20: twenty steps of restoring
// division, no 128-bit quotient needed.  false: the quotient exceeds the limit.
bool quotient(i128 num, int e, int64_t det, int64_t limit, int64_t *out)
{
    const i128 m = num < 0 ? -num : num;
    const i128 X = e > 0 ? m << e : m, Y = e < 0 ? (i128)det << -e : (i128)det;
    if (2 * X >= Y * (2 * limit + 1)) return false;
    i128 R = 2 * X + Y;
    const i128 D = 2 * Y;
    int64_t q = 0;
    for (int i = 19; i >= 0; i--)
        if (R >= (D << i)) R -= D << i, q |= (int64_t)1 << i;
    *out = num < 0 ? -q : q;
    return true;
}

// steps 4 (from the sums on) and 5 of the rule
Move finish(const Moments &m, int band)
{
    Move f{0, 0, true};
    if (m.n < 3) return f;
    const i128 A = (i128)m.n * m.suu - (i128)m.su * m.su;
    const i128 B = (i128)m.n * m.suv - (i128)m.su * m.sv;
    const i128 C = (i128)m.n * m.svv - (i128)m.sv * m.sv;
    const i128 P = (i128)m.n * m.suz - (i128)m.su * m.sz;
    const i128 Q = (i128)m.n * m.svz - (i128)m.sv * m.sz;
    i128 top = B < 0 ? -B : B;
    if (A > top) top = A;
    if (C > top) top = C;
    const int s = bitlength(top) > 31 ? bitlength(top) - 31 : 0;
    const int64_t a = (int64_t)(A >> s), b = (int64_t)(B >> s), c = (int64_t)(C >> s); // arithmetic: floor
    const int64_t det = a * c - b * b;
    if (det <= 0) return f;
    const int64_t limit = 65536ll * (band + 2);
    int64_t mx, my;
    if (!quotient(P * c - Q * b, 7 - s, det, limit, &mx) || !quotient(Q * a - P * b, 7 - s, det, limit, &my)) return f;
    return Move{mx, my, false};
}

// 0..15: quadrants counter-clockwise from +x towards +y, four sectors each; a boundary belongs to the sector it starts
int sector_of(int64_t dx, int64_t dy)
{
    int quad;
    int64_t p, q;
    if (dx > 0 && dy >= 0)
        quad = 0, p = dx, q = dy;
    else if (dx <= 0 && dy > 0)
        quad = 1, p = dy, q = -dx;
    else if (dx < 0 && dy <= 0)
        quad = 2, p = -dx, q = -dy;
    else if (dx >= 0 && dy < 0)
        quad = 3, p = -dy, q = dx;
    else
        return 0;
    return 4 * quad + (2 * q >= p) + (q >= p) + (q >= 2 * p);
}

struct Pt {
    int64_t u, v;
};

struct Fit {
    int64_t mx, my, r;
    std::vector<int64_t> d;
};

// steps 4 to 6 on one used set; false: degenerate
bool fit_set(const std::vector<Pt> &pts, int radius, int band, Fit &f)
{
    Moments m;
    const int64_t R2 = 65536ll * radius * radius;
    for (const Pt &p : pts) m.add(p.u, p.v, p.u * p.u + p.v * p.v - R2);
    const Move mv = finish(m, band);
    if (mv.degenerate) return false;
    f.mx = mv.mx, f.my = mv.my;
    f.d.resize(pts.size());
    int64_t se = 0;
    for (size_t i = 0; i < pts.size(); i++) {
        const int64_t U = 256 * pts[i].u - f.mx, V = 256 * pts[i].v - f.my;
        f.d[i] = (int64_t)isqrt64((uint64_t)(U * U) + (uint64_t)(V * V)); // rho for now
        se += f.d[i] - 65536ll * radius;
    }
    f.r = 65536ll * radius + rdiv(se, (int64_t)pts.size());
    for (int64_t &d : f.d) d = (d - f.r + 128) >> 8;
    return true;
}

} // namespace

extern "C" int canny_hip_circle_fits_from_plane(const unsigned char *bits, const void *plane, int plane_is_u8, int height,
                                                int width, const int *circles, int n_circles, int band, int trim_q8,
                                                int options, int *fits)
{
    if (!bits || !plane || n_circles < 0 || (n_circles && (!circles || !fits)) || band < 0 || trim_q8 < 0 ||
        (options & ~3) || height < 2 || width < 2)
        return CANNY_HIP_ERR_INVALID;
    if (height > CANNY_HIP_CIRCLE_FIT_MAX_AXIS || width > CANNY_HIP_CIRCLE_FIT_MAX_AXIS || band > CANNY_HIP_CIRCLE_FIT_MAX_BAND)
        return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t row_bytes = ((size_t)width + 7) / 8;
    std::vector<unsigned> px; // the set pixels of E as indices, raster order
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7)) & 1) px.push_back((unsigned)(y * width + x));
    std::vector<unsigned> sel;
    std::vector<int> edgels;
    std::vector<Pt> pts, kept;
    for (int j = 0; j < n_circles; j++) {
        const int *rec = circles + (size_t)j * CANNY_HIP_CIRCLE_INTS;
        int *out = fits + (size_t)j * CANNY_HIP_CIRCLE_FIT_INTS;
        std::memset(out, 0, CANNY_HIP_CIRCLE_FIT_INTS * sizeof(int));
        const int x2 = rec[0], y2 = rec[1], radius = rec[2];
        if (radius < 1 || radius > CANNY_HIP_CIRCLES_MAX_RADIUS || x2 < 0 || x2 >= 2 * width || y2 < 0 || y2 >= 2 * height) {
            out[4] = (int)CANNY_HIP_CIRCLE_FIT_INVALID;
            continue;
        }
        // step 2: the pixels of the band
        const int lo = radius - band > 1 ? radius - band : 1;
        const int64_t lo2 = (int64_t)(2 * lo - 1) * (2 * lo - 1);
        const int64_t hi2 = (int64_t)(2 * (radius + band) + 1) * (2 * (radius + band) + 1);
        sel.clear();
        for (unsigned p : px) {
            const int64_t dx = 2ll * (int)(p % (unsigned)width) - x2, dy = 2ll * (int)(p / (unsigned)width) - y2;
            const int64_t d = dx * dx + dy * dy;
            if (d >= lo2 && d < hi2) sel.push_back(p);
        }
        // step 3: their edgels, gated
        edgels.resize(sel.size() * CANNY_HIP_EDGEL_INTS + 1);
        const int rc = canny_hip_edgels_from_plane(plane, plane_is_u8, height, width, sel.data(), sel.size(), edgels.data());
        if (rc) return rc;
        pts.clear();
        for (size_t i = 0; i < sel.size(); i++) {
            const int *e = edgels.data() + i * CANNY_HIP_EDGEL_INTS;
            if (options & CANNY_HIP_CIRCLE_FIT_GATE) {
                const int64_t gx = (int16_t)((uint32_t)e[2] & 0xffffu), gy = (int16_t)((uint32_t)e[2] >> 16);
                const int64_t wx = 2ll * (int)(sel[i] % (unsigned)width) - x2, wy = 2ll * (int)(sel[i] / (unsigned)width) - y2;
                const int64_t dot = gx * wx + gy * wy;
                if (!(gx | gy) || 4 * dot * dot < 3 * (gx * gx + gy * gy) * (wx * wx + wy * wy)) continue;
            }
            if ((options & CANNY_HIP_CIRCLE_FIT_REFINED_ONLY) && !((uint32_t)e[3] & CANNY_HIP_EDGEL_REFINED)) continue;
            pts.push_back(Pt{(int64_t)e[0] - 128ll * x2, (int64_t)e[1] - 128ll * y2});
        }
        Fit f;
        if (!fit_set(pts, radius, band, f)) {
            out[0] = (int)(32768ll * x2), out[1] = (int)(32768ll * y2), out[2] = 65536 * radius, out[3] = (int)pts.size();
            out[4] = (int)CANNY_HIP_CIRCLE_FIT_DEGENERATE;
            continue;
        }
        uint32_t flags = 0;
        const std::vector<Pt> *used = &pts;
        if (trim_q8 > 0) {
            kept.clear();
            for (size_t i = 0; i < pts.size(); i++)
                if ((f.d[i] < 0 ? -f.d[i] : f.d[i]) <= trim_q8) kept.push_back(pts[i]);
            Fit g;
            if (fit_set(kept, radius, band, g))
                f = g, used = &kept;
            else
                flags = CANNY_HIP_CIRCLE_FIT_TRIM_FAILED;
        }
        uint64_t sdd = 0;
        int64_t maxd = 0;
        uint32_t sectors = 0;
        for (size_t i = 0; i < used->size(); i++) {
            const int64_t d = f.d[i], ad = d < 0 ? -d : d;
            sdd += (uint64_t)(d * d);
            if (ad > maxd) maxd = ad;
            sectors |= 1u << sector_of(256 * (*used)[i].u - f.mx, 256 * (*used)[i].v - f.my);
        }
        out[0] = (int)(32768ll * x2 + f.mx), out[1] = (int)(32768ll * y2 + f.my), out[2] = (int)f.r;
        out[3] = (int)used->size();
        out[4] = (int)(((uint32_t)maxd & CANNY_HIP_CIRCLE_FIT_MAXD_MASK) | flags);
        out[5] = (int)sectors;
        out[6] = (int)(uint32_t)sdd, out[7] = (int)(uint32_t)(sdd >> 32);
    }
    return CANNY_HIP_OK;
}

// Host-only test hook: steps 4 and 5 on moment sets, outputs as canny_hip_dev_circle_fits_arith.
extern "C" int canny_hip_circle_fits_finish(const long long *moments, size_t n_sets, int *out)
{
    if (!n_sets || !moments || !out) return CANNY_HIP_ERR_INVALID;
    for (size_t i = 0; i < n_sets; i++) {
        const long long *p = moments + CANNY_HIP_CIRCLE_FIT_MOMENT_WORDS * i;
        Moments m;
        m.n = p[0], m.su = p[1], m.sv = p[2], m.sz = p[3], m.suu = p[4], m.suv = p[5], m.svv = p[6];
        m.suz = (i128)(((unsigned __int128)(uint64_t)p[8] << 64) | (uint64_t)p[7]);
        m.svz = (i128)(((unsigned __int128)(uint64_t)p[10] << 64) | (uint64_t)p[9]);
        const Move f = finish(m, (int)p[11]);
        int *o = out + 4 * i;
        o[0] = (int)f.mx, o[1] = (int)f.my, o[2] = (int)m.n, o[3] = f.degenerate ? (int)CANNY_HIP_CIRCLE_FIT_DEGENERATE : 0;
    }
    return CANNY_HIP_OK;
}
