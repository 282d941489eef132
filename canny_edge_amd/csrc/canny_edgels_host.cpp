// canny_edgels_host.cpp -- canny_hip_edgels_from_plane: the sub-pixel edgel rule of include/canny_hip.h in plain C++ on one
// host plane and one index list.  No device, no HIP: what the CPU tests pin against tests/edgels_rule.py, and what
// tests/cpp/test_edgels_host.cpp compiles on its own under the host compiler's sanitizers.  The kernels of
// canny_edgels.hip are written separately from this file on purpose; the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

// the reference's 3x3 pair with its border rules and its wrap through short
template <class T>
void sobel_pair_host(const T *img, int h, int w, int y, int x, int *gx, int *gy)
{
    const int cl = x > 0 ? x - 1 : 0, cr = x < w - 1 ? x + 1 : w - 1;
    const int ru = y > 0 ? y - 1 : 0, rd = y < h - 1 ? y + 1 : h - 1;
    const T *row = img + (size_t)y * w, *up = img + (size_t)ru * w, *dn = img + (size_t)rd * w;
    int v = 2 * row[cr] - 2 * row[cl];
    if (y != h - 1) v += dn[cr] - dn[cl];
    if (y != 0) v += up[cr] - up[cl];
    int u = 2 * dn[x] - 2 * up[x];
    if (x != w - 1) u += dn[cr] - up[cr];
    if (x != 0) u += dn[cl] - up[cl];
    *gx = (int)(int16_t)(uint16_t)(unsigned)v;
    *gy = (int)(int16_t)(uint16_t)(unsigned)u;
}

// floor(sqrt(256 * M)), exact
uint32_t mag_q4(int gx, int gy)
{
    const uint32_t m = (uint32_t)(gx * gx) + (uint32_t)(gy * gy); // gx, gy in [-32768, 32767]: each square <= 2^30
    const uint64_t v = (uint64_t)m << 8;
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return (uint32_t)r;
}

template <class T>
uint32_t mag_at(const T *img, int h, int w, int y, int x)
{
    int gx, gy;
    sobel_pair_host(img, h, w, y, x, &gx, &gy);
    return mag_q4(gx, gy);
}

template <class T>
void edgel(const T *img, int h, int w, uint32_t index, int *rec)
{
    if (index >= (uint32_t)h * (uint32_t)w) { // never an address
        rec[0] = rec[1] = rec[2] = 0;
        rec[3] = (int)CANNY_HIP_EDGEL_INVALID;
        return;
    }
    const int y = (int)(index / (uint32_t)w), x = (int)(index - (uint32_t)y * (uint32_t)w);
    int gx, gy;
    sobel_pair_host(img, h, w, y, x, &gx, &gy);
    const uint32_t b = mag_q4(gx, gy);
    int dir = 0, dx = 1, dy = 0;
    const uint32_t ax = (uint32_t)(gx < 0 ? -gx : gx), ay = (uint32_t)(gy < 0 ? -gy : gy);
    const uint32_t t22 = ax * 13573u, y15 = ay << 15, t67 = t22 + (ax << 16);
    if (y15 < t22) {
    } else if (y15 > t67) {
        dir = 2, dx = 0, dy = 1;
    } else if ((gx ^ gy) >= 0) {
        dir = 1, dx = 1, dy = 1;
    } else {
        dir = 3, dx = 1, dy = -1;
    }
    if (!(gx | gy)) dir = 0;
    int t = 0;
    uint32_t refined = 0;
    const int xa = x - dx, ya = y - dy, xc = x + dx, yc = y + dy;
    if ((gx | gy) && xa >= 0 && xc < w && ya >= 0 && ya < h && yc >= 0 && yc < h) {
        const uint32_t a = mag_at(img, h, w, ya, xa), c = mag_at(img, h, w, yc, xc);
        if (b >= a && b >= c && 2 * b > a + c) {
            const uint32_t dn = 2 * b - a - c, d = c >= a ? c - a : a - c;
            t = (int)((256u * d + dn) / (2u * dn));
            if (c < a) t = -t;
            refined = CANNY_HIP_EDGEL_REFINED;
        }
    }
    rec[0] = 256 * x + t * dx;
    rec[1] = 256 * y + t * dy;
    rec[2] = (int)(((uint32_t)gx & 0xffffu) | ((uint32_t)gy << 16));
    rec[3] = (int)(b | (uint32_t)dir << CANNY_HIP_EDGEL_DIR_SHIFT | refined);
}

} // namespace

extern "C" int canny_hip_edgels_from_plane(const void *plane, int plane_is_u8, int height, int width,
                                           const unsigned int *points, unsigned long long n_points, int *edgels)
{
    if (!plane || height < 2 || width < 2 || ((!points || !edgels) && n_points)) return CANNY_HIP_ERR_INVALID;
    if ((long long)height * width > 0x7fffffffLL) return CANNY_HIP_ERR_UNSUPPORTED;
    for (unsigned long long q = 0; q < n_points; q++) {
        if (plane_is_u8)
            edgel((const uint8_t *)plane, height, width, points[q], edgels + q * CANNY_HIP_EDGEL_INTS);
        else
            edgel((const int16_t *)plane, height, width, points[q], edgels + q * CANNY_HIP_EDGEL_INTS);
    }
    return CANNY_HIP_OK;
}
