// canny_corners_host.cpp -- canny_hip_corners_from_plane and canny_hip_corner_response_of: the corner rule of
// include/canny_hip.h in plain C++ on one host u8 plane.  No device, no HIP: what the CPU tests pin
// against tests/corners_rule.py, and what tests/cpp/test_corners_host.cpp compiles under the host compiler's sanitizers.
// The kernels of canny_corners.hip are written separately from this file on purpose; the GPU tests compare both with the
// Python rule.
#include "canny_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

// ceil(sqrt(v)), exact, v < 2^54
int64_t ceil_sqrt(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return (int64_t)(r + (r * r < v));
}

int64_t response_of(int64_t sxx, int64_t syy, int64_t sxy, int mode, int k_q8)
{
    if (mode == CANNY_HIP_CORNERS_MIN_EIGEN) {
        const int64_t d = sxx - syy;
        return sxx + syy - ceil_sqrt((uint64_t)(d * d) + 4u * (uint64_t)(sxy * sxy));
    }
    const int64_t tr = sxx + syy;
    return 256 * (sxx * syy - sxy * sxy) - (int64_t)k_q8 * tr * tr;
}

bool bad_mode(int mode, int k_q8)
{
    return (mode != CANNY_HIP_CORNERS_MIN_EIGEN && mode != CANNY_HIP_CORNERS_HARRIS) || k_q8 < 0 ||
           k_q8 > CANNY_HIP_CORNERS_MAX_K_Q8 || (mode == CANNY_HIP_CORNERS_MIN_EIGEN && k_q8 != 0);
}

// the reference's Sobel pair with its border rules (calculateXYGradient)
void sobel_pair(const unsigned char *img, int h, int w, int y, int x, int *gx, int *gy)
{
    const int cl = x > 0 ? x - 1 : 0, cr = x < w - 1 ? x + 1 : w - 1;
    const int ru = y > 0 ? y - 1 : 0, rd = y < h - 1 ? y + 1 : h - 1;
    const unsigned char *row = img + (size_t)y * w, *up = img + (size_t)ru * w, *dn = img + (size_t)rd * w;
    int v = 2 * row[cr] - 2 * row[cl];
    if (y != h - 1) v += dn[cr] - dn[cl];
    if (y != 0) v += up[cr] - up[cl];
    int u = 2 * dn[x] - 2 * up[x];
    if (x != w - 1) u += dn[cr] - up[cr];
    if (x != 0) u += dn[cl] - up[cl];
    *gx = v, *gy = u;
}

} // namespace

extern "C" int canny_hip_corner_response_of(int sxx, int syy, int sxy, int mode, int k_q8, long long *r)
{
    const int M = CANNY_HIP_CORNERS_MAX_SUM;
    if (!r || bad_mode(mode, k_q8) || sxx < 0 || sxx > M || syy < 0 || syy > M || sxy < -M || sxy > M)
        return CANNY_HIP_ERR_INVALID;
    *r = response_of(sxx, syy, sxy, mode, k_q8);
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_corners_from_plane(const unsigned char *plane, int height, int width, int mode, int block,
                                            int k_q8, int quality_q16, long long min_response, int min_dist,
                                            int corners_max, long long *corners, int *count, int *cand_count,
                                            long long *max_response, long long *response)
{
    if (!plane || !corners || !count || height < 2 || width < 2 || bad_mode(mode, k_q8) ||
        (block != 3 && block != 5 && block != 7) || quality_q16 < 0 || quality_q16 > 65536 || min_response < 0 ||
        min_dist < 0 || corners_max < 1 || ((uintptr_t)corners & 7) || ((uintptr_t)response & 7))
        return CANNY_HIP_ERR_INVALID;
    const long long hw = (long long)height * width;
    if (corners_max > CANNY_HIP_HOUGH_MAX_LINES || hw >= 0x80000000LL) return CANNY_HIP_ERR_UNSUPPORTED;

    const int r = block / 2;
    std::vector<int> pxx((size_t)hw), pyy((size_t)hw), pxy((size_t)hw);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            int gx, gy;
            sobel_pair(plane, height, width, y, x, &gx, &gy);
            const size_t i = (size_t)y * width + x;
            pxx[i] = gx * gx, pyy[i] = gy * gy, pxy[i] = gx * gy;
        }
    std::vector<long long> own;
    long long *R = response;
    if (!R) {
        own.resize((size_t)hw);
        R = own.data();
    }
    long long rmax = LLONG_MIN;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            int64_t sxx = 0, syy = 0, sxy = 0;
            for (int v = std::max(0, y - r); v <= std::min(height - 1, y + r); v++)
                for (int u = std::max(0, x - r); u <= std::min(width - 1, x + r); u++) {
                    const size_t i = (size_t)v * width + u;
                    sxx += pxx[i], syy += pyy[i], sxy += pxy[i];
                }
            const long long val = response_of(sxx, syy, sxy, mode, k_q8);
            R[(size_t)y * width + x] = val;
            rmax = std::max(rmax, val);
        }
    // thr = floor(max(Rmax, 0) * q / 65536), exactly: Rmax = a * 65536 + b
    const uint64_t m = (uint64_t)std::max<long long>(rmax, 0), q = (uint64_t)quality_q16;
    const long long thr = (long long)((m >> 16) * q + (((m & 0xffffu) * q) >> 16));
    const long long cut = std::max<long long>(std::max(thr, min_response), 1);
    std::vector<std::pair<long long, long long>> cand; // (-R, base)
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const long long v = R[i];
            if (v < cut) continue;
            bool ok = true;
            for (int dy = -1; dy <= 1 && ok; dy++)
                for (int dx = -1; dx <= 1 && ok; dx++) {
                    const int yy = y + dy, xx = x + dx;
                    if ((!dy && !dx) || yy < 0 || yy >= height || xx < 0 || xx >= width) continue;
                    const long long o = R[(size_t)yy * width + xx];
                    ok = (dy < 0 || (dy == 0 && dx < 0)) ? v > o : v >= o;
                }
            if (ok) cand.emplace_back(-v, (long long)i);
        }
    std::sort(cand.begin(), cand.end());
    const size_t M = std::min<size_t>((size_t)corners_max, cand.size());
    std::vector<int> ax, ay;
    const long long md2 = (long long)min_dist * min_dist;
    int n_acc = 0;
    for (size_t c = 0; c < M; c++) {
        const int y = (int)(cand[c].second / width), x = (int)(cand[c].second % width);
        bool near = false;
        for (size_t j = 0; j < ax.size() && !near; j++) {
            const long long dx = x - ax[j], dy = y - ay[j];
            near = dx * dx + dy * dy < md2;
        }
        if (near) continue;
        ax.push_back(x);
        ay.push_back(y);
        long long *rec = corners + (size_t)n_acc * CANNY_HIP_CORNER_WORDS;
        rec[0] = x, rec[1] = y, rec[2] = -cand[c].first, rec[3] = (long long)c;
        n_acc++;
    }
    *count = n_acc;
    if (cand_count) *cand_count = (int)std::min<size_t>(cand.size(), 0x7fffffff);
    if (max_response) *max_response = rmax;
    return CANNY_HIP_OK;
}
