// canny_chamfer_host.cpp -- canny_hip_chamfer_from_dist2 and canny_hip_chamfer_cost_of: the chamfer-matching rule of
// include/canny_hip.h in plain C++ on one host dist2 plane with host template arrays.  No device, no
// HIP: what the CPU tests pin against tests/chamfer_rule.py, and what tests/cpp/test_chamfer_host.cpp compiles under the
// host compiler's sanitizers.  The kernels of canny_chamfer.hip are written separately from this file on purpose; the GPU
// tests compare both with the Python rule.
#include "canny_hip.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

// floor(sqrt(v)), exact, v < 2^53
uint64_t isqrt64(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

unsigned cost_of(int d2, int trunc_q4)
{
    const uint64_t r = isqrt64((uint64_t)(unsigned)d2 * 256u);
    return (unsigned)std::min<uint64_t>(r, (uint64_t)trunc_q4);
}

} // namespace

extern "C" int canny_hip_chamfer_cost_of(int d2, int trunc_q4)
{
    if (d2 < 0 || trunc_q4 < 1 || trunc_q4 > CANNY_HIP_CHAMFER_MAX_TRUNC) return -1;
    return (int)cost_of(d2, trunc_q4);
}

extern "C" int canny_hip_chamfer_from_dist2(const int *dist2, int height, int width, const int *offsets, const short *points,
                                            int n_templates, int trunc_q4, int max_mean_q4, int min_dist, int matches_max,
                                            int *matches, int *count, int *cand_count, unsigned int *scores)
{
    if (!dist2 || !offsets || !points || !count || height < 1 || width < 1 || n_templates < 1 || trunc_q4 < 1 ||
        max_mean_q4 < 0 || max_mean_q4 >= trunc_q4 || min_dist < 0 || matches_max < 1 || offsets[0] != 0)
        return CANNY_HIP_ERR_INVALID;
    if (n_templates > CANNY_HIP_CHAMFER_MAX_TEMPLATES || trunc_q4 > CANNY_HIP_CHAMFER_MAX_TRUNC ||
        matches_max > CANNY_HIP_HOUGH_MAX_LINES)
        return CANNY_HIP_ERR_UNSUPPORTED;
    for (int t = 0; t < n_templates; t++) {
        if (offsets[t + 1] <= offsets[t]) return CANNY_HIP_ERR_INVALID; // K_t >= 1
        if (offsets[t + 1] - offsets[t] > CANNY_HIP_CHAMFER_MAX_POINTS || offsets[t + 1] > CANNY_HIP_CHAMFER_MAX_TOTAL)
            return CANNY_HIP_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < 2 * offsets[n_templates]; k++)
        if (points[k] < -CANNY_HIP_CHAMFER_MAX_EXTENT || points[k] > CANNY_HIP_CHAMFER_MAX_EXTENT)
            return CANNY_HIP_ERR_UNSUPPORTED;
    const long long hw = (long long)height * width;
    if (hw * n_templates >= 0x80000000LL) return CANNY_HIP_ERR_UNSUPPORTED;

    std::vector<uint16_t> cost((size_t)hw);
    for (long long i = 0; i < hw; i++) cost[(size_t)i] = (uint16_t)cost_of(dist2[i], trunc_q4); // read as unsigned
    std::vector<unsigned> own;
    unsigned *S = scores;
    if (!S) {
        own.resize((size_t)(hw * n_templates));
        S = own.data();
    }
    for (int t = 0; t < n_templates; t++)
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                unsigned sum = 0;
                for (int k = offsets[t]; k < offsets[t + 1]; k++) {
                    const int px = x + points[2 * k], py = y + points[2 * k + 1];
                    sum += (px >= 0 && px < width && py >= 0 && py < height) ? cost[(size_t)py * width + px]
                                                                             : (unsigned)trunc_q4;
                }
                S[(size_t)t * hw + (size_t)y * width + x] = sum;
            }
    std::vector<std::pair<uint64_t, unsigned>> cand; // (mean_q12, base)
    for (int t = 0; t < n_templates; t++) {
        const unsigned K = (unsigned)(offsets[t + 1] - offsets[t]);
        const unsigned *P = S + (size_t)t * hw;
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t i = (size_t)y * width + x;
                const unsigned s = P[i];
                if (s > (unsigned)max_mean_q4 * K) continue;
                if (x > 0 && !(s < P[i - 1])) continue;
                if (x < width - 1 && !(s <= P[i + 1])) continue;
                if (y > 0 && !(s < P[i - width])) continue;
                if (y < height - 1 && !(s <= P[i + width])) continue;
                cand.emplace_back((uint64_t)s * 256u / K, (unsigned)((size_t)t * hw + i));
            }
    }
    std::sort(cand.begin(), cand.end());
    const size_t M = std::min<size_t>((size_t)matches_max, cand.size());
    std::vector<int> ax, ay;
    const long long md2 = (long long)min_dist * min_dist;
    int n_acc = 0;
    for (size_t c = 0; c < M; c++) {
        const unsigned base = cand[c].second;
        const int t = (int)(base / hw), y = (int)((base % hw) / width), x = (int)(base % width);
        bool near = false;
        for (size_t j = 0; j < ax.size() && !near; j++) {
            const long long dx = x - ax[j], dy = y - ay[j];
            near = dx * dx + dy * dy < md2;
        }
        if (near) continue;
        ax.push_back(x);
        ay.push_back(y);
        if (matches) {
            int *rec = matches + (size_t)n_acc * CANNY_HIP_MATCH_INTS;
            rec[0] = x, rec[1] = y, rec[2] = t, rec[3] = (int)S[base], rec[4] = (int)cand[c].first, rec[5] = (int)base;
        }
        n_acc++;
    }
    *count = n_acc;
    if (cand_count) *cand_count = (int)std::min<size_t>(cand.size(), 0x7fffffff);
    return CANNY_HIP_OK;
}
