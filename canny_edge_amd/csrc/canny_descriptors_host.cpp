// canny_descriptors_host.cpp -- canny_hip_descriptor_pattern, canny_hip_corner_descriptors_from_plane and
// canny_hip_match_descriptors: the descriptor and matching rule of include/canny_hip.h in plain C++
// on host buffers.  No device, no HIP: what the CPU tests pin against tests/descriptors_rule.py, and what
// tests/cpp/test_descriptors_host.cpp compiles under the host compiler's sanitizers.  The kernels of canny_descriptors.hip
// are written separately from this file on purpose; the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const signed char kPattern[CANNY_HIP_DESC_ROTATIONS * CANNY_HIP_DESC_BITS * 4] = {
#include "canny_desc_pattern.h"
};

const int kCos[9] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0};

int cos_q14(int k)
{
    k &= 31;
    if (k > 16) k = 32 - k;
    return k <= 8 ? kCos[k] : -kCos[16 - k];
}

int popcount64(uint64_t v)
{
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}

int distance_of(const unsigned long long *a, const unsigned long long *b)
{
    return popcount64(a[0] ^ b[0]) + popcount64(a[1] ^ b[1]) + popcount64(a[2] ^ b[2]) + popcount64(a[3] ^ b[3]);
}

} // namespace

extern "C" int canny_hip_descriptor_pattern(int k, signed char *out)
{
    if (!out || k < 0 || k >= CANNY_HIP_DESC_ROTATIONS) return CANNY_HIP_ERR_INVALID;
    std::memcpy(out, kPattern + (size_t)k * CANNY_HIP_DESC_BITS * 4, CANNY_HIP_DESC_BITS * 4);
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_corner_descriptors_from_plane(const unsigned char *plane, int height, int width,
                                                       const long long *corners, int count, int options,
                                                       unsigned long long *desc, int *meta)
{
    if (!plane || !desc || !meta || count < 0 || (count && !corners) || height < 2 || width < 2 ||
        (options & ~CANNY_HIP_DESC_STEERED) || ((uintptr_t)corners & 7) || ((uintptr_t)desc & 7))
        return CANNY_HIP_ERR_INVALID;
    if (count > CANNY_HIP_HOUGH_MAX_LINES || (long long)height * width >= 0x80000000LL) return CANNY_HIP_ERR_UNSUPPORTED;
    const int R = CANNY_HIP_DESC_RADIUS;
    for (int c = 0; c < count; c++) {
        const long long x = corners[(size_t)c * CANNY_HIP_CORNER_WORDS], y = corners[(size_t)c * CANNY_HIP_CORNER_WORDS + 1];
        unsigned long long *words = desc + (size_t)c * CANNY_HIP_DESC_WORDS;
        words[0] = words[1] = words[2] = words[3] = 0;
        if (x < 0 || x >= width || y < 0 || y >= height) {
            meta[c] = -1;
            continue;
        }
        const int cx = (int)x, cy = (int)y;
        auto at = [&](int yy, int xx) -> int {
            yy = std::min(std::max(yy, 0), height - 1);
            xx = std::min(std::max(xx, 0), width - 1);
            return plane[(size_t)yy * width + xx];
        };
        int k = 0;
        if (options & CANNY_HIP_DESC_STEERED) {
            int64_t m10 = 0, m01 = 0;
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++)
                    if (dx * dx + dy * dy <= R * R) {
                        const int v = at(cy + dy, cx + dx);
                        m10 += dx * v, m01 += dy * v;
                    }
            int64_t best = 0;
            for (int i = 0; i < CANNY_HIP_DESC_ROTATIONS; i++) {
                const int64_t s = m10 * cos_q14(i) + m01 * cos_q14(i - 8);
                if (i == 0 || s > best) best = s, k = i;
            }
        }
        const signed char *pat = kPattern + (size_t)k * CANNY_HIP_DESC_BITS * 4;
        for (int t = 0; t < CANNY_HIP_DESC_BITS; t++, pat += 4)
            if (at(cy + pat[1], cx + pat[0]) < at(cy + pat[3], cx + pat[2])) words[t / 64] |= 1ull << (t % 64);
        const int border = cx - R < 0 || cy - R < 0 || cx + R > width - 1 || cy + R > height - 1;
        meta[c] = k + 256 * border;
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_match_descriptors(const unsigned long long *q_desc, int n_q, const unsigned long long *t_desc,
                                           int n_t, int max_distance, int ratio_q8, int options, int *matches,
                                           int *accepted)
{
    if (n_q < 0 || n_t < 0 || (n_q && (!q_desc || !matches)) || (n_t && !t_desc) || !accepted || max_distance < 0 ||
        max_distance > CANNY_HIP_DESC_BITS || ratio_q8 < 0 || ratio_q8 > 256 || (options & ~CANNY_HIP_MATCH_CROSS_CHECK) ||
        ((uintptr_t)q_desc & 7) || ((uintptr_t)t_desc & 7))
        return CANNY_HIP_ERR_INVALID;
    if (n_q > CANNY_HIP_HOUGH_MAX_LINES || n_t > CANNY_HIP_HOUGH_MAX_LINES) return CANNY_HIP_ERR_UNSUPPORTED;
    const int none = CANNY_HIP_DESC_BITS + 1;
    // per train descriptor the query with the smallest (d, i)
    std::vector<int> back((size_t)n_t, -1), back_d((size_t)n_t, none);
    std::vector<int> j1((size_t)n_q, -1), d1((size_t)n_q, none), d2((size_t)n_q, none);
    for (int i = 0; i < n_q; i++)
        for (int j = 0; j < n_t; j++) {
            const int d = distance_of(q_desc + (size_t)i * 4, t_desc + (size_t)j * 4);
            if (d < d1[i]) d2[i] = d1[i], d1[i] = d, j1[i] = j;
            else if (d < d2[i]) d2[i] = d;
            if (d < back_d[j]) back_d[j] = d, back[j] = i;
        }
    int n_acc = 0;
    for (int i = 0; i < n_q; i++) {
        const bool f0 = d1[i] <= max_distance, f1 = ratio_q8 == 0 || d1[i] * 256 < ratio_q8 * d2[i];
        const bool mutual = j1[i] >= 0 && back[j1[i]] == i;
        const bool acc = f0 && f1 && (mutual || !(options & CANNY_HIP_MATCH_CROSS_CHECK));
        int *m = matches + (size_t)i * CANNY_HIP_MATCH_WORDS;
        m[0] = j1[i], m[1] = d1[i], m[2] = d2[i], m[3] = f0 | f1 << 1 | mutual << 2 | acc << 3;
        n_acc += acc;
    }
    *accepted = n_acc;
    return CANNY_HIP_OK;
}
