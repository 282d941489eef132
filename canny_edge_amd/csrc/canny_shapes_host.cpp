// canny_shapes_host.cpp -- canny_hip_shapes_from_chains: the shape rule of include/canny_hip.h on
// chains in host memory, in plain C++.  No HIP in this file: it is part of libcanny_hip.so, and tests/cpp/
// test_shapes_host.cpp compiles it on its own under the host compiler's sanitizers.
#include <algorithm>
#include <vector>

#include "canny_hip.h"

// The rule in plain C++: the sums in unsigned 64-bit words (they wrap by definition), the hull by a sort of the distinct
// points and the monotone chain, the rectangle by trying every edge.
int canny_hip_shapes_from_chains(const unsigned long long *chain_offsets, const int *points, unsigned long long n_records,
                                 unsigned long long point_capacity, int width, int height, unsigned long long *hull_offsets,
                                 int *hull, unsigned long long hull_capacity, long long *measures)
{
    if (!chain_offsets || (!points && point_capacity) || !hull_offsets || (!hull && hull_capacity))
        return CANNY_HIP_ERR_INVALID;
    if (height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    if (height > 32767 || width > 32767) return CANNY_HIP_ERR_UNSUPPORTED;
    using u64 = unsigned long long;
    using i64 = long long;
    constexpr int W = CANNY_HIP_SHAPE_WORDS;
    struct Pt {
        i64 x, y;
    };
    auto cross = [](i64 ax, i64 ay, i64 bx, i64 by) { return ax * by - ay * bx; };
    std::vector<unsigned> keys;
    std::vector<Pt> h, half;
    u64 total = 0;
    hull_offsets[0] = 0;
    for (u64 j = 0; j < n_records; j++) {
        const u64 begin = chain_offsets[j], end = chain_offsets[j + 1];
        i64 *m = measures ? measures + W * j : nullptr;
        if (m) std::fill(m, m + W, 0ll);
        if (end > point_capacity || end < begin) {
            if (m) m[CANNY_HIP_SHAPE_HULL_VERTICES] = -1;
            hull_offsets[j + 1] = total;
            continue;
        }
        const u64 n = end - begin;
        if (!n) {
            hull_offsets[j + 1] = total;
            continue;
        }
        const int *p = points + begin;
        const i64 x0 = p[0] % width, y0 = p[0] / width;
        // ---- the eleven sums ----
        u64 s[11] = {0};
        keys.clear();
        for (u64 i = 0; i < n; i++) {
            const int pi = p[i], pn = p[i + 1 == n ? 0 : i + 1];
            const i64 u0 = pi % width - x0, v0 = pi / width - y0, u1 = pn % width - x0, v1 = pn / width - y0;
            const u64 a = (u64)(u0 * v1 - u1 * v0);
            s[0] += a;
            s[1] += a * (u64)(u0 + u1);
            s[2] += a * (u64)(v0 + v1);
            s[3] += a * (u64)(u0 * u0 + u0 * u1 + u1 * u1);
            s[4] += a * (u64)(2 * u0 * v0 + u0 * v1 + u1 * v0 + 2 * u1 * v1);
            s[5] += a * (u64)(v0 * v0 + v0 * v1 + v1 * v1);
            s[6] += (u64)u0, s[7] += (u64)v0, s[8] += (u64)(u0 * u0), s[9] += (u64)(u0 * v0), s[10] += (u64)(v0 * v0);
            keys.push_back((unsigned)(pi % width) << 16 | (unsigned)(pi / width)); // sorts by x, then y
        }
        // ---- the hull ----
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        h.clear();
        if (keys.size() == 1) {
            h.push_back(Pt{(i64)(keys[0] >> 16), (i64)(keys[0] & 0xFFFFu)});
        } else {
            for (int pass = 0; pass < 2; pass++) {
                half.clear();
                for (size_t t = 0; t < keys.size(); t++) {
                    const unsigned k = keys[pass ? keys.size() - 1 - t : t];
                    const Pt q{(i64)(k >> 16), (i64)(k & 0xFFFFu)};
                    while (half.size() >= 2) {
                        const Pt &a = half[half.size() - 2], &b = half.back();
                        if (cross(b.x - a.x, b.y - a.y, q.x - b.x, q.y - b.y) > 0) break;
                        half.pop_back();
                    }
                    half.push_back(q);
                }
                h.insert(h.end(), half.begin(), half.end() - 1);
            }
        }
        const size_t v = h.size();
        for (size_t k = 0; k < v; k++)
            if (total + k < hull_capacity) hull[total + k] = (int)(h[k].y * width + h[k].x);
        total += v;
        hull_offsets[j + 1] = total;
        if (!m) continue;
        m[CANNY_HIP_SHAPE_HULL_VERTICES] = (i64)v, m[CANNY_HIP_SHAPE_POINTS] = (i64)n, m[CANNY_HIP_SHAPE_ANCHOR] = p[0];
        for (int t = 0; t < 11; t++) m[CANNY_HIP_SHAPE_AREA2 + t] = (i64)s[t];
        if (v < 2) continue;
        // ---- the hull's area and the rectangle ----
        i64 area2 = 0;
        u64 best_en = 0, best_len2 = 0;
        for (size_t k = 0; k < v; k++) {
            const Pt &a = h[k], &b = h[(k + 1) % v];
            area2 += cross(a.x, a.y, b.x, b.y);
            const i64 dx = b.x - a.x, dy = b.y - a.y;
            i64 lo = 0, hi = 0, across = 0;
            for (size_t i = 0; i < v; i++) {
                const i64 ex = h[i].x - a.x, ey = h[i].y - a.y;
                const i64 al = ex * dx + ey * dy, ac = cross(dx, dy, ex, ey);
                lo = std::min(lo, al), hi = std::max(hi, al), across = std::max(across, ac);
            }
            const u64 en = (u64)(hi - lo) * (u64)across, len2 = (u64)(dx * dx + dy * dy);
            if (k == 0 || (unsigned __int128)en * best_len2 < (unsigned __int128)best_en * len2) {
                best_en = en, best_len2 = len2;
                m[CANNY_HIP_SHAPE_RECT_EDGE] = (i64)k, m[CANNY_HIP_SHAPE_RECT_ALONG_MIN] = lo;
                m[CANNY_HIP_SHAPE_RECT_ALONG_MAX] = hi, m[CANNY_HIP_SHAPE_RECT_ACROSS] = across;
                m[CANNY_HIP_SHAPE_RECT_LEN2] = (i64)len2;
            }
        }
        m[CANNY_HIP_SHAPE_HULL_AREA2] = area2;
    }
    return CANNY_HIP_OK;
}
