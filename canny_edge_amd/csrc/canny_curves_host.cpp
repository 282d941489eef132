// canny_curves_host.cpp -- canny_hip_curves_from_bits: the edge-curve rule of include/canny_hip.h on
// ONE bit map in host memory, in plain C++.  No HIP in this file: it is part of libcanny_hip.so, and tests/cpp/
// test_curves_host.cpp compiles it on its own under the host compiler's sanitizers.
#include <cstddef>
#include <vector>

#include "canny_hip.h"

// The rule in plain C++: a byte per pixel that holds the pixel's links (bit d = linked in direction d) on a map with a
// one-pixel border of zeros, then the curves in raster order of their first pixels and ascending first direction, which is
// the order of the keys.
int canny_hip_curves_from_bits(const unsigned char *bits, int height, int width, int min_length, int *records,
                               unsigned long long capacity, unsigned long long *count, unsigned long long *chain_offsets,
                               int *points, unsigned long long point_capacity, unsigned long long *point_count)
{
    if (!bits || !count || !point_count || (!chain_offsets && capacity) || (!points && point_capacity))
        return CANNY_HIP_ERR_INVALID;
    if (height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    if ((long long)height * width > (1ll << 28)) return CANNY_HIP_ERR_UNSUPPORTED;
    static const int dy[8] = {0, 1, 1, 1, 0, -1, -1, -1}, dx[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    const size_t row_bytes = ((size_t)width + 7) / 8, pitch = (size_t)width + 2;
    std::vector<unsigned char> set(((size_t)height + 2) * pitch, 0), link(set.size(), 0);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            set[((size_t)y + 1) * pitch + x + 1] = (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7))) & 1;
    std::ptrdiff_t step[8], index_step[8];
    for (int d = 0; d < 8; d++) {
        step[d] = dy[d] * (std::ptrdiff_t)pitch + dx[d]; // in the padded maps
        index_step[d] = dy[d] * (std::ptrdiff_t)width + dx[d]; // in r * width + c
    }
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t at = ((size_t)y + 1) * pitch + x + 1;
            if (!set[at]) continue;
            unsigned r = 0;
            for (int d = 0; d < 8; d++) r |= (unsigned)set[at + step[d]] << d;
            const unsigned rl = ((r << 1) | (r >> 7)) & 0xFFu, rr = ((r >> 1) | (r << 7)) & 0xFFu;
            link[at] = (unsigned char)(r & (0x55u | ~(rl | rr)) & 0xFFu);
        }
    auto degree = [](unsigned l) { return __builtin_popcount(l); };
    auto lowest = [](unsigned l) { return __builtin_ctz(l); };

    unsigned long long k = 0, total = 0;
    std::vector<int> curve;
    if (chain_offsets) chain_offsets[0] = 0;
    // the walk from padded position `at` (index p) along d: the pixels go to `curve`; returns false for a closed-curve
    // candidate that meets a node or a smaller index.  *last receives the direction of the step that reached the end.
    auto follow = [&](size_t at, int p, int d, bool closed, int *last) {
        curve.assign(1, p);
        int cur = p;
        *last = d;
        for (;;) {
            at += step[d], cur += (int)index_step[d];
            if (closed && cur == p) return true;
            const unsigned l = link[at];
            if (closed && (degree(l) != 2 || cur < p)) return false;
            curve.push_back(cur);
            *last = d;
            if (degree(l) != 2) return true;
            d = lowest(l & ~(1u << ((d + 4) & 7)));
        }
    };
    auto emit = [&](int flags) {
        if ((long long)curve.size() < (long long)min_length) return;
        if (k < capacity) {
            if (records) {
                int *rec = records + k * CANNY_HIP_CURVE_RECORD;
                rec[CANNY_HIP_CURVE_START] = curve.front(), rec[CANNY_HIP_CURVE_END] = curve.back();
                rec[CANNY_HIP_CURVE_POINTS] = (int)curve.size(), rec[CANNY_HIP_CURVE_FLAGS] = flags;
            }
            for (size_t i = 0; i < curve.size() && total + i < point_capacity; i++) points[total + i] = curve[i];
            chain_offsets[k + 1] = total + curve.size();
        }
        total += curve.size();
        k++;
    };
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t at = ((size_t)y + 1) * pitch + x + 1;
            if (!set[at]) continue;
            const int p = y * width + x;
            const unsigned l = link[at];
            const int deg = degree(l);
            int last = 0;
            if (deg == 0) {
                curve.assign(1, p);
                emit(CANNY_HIP_CURVE_ISOLATED);
            } else if (deg != 2) {
                for (unsigned rest = l; rest; rest &= rest - 1) {
                    const int d = lowest(rest);
                    follow(at, p, d, false, &last);
                    const int e = curve.back();
                    if (8ll * p + d > 8ll * e + ((last + 4) & 7)) continue; // emitted from the other end
                    const size_t e_at = ((size_t)(e / width) + 1) * pitch + (size_t)(e % width) + 1;
                    emit((d << CANNY_HIP_CURVE_FIRST_DIR_SHIFT) | (last << CANNY_HIP_CURVE_LAST_DIR_SHIFT) |
                         (deg >= 3 ? CANNY_HIP_CURVE_START_JUNCTION : 0) |
                         (degree(link[e_at]) >= 3 ? CANNY_HIP_CURVE_END_JUNCTION : 0));
                }
            } else if (!(l & 0xF0u)) {
                const int d = lowest(l);
                if (follow(at, p, d, true, &last))
                    emit(CANNY_HIP_CURVE_CLOSED | (d << CANNY_HIP_CURVE_FIRST_DIR_SHIFT) |
                         (last << CANNY_HIP_CURVE_LAST_DIR_SHIFT));
            }
        }
    *count = k;
    *point_count = total;
    return CANNY_HIP_OK;
}
