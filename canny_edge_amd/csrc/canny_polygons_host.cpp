// canny_polygons_host.cpp -- canny_hip_polygons_from_chains: the polygon rule of include/canny_hip.h
// on chains in host memory, in plain C++.  No HIP in this file: it is part of libcanny_hip.so, and tests/cpp/
// test_polygons_host.cpp compiles it on its own under the host compiler's sanitizers.
#include <algorithm>
#include <utility>
#include <vector>

#include "canny_hip.h"

// The rule in plain C++: the recursion on an explicit stack of runs, one flag per chain position.
int canny_hip_polygons_from_chains(const unsigned long long *chain_offsets, const int *points,
                                   unsigned long long n_records, unsigned long long point_capacity, int width, int height,
                                   unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *vertex_offsets,
                                   int *vertices, unsigned long long vertex_capacity, long long *measures)
{
    if (!chain_offsets || (!points && point_capacity) || !vertex_offsets || (!vertices && vertex_capacity) ||
        ratio_q16 >= 65536u)
        return CANNY_HIP_ERR_INVALID;
    if (height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    if (height > 32768 || width > 32768) return CANNY_HIP_ERR_UNSUPPORTED; // every cross product stays below 2^31
    using u64 = unsigned long long;
    auto cross = [](long long ax, long long ay, long long bx, long long by) { return ax * by - ay * bx; };
    std::vector<unsigned char> flag;
    std::vector<std::pair<u64, u64>> runs;
    std::vector<int> vx, vy;
    u64 total = 0;
    vertex_offsets[0] = 0;
    for (u64 j = 0; j < n_records; j++) {
        const u64 begin = chain_offsets[j], end = chain_offsets[j + 1];
        long long *m = measures ? measures + 4 * j : nullptr;
        if (end > point_capacity || end < begin) {
            if (m) m[0] = -1, m[1] = 0, m[2] = 0, m[3] = 0;
            vertex_offsets[j + 1] = total;
            continue;
        }
        const u64 n = end - begin;
        const int *p = points + begin;
        auto X = [&](u64 i) { return p[i == n ? 0 : i] % width; };
        auto Y = [&](u64 i) { return p[i == n ? 0 : i] / width; };
        u64 n_axis = 0, n_diag = 0, k = 0;
        long long far = -1;
        for (u64 i = 0; i < n; i++) {
            const int dx = X(i + 1) - X(i), dy = Y(i + 1) - Y(i);
            n_diag += dx != 0 && dy != 0;
            n_axis += (dx != 0) != (dy != 0);
            const long long ex = X(i) - X(0), ey = Y(i) - Y(0), d2 = ex * ex + ey * ey;
            if (d2 > far) far = d2, k = i;
        }
        const u64 length_q8 = 256 * n_axis + 362 * n_diag;
        const u64 eps = std::min<u64>((u64)epsilon_q8 + (((u64)ratio_q16 * length_q8) >> 16), 1ull << 24);
        flag.assign((size_t)n, 0);
        runs.clear();
        if (n) flag[0] = 1, flag[(size_t)k] = 1;
        if (n >= 2) runs.push_back({k, n}), runs.push_back({0, k});
        while (!runs.empty()) {
            const u64 a = runs.back().first, b = runs.back().second;
            runs.pop_back();
            if (b - a < 2) continue;
            const long long bx = X(b) - X(a), by = Y(b) - Y(a);
            u64 at = a + 1, best = 0;
            for (u64 i = a + 1; i < b; i++) {
                const long long c = cross(bx, by, X(i) - X(a), Y(i) - Y(a));
                const u64 ci = (u64)(c < 0 ? -c : c);
                if (ci > best) best = ci, at = i;
            }
            const unsigned __int128 lhs = (unsigned __int128)(best * best) << 16;
            const unsigned __int128 rhs = (unsigned __int128)(eps * eps) * (u64)(bx * bx + by * by);
            if (!(lhs > rhs)) continue;
            flag[(size_t)at] = 1;
            runs.push_back({at, b}), runs.push_back({a, at});
        }
        vx.clear(), vy.clear();
        for (u64 i = 0; i < n; i++) {
            if (!flag[(size_t)i]) continue;
            if (total + vx.size() < vertex_capacity) vertices[total + vx.size()] = p[i];
            vx.push_back(X(i)), vy.push_back(Y(i));
        }
        const size_t v = vx.size();
        total += v;
        vertex_offsets[j + 1] = total;
        if (!m) continue;
        long long area = 0;
        bool pos = false, neg = false;
        for (size_t i = 0; i < v; i++) {
            const size_t i1 = (i + 1) % v, i2 = (i + 2) % v;
            area += cross(vx[i], vy[i], vx[i1], vy[i1]);
            const long long t = cross(vx[i1] - vx[i], vy[i1] - vy[i], vx[i2] - vx[i1], vy[i2] - vy[i1]);
            pos |= t > 0, neg |= t < 0;
        }
        m[0] = (long long)v, m[1] = (long long)length_q8, m[2] = area < 0 ? -area : area;
        m[3] = v >= 3 && pos != neg ? 1 : 0;
    }
    return CANNY_HIP_OK;
}
