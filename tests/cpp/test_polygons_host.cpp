// test_polygons_host.cpp -- canny_hip_polygons_from_chains (csrc/canny_polygons_host.cpp) on designed chains, with every
// buffer allocated at its exact size: built with the host compiler's -fsanitize=address,undefined together with that one
// source file, it shows that the host rule neither reads nor writes outside its buffers and computes without overflow.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_polygons_host.cpp canny_edge_amd/csrc/canny_polygons_host.cpp -o test_polygons_host
// No device, no library: the program has its own main and links nothing else.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "canny_hip.h"

namespace {

const int kWidth = 32768, kHeight = 32768; // the largest frame: the cross products reach their bound

int failures = 0;

void expect(bool ok, const char *what, int line)
{
    if (ok) return;
    fprintf(stderr, "FAILED line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

int px(int x, int y) { return y * kWidth + x; }

// a one-pixel-wide horizontal line of n pixels as the border follower walks it: out and back, 2 n - 2 points (1 for n = 1)
std::vector<int> line_chain(int x0, int y, int n)
{
    std::vector<int> c;
    for (int i = 0; i < n; i++) c.push_back(px(x0 + i, y));
    for (int i = n - 2; i >= 1; i--) c.push_back(px(x0 + i, y));
    return c;
}

// the border of a filled rectangle, clockwise from its top-left pixel
std::vector<int> rectangle_chain(int x0, int y0, int w, int h)
{
    std::vector<int> c;
    for (int x = x0; x < x0 + w; x++) c.push_back(px(x, y0));
    for (int y = y0 + 1; y < y0 + h; y++) c.push_back(px(x0 + w - 1, y));
    for (int x = x0 + w - 2; x >= x0; x--) c.push_back(px(x, y0 + h - 1));
    for (int y = y0 + h - 2; y > y0; y--) c.push_back(px(x0, y));
    return c;
}

struct Result {
    int status;
    std::vector<unsigned long long> vertex_offsets;
    std::vector<int> vertices;
    std::vector<long long> measures;
};

// every buffer lives on the heap at exactly the size the call may touch
Result run(const std::vector<std::vector<int>> &chains, unsigned long long point_capacity, unsigned eps_q8, unsigned ratio_q16,
           unsigned long long vertex_capacity, bool want_measures)
{
    const size_t k = chains.size();
    std::unique_ptr<unsigned long long[]> co(new unsigned long long[k + 1]);
    co[0] = 0;
    for (size_t j = 0; j < k; j++) co[j + 1] = co[j] + chains[j].size();
    const unsigned long long stored = co[k] < point_capacity ? co[k] : point_capacity;
    std::unique_ptr<int[]> pts(new int[stored]);
    unsigned long long at = 0;
    for (const auto &c : chains)
        for (int p : c) {
            if (at < stored) pts[at] = p;
            at++;
        }
    std::unique_ptr<unsigned long long[]> voff(new unsigned long long[k + 1]);
    std::unique_ptr<int[]> verts(new int[vertex_capacity]);
    std::unique_ptr<long long[]> meas(new long long[4 * k]);
    Result r;
    r.status = canny_hip_polygons_from_chains(co.get(), stored ? pts.get() : nullptr, k, stored, kWidth, kHeight, eps_q8,
                                              ratio_q16, voff.get(), vertex_capacity ? verts.get() : nullptr,
                                              vertex_capacity, want_measures ? meas.get() : nullptr);
    if (r.status) return r;
    r.vertex_offsets.assign(voff.get(), voff.get() + k + 1);
    const unsigned long long fit = voff[k] < vertex_capacity ? voff[k] : vertex_capacity;
    r.vertices.assign(verts.get(), verts.get() + fit);
    if (want_measures) r.measures.assign(meas.get(), meas.get() + 4 * k);
    return r;
}

} // namespace

int main()
{
    // chains of 1, 2, 62, 64 and 66 points, a rectangle in the far corner of the largest frame, an L
    std::vector<std::vector<int>> chains = {line_chain(5, 3, 1),  line_chain(9, 5, 2),   line_chain(0, 7, 32),
                                            line_chain(100, 9, 33), line_chain(32768 - 34, 11, 34),
                                            rectangle_chain(32768 - 40, 32768 - 25, 40, 25)};
    std::vector<int> l_chain; // an L: (0,100) -> (20,100) -> (20,110) -> (50,110) -> (50,120) -> (0,120), pixel by pixel
    {
        const int cx[7] = {0, 20, 20, 50, 50, 0, 0}, cy[7] = {100, 100, 110, 110, 120, 120, 100};
        for (int s = 0; s < 6; s++) {
            int x = cx[s], y = cy[s];
            while (x != cx[s + 1] || y != cy[s + 1]) {
                l_chain.push_back(px(x, y));
                x += (cx[s + 1] > x) - (cx[s + 1] < x), y += (cy[s + 1] > y) - (cy[s + 1] < y);
            }
        }
    }
    chains.push_back(l_chain);
    unsigned long long total = 0;
    for (const auto &c : chains) total += c.size();
    EXPECT(chains[0].size() == 1 && chains[1].size() == 2 && chains[2].size() == 62 && chains[3].size() == 64 &&
           chains[4].size() == 66 && chains[5].size() == 126);

    const unsigned tolerances[][2] = {{0, 0}, {256, 0}, {512, 0}, {0, 1311}, {384, 655}, {1u << 24, 0}, {0xFFFFFFFFu, 65535}};
    for (const auto &tol : tolerances) {
        const Result r = run(chains, total, tol[0], tol[1], total, true);
        EXPECT(r.status == 0);
        if (r.status) continue;
        const long long *m = r.measures.data();
        EXPECT(m[0] == 1 && m[1] == 0 && m[2] == 0 && m[3] == 0);                    // one pixel
        EXPECT(m[4] == 2 && m[5] == 512 && m[6] == 0 && m[7] == 0);                  // two pixels
        for (int j = 2; j <= 4; j++) EXPECT(m[4 * j] == 2 && m[4 * j + 2] == 0 && m[4 * j + 3] == 0);
        EXPECT(m[4 * 2 + 1] == 256 * 62 && m[4 * 3 + 1] == 256 * 64 && m[4 * 4 + 1] == 256 * 66);
        EXPECT(r.vertices[3] == px(0, 7) && r.vertices[4] == px(31, 7));             // a line: its two end points
        const bool huge = tol[0] >= (1u << 24);
        EXPECT(m[4 * 5] == (huge ? 2 : 4) && m[4 * 5 + 1] == 256 * 126);
        if (!huge) EXPECT(m[4 * 5 + 2] == 2 * 39 * 24 && m[4 * 5 + 3] == 1);         // the rectangle: corners, convex
        if (!huge) EXPECT(m[4 * 6] == 6 && m[4 * 6 + 2] == 2 * (50 * 10 + 20 * 10) && m[4 * 6 + 3] == 0); // the L
        EXPECT(r.vertex_offsets.back() == r.vertices.size());
        // exact-size and cut vertex buffers, measures absent: the same prefix
        const unsigned long long caps[] = {r.vertex_offsets.back(), r.vertex_offsets.back() - 1, 5, 1, 0};
        for (unsigned long long cap : caps) {
            const Result c = run(chains, total, tol[0], tol[1], cap, false);
            EXPECT(c.status == 0 && c.vertex_offsets == r.vertex_offsets && c.vertices.size() == cap);
            for (size_t q = 0; q < c.vertices.size(); q++) EXPECT(c.vertices[q] == r.vertices[q]);
        }
        // a point buffer that cuts the rectangle: it and the L are incomplete
        const Result cut = run(chains, total - l_chain.size() - 7, tol[0], tol[1], total, true);
        EXPECT(cut.status == 0 && cut.measures[4 * 5] == -1 && cut.measures[4 * 6] == -1 && cut.measures[4 * 6 + 1] == 0);
        EXPECT(cut.vertex_offsets[7] == cut.vertex_offsets[5] && cut.vertex_offsets[5] == r.vertex_offsets[5]);
        const Result none = run(chains, 0, tol[0], tol[1], 0, true);
        EXPECT(none.status == 0 && none.vertex_offsets.back() == 0 && none.measures[0] == -1);
    }
    EXPECT(run({}, 0, 0, 0, 0, true).status == 0);
    EXPECT(run(chains, total, 0, 65536, total, true).status == CANNY_HIP_ERR_INVALID);
    if (failures) return 1;
    printf("polygons_from_chains: designed chains ok\n");
    return 0;
}
