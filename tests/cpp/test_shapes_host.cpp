// test_shapes_host.cpp -- canny_hip_shapes_from_chains (csrc/canny_shapes_host.cpp) on designed chains, with every buffer
// allocated at its exact size: built with the host compiler's -fsanitize=address,undefined together with that one source
// file, it shows that the host rule neither reads nor writes outside its buffers and computes without signed overflow.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_shapes_host.cpp canny_edge_amd/csrc/canny_shapes_host.cpp -o test_shapes_host
// No device, no library: the program has its own main and links nothing else.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "canny_hip.h"

namespace {

const int kWidth = 32767, kHeight = 32767; // the largest frame: the moments reach their bound
const int W = CANNY_HIP_SHAPE_WORDS;

int failures = 0;

void expect(bool ok, const char *what, int line)
{
    if (ok) return;
    fprintf(stderr, "FAILED line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

int px(int x, int y) { return y * kWidth + x; }

// the closed walk through the corners (cx[i], cy[i]), pixel by pixel: every edge is horizontal, vertical or diagonal
std::vector<int> walk(const std::vector<int> &cx, const std::vector<int> &cy)
{
    std::vector<int> c;
    const size_t k = cx.size();
    for (size_t s = 0; s < k; s++) {
        int x = cx[s], y = cy[s];
        const int tx = cx[(s + 1) % k], ty = cy[(s + 1) % k];
        while (x != tx || y != ty) {
            c.push_back(px(x, y));
            x += (tx > x) - (tx < x), y += (ty > y) - (ty < y);
        }
    }
    if (c.empty()) c.push_back(px(cx[0], cy[0]));
    return c;
}

// (x0, y0) -> (x0 + a, y0) -> (x0 + a + b, y0 + b) -> (x0, y0 + b): 2 a + 3 b points, clockwise on the screen
std::vector<int> trapezoid(int x0, int y0, int a, int b)
{
    return walk({x0, x0 + a, x0 + a + b, x0}, {y0, y0, y0 + b, y0 + b});
}

std::vector<int> rectangle(int x0, int y0, int w, int h)
{
    return walk({x0, x0 + w - 1, x0 + w - 1, x0}, {y0, y0, y0 + h - 1, y0 + h - 1});
}

struct Result {
    int status;
    std::vector<unsigned long long> hull_offsets;
    std::vector<int> hull;
    std::vector<long long> measures;
};

// every buffer lives on the heap at exactly the size the call may touch
Result run(const std::vector<std::vector<int>> &chains, unsigned long long point_capacity, unsigned long long hull_capacity,
           bool want_measures, int width = kWidth, int height = kHeight)
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
    std::unique_ptr<unsigned long long[]> hoff(new unsigned long long[k + 1]);
    std::unique_ptr<int[]> hull(new int[hull_capacity]);
    std::unique_ptr<long long[]> meas(new long long[W * k]);
    Result r;
    r.status = canny_hip_shapes_from_chains(co.get(), stored ? pts.get() : nullptr, k, stored, width, height, hoff.get(),
                                            hull_capacity ? hull.get() : nullptr, hull_capacity,
                                            want_measures ? meas.get() : nullptr);
    if (r.status) return r;
    r.hull_offsets.assign(hoff.get(), hoff.get() + k + 1);
    const unsigned long long fit = hoff[k] < hull_capacity ? hoff[k] : hull_capacity;
    r.hull.assign(hull.get(), hull.get() + fit);
    if (want_measures) r.measures.assign(meas.get(), meas.get() + W * k);
    return r;
}

} // namespace

int main()
{
    // chains of 1, 2, 63, 64 and 65 points, a rectangle in the far corner of the largest frame, and the frame's own border
    std::vector<std::vector<int>> chains = {walk({5}, {3}),          walk({9, 10}, {5, 5}),
                                            trapezoid(100, 7, 30, 1), trapezoid(200, 9, 29, 2),
                                            trapezoid(300, 20, 31, 1), rectangle(32767 - 40, 32767 - 25, 40, 25),
                                            rectangle(0, 0, 32767, 32767)};
    unsigned long long total = 0;
    for (const auto &c : chains) total += c.size();
    EXPECT(chains[0].size() == 1 && chains[1].size() == 2 && chains[2].size() == 63 && chains[3].size() == 64 &&
           chains[4].size() == 65 && chains[5].size() == 126 && chains[6].size() == 4 * 32766);

    const Result r = run(chains, total, total, true);
    EXPECT(r.status == 0);
    if (r.status) return 1;
    const long long *m = r.measures.data();
    // one pixel: a hull of one vertex, everything else zero
    EXPECT(m[0] == 1 && m[1] == 1 && m[2] == px(5, 3));
    for (int t = 3; t < W; t++) EXPECT(m[t] == 0);
    // two pixels, walked out and back: a segment
    m += W;
    EXPECT(m[0] == 2 && m[1] == 2 && m[2] == px(9, 5) && m[CANNY_HIP_SHAPE_AREA2] == 0 && m[CANNY_HIP_SHAPE_S10] == 1 &&
           m[CANNY_HIP_SHAPE_S20] == 1 && m[CANNY_HIP_SHAPE_S01] == 0 && m[CANNY_HIP_SHAPE_HULL_AREA2] == 0);
    EXPECT(m[CANNY_HIP_SHAPE_RECT_EDGE] == 0 && m[CANNY_HIP_SHAPE_RECT_ALONG_MIN] == 0 &&
           m[CANNY_HIP_SHAPE_RECT_ALONG_MAX] == 1 && m[CANNY_HIP_SHAPE_RECT_ACROSS] == 0 && m[CANNY_HIP_SHAPE_RECT_LEN2] == 1);
    EXPECT(r.hull[1] == px(9, 5) && r.hull[2] == px(10, 5));
    // the trapezoids: four hull vertices from the top-left corner on, area2 = 2 a b + b^2
    const int ab[3][2] = {{30, 1}, {29, 2}, {31, 1}};
    for (int j = 0; j < 3; j++) {
        m += W;
        const long long a = ab[j][0], b = ab[j][1];
        EXPECT(m[0] == 4 && m[1] == 2 * a + 3 * b && m[CANNY_HIP_SHAPE_AREA2] == 2 * a * b + b * b);
        EXPECT(m[CANNY_HIP_SHAPE_HULL_AREA2] == 2 * a * b + b * b);
        // the box on the long side (edge 2, from (a + b, b) back to (0, b)) is the smallest: (a + b) by b
        EXPECT(m[CANNY_HIP_SHAPE_RECT_EDGE] == 0 || m[CANNY_HIP_SHAPE_RECT_EDGE] == 2);
        EXPECT(m[CANNY_HIP_SHAPE_RECT_ACROSS] * (m[CANNY_HIP_SHAPE_RECT_ALONG_MAX] - m[CANNY_HIP_SHAPE_RECT_ALONG_MIN]) ==
               (a + b) * b * m[CANNY_HIP_SHAPE_RECT_LEN2]);
        EXPECT(m[CANNY_HIP_SHAPE_RECT_EDGE] == 0); // ties go to the smaller edge: edge 0 is parallel to edge 2
        const unsigned long long at = r.hull_offsets[2 + j];
        EXPECT(r.hull_offsets[3 + j] - at == 4 && r.hull[at] == m[2]);
    }
    // the rectangle in the far corner: its corners, the closed forms of its moments about its own corner
    m += W;
    {
        const long long a = 39, b = 24;
        EXPECT(m[0] == 4 && m[1] == 126 && m[2] == px(32767 - 40, 32767 - 25) && m[CANNY_HIP_SHAPE_AREA2] == 2 * a * b);
        EXPECT(m[CANNY_HIP_SHAPE_M10_6] == 3 * a * a * b && m[CANNY_HIP_SHAPE_M01_6] == 3 * a * b * b);
        EXPECT(m[CANNY_HIP_SHAPE_M20_12] == 4 * a * a * a * b && m[CANNY_HIP_SHAPE_M02_12] == 4 * a * b * b * b);
        EXPECT(m[CANNY_HIP_SHAPE_M11_24] == 6 * a * a * b * b && m[CANNY_HIP_SHAPE_HULL_AREA2] == 2 * a * b);
        EXPECT(m[CANNY_HIP_SHAPE_RECT_EDGE] == 0 && m[CANNY_HIP_SHAPE_RECT_ALONG_MIN] == 0 &&
               m[CANNY_HIP_SHAPE_RECT_ALONG_MAX] == a * a && m[CANNY_HIP_SHAPE_RECT_ACROSS] == a * b &&
               m[CANNY_HIP_SHAPE_RECT_LEN2] == a * a);
        const unsigned long long at = r.hull_offsets[5];
        EXPECT(r.hull[at] == px(32727, 32742) && r.hull[at + 1] == px(32766, 32742) && r.hull[at + 2] == px(32766, 32766) &&
               r.hull[at + 3] == px(32727, 32766));
    }
    // the border of the largest frame: the largest moments an outer border has; they fit
    m += W;
    {
        const long long a = 32766;
        EXPECT(m[0] == 4 && m[CANNY_HIP_SHAPE_AREA2] == 2 * a * a && m[CANNY_HIP_SHAPE_M20_12] == 4 * a * a * a * a);
        EXPECT(m[CANNY_HIP_SHAPE_M11_24] == 6 * a * a * a * a && m[CANNY_HIP_SHAPE_RECT_ACROSS] == a * a);
    }
    EXPECT(r.hull_offsets.back() == r.hull.size() && r.hull.size() == 1 + 2 + 3 * 4 + 4 + 4);
    // exact-size and cut hull buffers, measures absent: the same prefix
    const unsigned long long caps[] = {r.hull_offsets.back(), r.hull_offsets.back() - 1, 5, 1, 0};
    for (unsigned long long cap : caps) {
        const Result c = run(chains, total, cap, false);
        EXPECT(c.status == 0 && c.hull_offsets == r.hull_offsets && c.hull.size() == cap);
        for (size_t q = 0; q < c.hull.size(); q++) EXPECT(c.hull[q] == r.hull[q]);
    }
    // a point buffer that cuts the far rectangle: it and the frame's border are incomplete
    const Result cut = run(chains, total - chains[6].size() - 7, total, true);
    EXPECT(cut.status == 0 && cut.measures[W * 5] == -1 && cut.measures[W * 6] == -1 && cut.measures[W * 6 + 1] == 0);
    EXPECT(cut.hull_offsets[7] == cut.hull_offsets[5] && cut.hull_offsets[5] == r.hull_offsets[5]);
    for (int t = 0; t < W * 5; t++) EXPECT(cut.measures[t] == r.measures[t]);
    const Result none = run(chains, 0, 0, true);
    EXPECT(none.status == 0 && none.hull_offsets.back() == 0 && none.measures[0] == -1 && none.measures[1] == 0);
    EXPECT(run({}, 0, 0, true).status == 0);
    EXPECT(run(chains, total, total, true, 32768, 100).status == CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(run(chains, total, total, true, 100, 32768).status == CANNY_HIP_ERR_UNSUPPORTED);
    EXPECT(run(chains, total, total, true, 0, 100).status == CANNY_HIP_ERR_INVALID);
    if (failures) return 1;
    printf("shapes_from_chains: designed chains ok\n");
    return 0;
}
