// test_curves_host.cpp -- canny_hip_curves_from_bits (csrc/canny_curves_host.cpp) on designed masks, random maps and frames
// one pixel wide or high, with every buffer allocated at its exact size: built with the host compiler's
// -fsanitize=address,undefined together with that one source file, it shows that the host rule neither reads nor writes
// outside its buffers and computes without signed overflow.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tests/cpp/test_curves_host.cpp canny_edge_amd/csrc/canny_curves_host.cpp -o test_curves_host
// No device, no library: the program has its own main and links nothing else.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "canny_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line)
{
    if (ok) return;
    fprintf(stderr, "FAILED line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

struct Map {
    int h, w;
    std::vector<unsigned char> px; // one byte per pixel
    Map(int hh, int ww) : h(hh), w(ww), px((size_t)hh * ww, 0) {}
    explicit Map(const std::vector<std::string> &rows) : h((int)rows.size()), w((int)rows[0].size()), px((size_t)h * w, 0)
    {
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) px[(size_t)y * w + x] = rows[y][x] == '#';
    }
    unsigned char &at(int y, int x) { return px[(size_t)y * w + x]; }
    int set() const
    {
        int n = 0;
        for (unsigned char v : px) n += v;
        return n;
    }
};

struct Result {
    int status;
    unsigned long long count, point_count;
    std::vector<int> records, points;
    std::vector<unsigned long long> chain;
};

// the packed map at its exact size (padding bits set: they are ignored), every output at its exact size on the heap
Result run(const Map &m, int min_length, long long capacity = -1, long long point_capacity = -1)
{
    const size_t row_bytes = ((size_t)m.w + 7) / 8;
    std::unique_ptr<unsigned char[]> bits(new unsigned char[(size_t)m.h * row_bytes]);
    for (int y = 0; y < m.h; y++)
        for (size_t b = 0; b < row_bytes; b++) {
            unsigned v = 0;
            for (int i = 0; i < 8; i++) {
                const size_t x = b * 8 + i;
                v = (v << 1) | (x < (size_t)m.w ? m.px[(size_t)y * m.w + x] : 1u);
            }
            bits[(size_t)y * row_bytes + b] = (unsigned char)v;
        }
    Result r{};
    r.status = canny_hip_curves_from_bits(bits.get(), m.h, m.w, min_length, nullptr, 0, &r.count, nullptr, nullptr, 0,
                                          &r.point_count);
    if (r.status) return r;
    const unsigned long long total = r.count, total_points = r.point_count;
    const unsigned long long cap = capacity < 0 ? total : (unsigned long long)capacity;
    const unsigned long long pcap = point_capacity < 0 ? total_points : (unsigned long long)point_capacity;
    std::unique_ptr<int[]> rec(new int[(size_t)cap * CANNY_HIP_CURVE_RECORD]), pts(new int[(size_t)pcap]);
    std::unique_ptr<unsigned long long[]> chain(new unsigned long long[(size_t)cap + 1]);
    r.status = canny_hip_curves_from_bits(bits.get(), m.h, m.w, min_length, cap ? rec.get() : nullptr, cap, &r.count,
                                          chain.get(), pcap ? pts.get() : nullptr, pcap, &r.point_count);
    EXPECT(r.count == total && r.point_count == total_points);
    const unsigned long long fit = cap < total ? cap : total;
    r.chain.assign(chain.get(), chain.get() + fit + 1);
    r.records.assign(rec.get(), rec.get() + fit * CANNY_HIP_CURVE_RECORD);
    const unsigned long long pfit = r.chain[fit] < pcap ? r.chain[fit] : pcap;
    r.points.assign(pts.get(), pts.get() + pfit);
    return r;
}

int flags_of(const Result &r, size_t j) { return r.records[j * CANNY_HIP_CURVE_RECORD + CANNY_HIP_CURVE_FLAGS]; }
int points_of(const Result &r, size_t j) { return r.records[j * CANNY_HIP_CURVE_RECORD + CANNY_HIP_CURVE_POINTS]; }

// what follows from the rule and needs no reference: records and offsets agree, consecutive points are 8-neighbours, and
// the full output lists every set pixel
void check_consistent(const Map &m, const Result &r, bool everything)
{
    EXPECT(r.status == CANNY_HIP_OK);
    EXPECT(r.chain[0] == 0);
    std::vector<int> seen((size_t)m.h * m.w, 0);
    for (size_t j = 0; j + 1 < r.chain.size(); j++) {
        const unsigned long long b = r.chain[j], e = r.chain[j + 1];
        EXPECT(e > b && (long long)(e - b) == points_of(r, j));
        if (e > r.points.size()) continue; // cut by point_capacity
        EXPECT(r.points[b] == r.records[j * CANNY_HIP_CURVE_RECORD + CANNY_HIP_CURVE_START]);
        EXPECT(r.points[e - 1] == r.records[j * CANNY_HIP_CURVE_RECORD + CANNY_HIP_CURVE_END]);
        for (unsigned long long q = b; q < e; q++) {
            const int p = r.points[q];
            EXPECT(p >= 0 && p < m.h * m.w && m.px[p]);
            if (p >= 0 && p < m.h * m.w) seen[p]++;
            if (q > b) {
                const int dy = p / m.w - r.points[q - 1] / m.w, dx = p % m.w - r.points[q - 1] % m.w;
                EXPECT(dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1 && (dx || dy));
            }
        }
    }
    if (everything)
        for (size_t p = 0; p < seen.size(); p++) EXPECT((seen[p] > 0) == (m.px[p] != 0));
}

Map ring5()
{
    Map m(7, 7);
    for (int i = 1; i <= 5; i++) m.at(1, i) = m.at(5, i) = m.at(i, 1) = m.at(i, 5) = 1;
    return m;
}

Map diamond()
{
    Map m(11, 11);
    for (int i = 0; i < 5; i++) m.at(1 + i, 5 + i) = m.at(5 + i, 9 - i) = m.at(9 - i, 5 - i) = m.at(5 - i, 1 + i) = 1;
    return m;
}

Map random_map(int h, int w, unsigned seed, unsigned per_mille)
{
    Map m(h, w);
    unsigned s = seed * 2654435761u + 12345u;
    for (auto &v : m.px) {
        s = s * 1664525u + 1013904223u;
        v = (s >> 8) % 1000u < per_mille;
    }
    return m;
}

} // namespace

int main()
{
    { // the two rings: 16 points, CLOSED
        for (const Map &m : {ring5(), diamond()}) {
            const Result r = run(m, 1);
            check_consistent(m, r, true);
            EXPECT(r.count == 1 && r.point_count == 16);
            EXPECT((flags_of(r, 0) & 0xF) == CANNY_HIP_CURVE_CLOSED);
            EXPECT(run(m, 17).count == 0);
        }
    }
    { // plus, X, T: the junction ends every arm
        Map plus(9, 9), x(9, 9), t(8, 11);
        for (int i = 1; i <= 7; i++) plus.at(4, i) = plus.at(i, 4) = x.at(i, i) = x.at(i, 8 - i) = 1;
        for (int i = 1; i <= 9; i++) t.at(1, i) = 1;
        for (int i = 1; i <= 6; i++) t.at(i, 5) = 1;
        const Map *maps[3] = {&plus, &x, &t};
        const unsigned arms[3] = {4, 4, 3};
        for (int k = 0; k < 3; k++) {
            const Result r = run(*maps[k], 1);
            check_consistent(*maps[k], r, true);
            EXPECT(r.count == arms[k] && r.point_count == (unsigned)maps[k]->set() + arms[k] - 1);
            for (size_t j = 0; j < r.count; j++)
                EXPECT(!(flags_of(r, j) & CANNY_HIP_CURVE_START_JUNCTION) != !(flags_of(r, j) & CANNY_HIP_CURVE_END_JUNCTION));
        }
    }
    { // a loop on a junction, a figure-eight through one junction pixel, two adjacent nodes
        const Map lollipop({".........", "..####...", "..#..#...", "..#..#...", "..####...", "..#......", "..#......",
                            "........."});
        Result r = run(lollipop, 1);
        check_consistent(lollipop, r, true);
        EXPECT(r.count == 2 && r.point_count == (unsigned)lollipop.set() + 2);
        const Map eight({"......", "..#...", ".#.#..", "..#...", ".#.#..", "..#...", "......"});
        r = run(eight, 1);
        check_consistent(eight, r, true);
        EXPECT(r.count == 2 && points_of(r, 0) == 5 && points_of(r, 1) == 5);
        EXPECT(r.records[CANNY_HIP_CURVE_START] == r.records[CANNY_HIP_CURVE_END]);
        const Map two({".....", ".##..", "....."});
        r = run(two, 1);
        check_consistent(two, r, true);
        EXPECT(r.count == 1 && points_of(r, 0) == 2 && flags_of(r, 0) == 0);
        EXPECT(run(two, 3).count == 0);
    }
    { // all set, checkerboard, staircase
        Map all(8, 9), checker(8, 9), stairs(8, 9);
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 9; x++) {
                all.at(y, x) = 1;
                checker.at(y, x) = !((x | y) & 1);
                stairs.at(y, x) = x == y || x == y + 1;
            }
        Result r = run(all, 1);
        check_consistent(all, r, true);
        r = run(checker, 1);
        check_consistent(checker, r, true);
        EXPECT(r.count == 20 && r.point_count == 20 && flags_of(r, 0) == CANNY_HIP_CURVE_ISOLATED);
        r = run(stairs, 1);
        check_consistent(stairs, r, true);
        EXPECT(r.count == 1 && r.point_count == (unsigned)stairs.set());
    }
    { // frames one pixel wide or high
        const int dims[5][2] = {{1, 1}, {1, 70}, {70, 1}, {1, 8}, {2, 1}};
        for (const auto &d : dims) {
            Map m(d[0], d[1]);
            for (auto &v : m.px) v = 1;
            const Result r = run(m, 1);
            check_consistent(m, r, true);
            EXPECT(r.count == 1 && r.point_count == (unsigned)(d[0] * d[1]));
            Map gaps = m;
            for (size_t i = 2; i < gaps.px.size(); i += 3) gaps.px[i] = 0;
            check_consistent(gaps, run(gaps, 1), true);
        }
    }
    { // random maps: exact, halved and zero capacities, several min_length
        const unsigned dens[6] = {50, 200, 350, 500, 700, 900};
        for (unsigned k = 0; k < 6; k++)
            for (unsigned seed = 0; seed < 3; seed++) {
                const Map m = random_map(37, 53, 10 * k + seed, dens[k]);
                const Result full = run(m, 1);
                check_consistent(m, full, true);
                for (int min_length : {3, 10}) {
                    const Result kept = run(m, min_length);
                    check_consistent(m, kept, false);
                    EXPECT(kept.count <= full.count && kept.point_count <= full.point_count);
                    for (size_t j = 0; j < kept.count; j++) EXPECT(points_of(kept, j) >= min_length);
                }
                const Result half = run(m, 1, (long long)(full.count / 2), (long long)(full.point_count / 2));
                check_consistent(m, half, false);
                EXPECT(half.chain.size() == full.count / 2 + 1);
                for (size_t j = 0; j < half.chain.size(); j++) EXPECT(half.chain[j] == full.chain[j]);
                for (size_t q = 0; q < half.points.size(); q++) EXPECT(half.points[q] == full.points[q]);
                const Result cut = run(m, 1, -1, (long long)(full.point_count / 3));
                EXPECT(cut.points.size() == full.point_count / 3);
                for (size_t q = 0; q < cut.points.size(); q++) EXPECT(cut.points[q] == full.points[q]);
                const Result none = run(m, 1, 0, 0);
                EXPECT(none.status == CANNY_HIP_OK && none.chain.size() == 1 && none.chain[0] == 0);
            }
    }
    { // arguments
        unsigned char b[8] = {0};
        unsigned long long k = 0, p = 0;
        EXPECT(canny_hip_curves_from_bits(nullptr, 1, 8, 1, nullptr, 0, &k, nullptr, nullptr, 0, &p) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 1, 8, 1, nullptr, 0, nullptr, nullptr, nullptr, 0, &p) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 1, 8, 1, nullptr, 0, &k, nullptr, nullptr, 0, nullptr) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 1, 8, 1, nullptr, 1, &k, nullptr, nullptr, 0, &p) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 1, 8, 1, nullptr, 0, &k, nullptr, nullptr, 1, &p) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 0, 8, 1, nullptr, 0, &k, nullptr, nullptr, 0, &p) == CANNY_HIP_ERR_INVALID);
        EXPECT(canny_hip_curves_from_bits(b, 1 << 15, (1 << 13) + 1, 1, nullptr, 0, &k, nullptr, nullptr, 0, &p) ==
               CANNY_HIP_ERR_UNSUPPORTED);
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("test_curves_host: ok\n");
    return 0;
}
