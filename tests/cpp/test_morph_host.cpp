// Stand-alone check of csrc/canny_morph_host.cpp (own main; built by tests/test_morph_rule.py with the host compiler's address
// and undefined-behaviour sanitizers, together with that one file): every op, border and shape against a restatement written
// here straight from the definitions, asymmetric and random elements up to 31 x 31, dirty pad bits, widths around the byte,
// sixteen iterations, the typed-out ellipse and refused calls -- all with buffers of exactly the needed size.
#include "canny_hip.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

typedef std::vector<unsigned char> Bytes;
typedef std::vector<int> Px;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Element {
    std::vector<unsigned> rows;
    int kw, kh;
};

// one primitive on one unpacked frame, straight from the definition
static Px primitive(const Px &in, int h, int w, const Element &e, bool erode, int outside)
{
    Px out((size_t)h * w);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int v = erode ? 1 : 0;
            for (int j = 0; j < e.kh; j++)
                for (int i = 0; i < e.kw; i++) {
                    if (!((e.rows[j] >> i) & 1u)) continue;
                    const int dx = i - e.kw / 2, dy = j - e.kh / 2;
                    const int xx = erode ? x + dx : x - dx, yy = erode ? y + dy : y - dy;
                    const int s = xx < 0 || xx >= w || yy < 0 || yy >= h ? outside : in[(size_t)yy * w + xx];
                    v = erode ? (v & s) : (v | s);
                }
            out[(size_t)y * w + x] = v;
        }
    return out;
}

static Px repeat(Px a, int h, int w, const Element &e, bool erode, int border, int iterations)
{
    const int outside = border == CANNY_HIP_MORPH_BORDER_NEUTRAL ? (erode ? 1 : 0) : border;
    for (int k = 0; k < iterations; k++) a = primitive(a, h, w, e, erode, outside);
    return a;
}

static Px expected(const Px &in, int h, int w, int op, const Element &e, int border, int it)
{
    Px r;
    switch (op) {
    case CANNY_HIP_MORPH_ERODE: return repeat(in, h, w, e, true, border, it);
    case CANNY_HIP_MORPH_DILATE: return repeat(in, h, w, e, false, border, it);
    case CANNY_HIP_MORPH_OPEN: return repeat(repeat(in, h, w, e, true, border, it), h, w, e, false, border, it);
    case CANNY_HIP_MORPH_CLOSE: return repeat(repeat(in, h, w, e, false, border, it), h, w, e, true, border, it);
    case CANNY_HIP_MORPH_GRADIENT: {
        const Px d = repeat(in, h, w, e, false, border, it), er = repeat(in, h, w, e, true, border, it);
        r.resize(in.size());
        for (size_t i = 0; i < in.size(); i++) r[i] = d[i] & (er[i] ^ 1);
        return r;
    }
    case CANNY_HIP_MORPH_TOPHAT: {
        const Px o = expected(in, h, w, CANNY_HIP_MORPH_OPEN, e, border, it);
        r.resize(in.size());
        for (size_t i = 0; i < in.size(); i++) r[i] = in[i] & (o[i] ^ 1);
        return r;
    }
    default: {
        const Px c = expected(in, h, w, CANNY_HIP_MORPH_CLOSE, e, border, it);
        r.resize(in.size());
        for (size_t i = 0; i < in.size(); i++) r[i] = c[i] & (in[i] ^ 1);
        return r;
    }
    }
}

static int one_case(int n, int h, int w, int op, const Element &e, int border, int it, uint32_t seed, int density, bool with_counts)
{
    const int rb = (w + 7) / 8;
    Bytes bits((size_t)n * h * rb), out(bits.size(), 0x5A);
    for (auto &b : bits) b = 0;
    std::vector<Px> frames(n, Px((size_t)h * w));
    for (int f = 0; f < n; f++)
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                const int v = (int)((lcg(seed) >> 16) % 100u) < density;
                frames[f][(size_t)y * w + x] = v;
                if (v) bits[((size_t)f * h + y) * rb + (x >> 3)] |= (unsigned char)(0x80u >> (x & 7));
            }
            if (w % 8) bits[((size_t)f * h + y) * rb + rb - 1] |= (unsigned char)((lcg(seed) >> 8) & (0xFFu >> (w % 8))); // dirty pad bits
        }
    std::vector<long long> counts(n, -7);
    CHECK(canny_hip_morph_bits(bits.data(), n, h, w, op, e.rows.data(), e.kw, e.kh, border, it, out.data(),
                               with_counts ? counts.data() : nullptr) == CANNY_HIP_OK);
    for (int f = 0; f < n; f++) {
        const Px want = expected(frames[f], h, w, op, e, border, it);
        long long set = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < rb * 8; x++) {
                const int got = (out[((size_t)f * h + y) * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
                CHECK(got == (x < w ? want[(size_t)y * w + x] : 0)); // pad bits are written 0
                set += got;
            }
        CHECK(counts[f] == (with_counts ? set : -7));
    }
    return 0;
}

int main()
{
    // the shapes
    unsigned rows[31];
    CHECK(canny_hip_morph_element(CANNY_HIP_MORPH_ELLIPSE, 5, 5, rows) == CANNY_HIP_OK);
    CHECK(rows[0] == 4 && rows[1] == 14 && rows[2] == 31 && rows[3] == 14 && rows[4] == 4);
    CHECK(canny_hip_morph_element(CANNY_HIP_MORPH_CROSS, 3, 5, rows) == CANNY_HIP_OK);
    CHECK(rows[0] == 2 && rows[1] == 2 && rows[2] == 7 && rows[3] == 2 && rows[4] == 2);
    CHECK(canny_hip_morph_element(CANNY_HIP_MORPH_RECT, 31, 31, rows) == CANNY_HIP_OK);
    for (int j = 0; j < 31; j++) CHECK(rows[j] == 0x7FFFFFFFu);
    CHECK(canny_hip_morph_element(CANNY_HIP_MORPH_ELLIPSE, 31, 1, rows) == CANNY_HIP_OK && rows[0] == 0x7FFFFFFFu);
    CHECK(canny_hip_morph_element(3, 3, 3, rows) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_morph_element(0, 2, 3, rows) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_morph_element(0, 33, 3, rows) == CANNY_HIP_ERR_INVALID);
    CHECK(canny_hip_morph_element(0, 3, 3, nullptr) == CANNY_HIP_ERR_INVALID);

    std::vector<Element> elements;
    for (int shape = 0; shape < 3; shape++)
        for (int k : {1, 3, 5, 9}) {
            Element e{std::vector<unsigned>((size_t)(k == 9 ? 5 : k)), k, k == 9 ? 5 : k};
            CHECK(canny_hip_morph_element(shape, e.kw, e.kh, e.rows.data()) == CANNY_HIP_OK);
            elements.push_back(e);
        }
    elements.push_back(Element{{1, 1, 1, 1, 31}, 5, 5});                  // an L
    elements.push_back(Element{{7, 5, 7}, 3, 3});                         // a ring, the centre unset
    elements.push_back(Element{{0x55555555u}, 31, 1});                    // alternating bits
    Element far_bit{std::vector<unsigned>(31, 0u), 31, 31};               // the single offset (+15, -15)
    far_bit.rows[0] = 1u << 30;
    elements.push_back(far_bit);
    uint32_t seed = 34;
    Element random{std::vector<unsigned>(31), 31, 31};
    for (auto &r : random.rows) r = lcg(seed) & lcg(seed) & 0x7FFFFFFFu;
    random.rows[30] |= 1u;
    elements.push_back(random);

    int k = 0;
    for (const Element &e : elements)
        for (int op = 0; op <= CANNY_HIP_MORPH_BLACKHAT; op++)
            for (int border = 0; border <= CANNY_HIP_MORPH_BORDER_NEUTRAL; border++, k++) {
                const int ws[] = {1, 7, 8, 9, 17, 33}, hs[] = {1, 2, 9, 20};
                if (one_case(1 + k % 3, hs[k % 4], ws[k % 6], op, e, border, 1 + k % 3, 100u + k, (5 + 45 * (k % 3)), k % 4 != 3)) return 1;
            }
    if (one_case(2, 23, 37, CANNY_HIP_MORPH_CLOSE, elements[1], CANNY_HIP_MORPH_BORDER_NEUTRAL, 16, 9, 10, true)) return 1;
    if (one_case(1, 40, 70, CANNY_HIP_MORPH_GRADIENT, random, CANNY_HIP_MORPH_BORDER_ONE, 2, 10, 50, true)) return 1;

    // refused calls write nothing
    {
        Bytes in(2 * 6 * 2, 0xFF), out(in.size(), 0x5A);
        long long counts[3] = {-7, -7, -7};
        const unsigned good[3] = {7, 7, 7}, high[3] = {7, 8, 7}, none[3] = {0, 0, 0};
        struct {
            const unsigned char *in;
            int n, h, w, op;
            const unsigned *rows;
            int kw, kh, border, it;
            unsigned char *out;
            long long *counts;
            int want;
        } bad[] = {
            {nullptr, 2, 6, 9, 2, good, 3, 3, 2, 1, out.data(), counts, 1}, {in.data(), 2, 6, 9, 2, good, 3, 3, 2, 1, nullptr, counts, 1},
            {in.data(), 2, 6, 9, 2, nullptr, 3, 3, 2, 1, out.data(), counts, 1}, {in.data(), 0, 6, 9, 2, good, 3, 3, 2, 1, out.data(), counts, 1},
            {in.data(), 2, 0, 9, 2, good, 3, 3, 2, 1, out.data(), counts, 1}, {in.data(), 2, 6, 0, 2, good, 3, 3, 2, 1, out.data(), counts, 1},
            {in.data(), 2, 6, 9, 7, good, 3, 3, 2, 1, out.data(), counts, 1}, {in.data(), 2, 6, 9, -1, good, 3, 3, 2, 1, out.data(), counts, 1},
            {in.data(), 2, 6, 9, 2, high, 3, 3, 2, 1, out.data(), counts, 1}, {in.data(), 2, 6, 9, 2, none, 3, 3, 2, 1, out.data(), counts, 1},
            {in.data(), 2, 6, 9, 2, good, 2, 3, 2, 1, out.data(), counts, 1}, {in.data(), 2, 6, 9, 2, good, 3, 33, 2, 1, out.data(), counts, 1},
            {in.data(), 2, 6, 9, 2, good, 3, 3, 3, 1, out.data(), counts, 1}, {in.data(), 2, 6, 9, 2, good, 3, 3, 2, 0, out.data(), counts, 1},
            {in.data(), 2, 6, 9, 2, good, 3, 3, 2, 17, out.data(), counts, 1}, {in.data(), 2, 6, 9, 2, good, 3, 3, 2, 1, in.data() + 5, counts, 1},
            {in.data(), 2, 6, 9, 2, good, 3, 3, 2, 1, out.data(), (long long *)((char *)counts + 4), 1},
            {in.data(), 2, 32769, 9, 2, good, 3, 3, 2, 1, out.data(), counts, 2}, {in.data(), 65536, 6, 9, 2, good, 3, 3, 2, 1, out.data(), counts, 2},
        };
        for (const auto &b : bad) {
            CHECK(canny_hip_morph_bits(b.in, b.n, b.h, b.w, b.op, b.rows, b.kw, b.kh, b.border, b.it, b.out, b.counts) == b.want);
            for (unsigned char v : out) CHECK(v == 0x5A);
            for (unsigned char v : in) CHECK(v == 0xFF);
            CHECK(counts[0] == -7 && counts[1] == -7 && counts[2] == -7);
        }
        CHECK(canny_hip_morph_bits(in.data(), 2, 6, 9, 0, good, 3, 3, CANNY_HIP_MORPH_BORDER_ONE, 16, out.data(), counts) == CANNY_HIP_OK);
        CHECK(counts[0] == 54 && counts[1] == 54 && counts[2] == -7); // ones stay ones; the dirty pad bits are not counted
    }
    std::printf("morph ok\n");
    return 0;
}
