// test_recon_words.cpp -- csrc/canny_recon_words.h, the word steps of the reconstruction kernels, on the host: the occluded
// fill against the bit-by-bit flood on every single-run mask with every seed position, carries in from both sides and random
// words; the dilation step against a per-pixel restatement.  Compiled by tests/test_reconstruct_rule.py with the host
// compiler's sanitizers; nothing but the header is involved.
#include "canny_recon_words.h"

#include <cstdint>
#include <cstdio>
#include <random>

using canny::recon_fill;

// the flood, one pixel at a time, to the fixed point
static uint64_t fill_ref(uint64_t s, uint64_t g, bool lo, bool hi)
{
    if (lo) s |= g & 1ull;
    if (hi) s |= g & (1ull << 63);
    for (bool moved = true; moved;) {
        moved = false;
        for (int i = 0; i < 64; i++) {
            if (!(s >> i & 1)) continue;
            if (i > 0 && (g >> (i - 1) & 1) && !(s >> (i - 1) & 1)) s |= 1ull << (i - 1), moved = true;
            if (i < 63 && (g >> (i + 1) & 1) && !(s >> (i + 1) & 1)) s |= 1ull << (i + 1), moved = true;
        }
    }
    return s;
}

static int fails = 0;
static void check_fill(uint64_t s, uint64_t g, bool lo, bool hi)
{
    const uint64_t got = recon_fill(s, g, lo, hi), want = fill_ref(s, g, lo, hi);
    if (got != want && fails++ < 10)
        printf("fill s %016llx g %016llx carries %d %d: %016llx != %016llx\n", (unsigned long long)s, (unsigned long long)g, lo, hi,
               (unsigned long long)got, (unsigned long long)want);
}

static int bit(uint64_t v, int i) { return i < 0 || i > 63 ? 0 : (int)(v >> i & 1); }

int main()
{
    long n = 0;
    // every single run [a, b] and every seed position inside it, all four carry pairs; a second run next to it stays empty
    for (int a = 0; a < 64; a++)
        for (int b = a; b < 64; b++) {
            const uint64_t run = (b - a == 63 ? ~0ull : ((1ull << (b - a + 1)) - 1ull) << a);
            const uint64_t other = b + 2 < 64 ? ~0ull << (b + 2) : 0ull; // a run that no seed touches, behind one unset column
            for (int c = 0; c < 4; c++) {
                check_fill(0, run, c & 1, c >> 1), n++;
                for (int p = a; p <= b; p++) {
                    check_fill(1ull << p, run, c & 1, c >> 1), n++;
                    check_fill(1ull << p, run | other, c & 1, false), n++;
                }
            }
        }
    std::mt19937_64 rng(38);
    for (int i = 0; i < 200000; i++) {
        uint64_t g = rng();
        if (i & 1) g |= rng(); // long runs as well
        if (i % 7 == 0) g |= rng();
        const uint64_t s = rng() & rng() & rng() & g;
        check_fill(s, g, rng() & 1, rng() & 1), n++;
    }
    // the dilation step: every pixel of g with a neighbour in the state
    for (int i = 0; i < 20000; i++) {
        uint64_t w[3][3]; // rows above, at, below; words left, at, right
        for (auto &row : w)
            for (auto &v : row) v = rng() & rng();
        const uint64_t g = rng() | rng(), s = w[1][1] & g;
        for (int eight = 0; eight < 2; eight++) {
            const uint64_t got = canny::recon_step(s, g, w[1][0], w[1][2],
                                                   canny::recon_vertical(w[0][0], w[0][1], w[0][2], w[2][0], w[2][1], w[2][2], eight));
            uint64_t want = s;
            for (int x = 0; x < 64; x++) {
                // the pixel at column x + dx of a row: the word left of, at or right of the middle one
                auto at = [&](const uint64_t *row, int xx) {
                    return xx < 0 ? bit(row[0], 64 + xx) : (xx > 63 ? bit(row[2], xx - 64) : bit(row[1], xx));
                };
                const uint64_t mid[3] = {w[1][0], s, w[1][2]};
                int any = at(mid, x - 1) | at(mid, x + 1) | at(w[0], x) | at(w[2], x);
                if (eight) any |= at(w[0], x - 1) | at(w[0], x + 1) | at(w[2], x - 1) | at(w[2], x + 1);
                if (any && bit(g, x)) want |= 1ull << x;
            }
            if (got != want && fails++ < 10) printf("step %d: %016llx != %016llx\n", eight, (unsigned long long)got, (unsigned long long)want);
            n++;
        }
    }
    if (fails) {
        printf("%d of %ld cases failed\n", fails, n);
        return 1;
    }
    printf("recon words ok: %ld cases\n", n);
    return 0;
}
