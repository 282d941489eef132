// Stand-alone check of csrc/canny_thin_words.h (own main; built by tests/test_thin_rule.py with the host compiler): the
// bit-sliced sub-iteration the kernels run on 64 pixels at once against the per-pixel rule written here straight from the
// header's definitions -- all 512 neighbourhoods at every bit position, both methods, both sub-iterations, then random words,
// whose 64 bit positions are 64 independent neighbourhoods.
#include "canny_thin_words.h"

#include <cstdint>
#include <cstdio>

// p[1] .. p[9] = P1 .. P9
static bool deletes(int method, int sub, const int *p)
{
    if (!p[1]) return false;
    if (method == 0) {
        int b = 0, a = 0;
        for (int i = 2; i <= 9; i++) b += p[i], a += !p[i] && p[i == 9 ? 2 : i + 1];
        const bool guard = sub == 0 ? (p[2] && p[4] && p[6]) || (p[4] && p[6] && p[8]) : (p[2] && p[4] && p[8]) || (p[2] && p[6] && p[8]);
        return b >= 2 && b <= 6 && a == 1 && !guard;
    }
    const int c = (!p[2] && (p[3] || p[4])) + (!p[4] && (p[5] || p[6])) + (!p[6] && (p[7] || p[8])) + (!p[8] && (p[9] || p[2]));
    const int n1 = (p[9] || p[2]) + (p[3] || p[4]) + (p[5] || p[6]) + (p[7] || p[8]);
    const int n2 = (p[2] || p[3]) + (p[4] || p[5]) + (p[6] || p[7]) + (p[8] || p[9]);
    const int n = n1 < n2 ? n1 : n2;
    const bool m = sub == 0 ? (p[6] || p[7] || !p[9]) && p[8] : (p[2] || p[3] || !p[5]) && p[4];
    return c == 1 && n >= 2 && n <= 3 && !m;
}

static uint64_t sliced(int method, int sub, const uint64_t *w)
{
    return method == 0 ? canny::thin_deletions<0>(w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], sub)
                       : canny::thin_deletions<1>(w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], sub);
}

static int check(const uint64_t *w)
{
    int bad = 0;
    for (int method = 0; method < 2; method++)
        for (int sub = 0; sub < 2; sub++) {
            const uint64_t got = sliced(method, sub, w);
            for (int bit = 0; bit < 64; bit++) {
                int p[10] = {0};
                for (int i = 1; i <= 9; i++) p[i] = (int)((w[i] >> bit) & 1);
                bad += (int)((got >> bit) & 1) != (int)deletes(method, sub, p);
            }
        }
    return bad;
}

int main()
{
    long long bad = 0, cases = 0;
    for (int cfg = 0; cfg < 512; cfg++)
        for (int bit = 0; bit < 64; bit++) { // the neighbourhood at one bit position, its complement at all the others
            uint64_t w[10] = {0};
            for (int i = 1; i <= 9; i++) w[i] = ((cfg >> (i - 1)) & 1) ? 1ull << bit : ~(1ull << bit);
            bad += check(w), cases++;
        }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 20000; k++) {
        uint64_t w[10] = {0};
        for (int i = 1; i <= 9; i++) {
            s ^= s << 13, s ^= s >> 7, s ^= s << 17;
            w[i] = k % 3 == 0 ? s : (k % 3 == 1 ? s | (s << 1) | (s >> 3) : s & (s >> 2)); // even, dense and sparse words
        }
        bad += check(w), cases++;
    }
    if (bad) {
        std::fprintf(stderr, "%lld bits differ from the per-pixel rule\n", bad);
        return 1;
    }
    std::printf("thin words ok (%lld cases)\n", cases);
    return 0;
}
