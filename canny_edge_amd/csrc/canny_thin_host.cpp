// canny_thin_host.cpp -- canny_hip_thin_bits: the thinning rule of include/canny_hip.h in plain C++ on
// host buffers.  No device, no HIP: what the CPU tests pin against tests/thin_rule.py, and what tests/cpp/test_thin_host.cpp
// compiles under the host compiler's sanitizers.  It works pixel by pixel on an unpacked frame, on purpose unlike the kernels
// of canny_thin.hip (whole words, bit-sliced counts); the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const long long kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31;

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// Whether sub-iteration `sub` deletes the set pixel whose neighbours are p[2] .. p[9].
bool deletes(int method, int sub, const int *p)
{
    if (method == CANNY_HIP_THIN_ZHANGSUEN) {
        int b = 0, a = 0;
        for (int i = 2; i <= 9; i++) {
            b += p[i];
            a += !p[i] && p[i == 9 ? 2 : i + 1];
        }
        if (b < 2 || b > 6 || a != 1) return false;
        return sub == 0 ? !(p[2] && p[4] && p[6]) && !(p[4] && p[6] && p[8]) : !(p[2] && p[4] && p[8]) && !(p[2] && p[6] && p[8]);
    }
    const int c = (!p[2] && (p[3] || p[4])) + (!p[4] && (p[5] || p[6])) + (!p[6] && (p[7] || p[8])) + (!p[8] && (p[9] || p[2]));
    const int n1 = (p[9] || p[2]) + (p[3] || p[4]) + (p[5] || p[6]) + (p[7] || p[8]);
    const int n2 = (p[2] || p[3]) + (p[4] || p[5]) + (p[6] || p[7]) + (p[8] || p[9]);
    const int n = n1 < n2 ? n1 : n2;
    const bool m = sub == 0 ? (p[6] || p[7] || !p[9]) && p[8] : (p[2] || p[3] || !p[5]) && p[4];
    return c == 1 && n >= 2 && n <= 3 && !m;
}

// One sub-iteration of the whole frame, a -> a through the list of deleted pixels; the number of deletions.
long long sub_iteration(std::vector<unsigned char> &a, std::vector<size_t> &gone, int h, int w, int method, int sub)
{
    static const int dy[10] = {0, 0, -1, -1, 0, 1, 1, 1, 0, -1}, dx[10] = {0, 0, 0, 1, 1, 1, 0, -1, -1, -1};
    gone.clear();
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (!a[(size_t)y * w + x]) continue;
            int p[10] = {0};
            for (int i = 2; i <= 9; i++) {
                const int yy = y + dy[i], xx = x + dx[i];
                p[i] = (yy < 0 || yy >= h || xx < 0 || xx >= w) ? 0 : a[(size_t)yy * w + xx];
            }
            if (deletes(method, sub, p)) gone.push_back((size_t)y * w + x);
        }
    for (size_t i : gone) a[i] = 0;
    return (long long)gone.size();
}

} // namespace

extern "C" int canny_hip_thin_bits(const unsigned char *bits, int n_frames, int h, int w, int method, int max_iterations,
                                   unsigned char *out_bits, long long *info)
{
    if (!bits || !out_bits || n_frames < 1 || h < 1 || w < 1 || method < CANNY_HIP_THIN_ZHANGSUEN ||
        method > CANNY_HIP_THIN_GUOHALL || max_iterations < 0 || max_iterations > CANNY_HIP_THIN_MAX_ITERATIONS ||
        ((uintptr_t)info & 7))
        return CANNY_HIP_ERR_INVALID;
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t rb = ((size_t)w + 7) / 8, fbytes = rb * h, bytes = fbytes * n_frames;
    const size_t ibytes = (size_t)n_frames * CANNY_HIP_THIN_INFO * sizeof(long long);
    if (overlap(bits, bytes, out_bits, bytes) || overlap(bits, bytes, info, ibytes) || overlap(out_bits, bytes, info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    std::vector<unsigned char> a((size_t)h * w);
    std::vector<size_t> gone;
    for (int f = 0; f < n_frames; f++) {
        const unsigned char *src = bits + (size_t)f * fbytes;
        long long in_set = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                in_set += a[(size_t)y * w + x] = (src[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
        long long iterations = 0, converged = 0;
        while (max_iterations == 0 || iterations < max_iterations) {
            long long n = sub_iteration(a, gone, h, w, method, 0);
            n += sub_iteration(a, gone, h, w, method, 1);
            if (!n) {
                converged = 1;
                break;
            }
            iterations++;
        }
        unsigned char *dst = out_bits + (size_t)f * fbytes;
        std::memset(dst, 0, fbytes);
        long long n = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (a[(size_t)y * w + x]) dst[(size_t)y * rb + (x >> 3)] |= (unsigned char)(0x80u >> (x & 7)), n++;
        if (info) {
            long long *r = info + (size_t)f * CANNY_HIP_THIN_INFO;
            r[0] = n, r[1] = iterations, r[2] = in_set - n, r[3] = converged;
        }
    }
    return CANNY_HIP_OK;
}
