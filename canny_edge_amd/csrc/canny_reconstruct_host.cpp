// canny_reconstruct_host.cpp -- canny_hip_reconstruct_bits: the reconstruction rule of include/canny_hip.h (DESIGN.md section
// 38) in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against tests/reconstruct_rule.py, and what
// tests/cpp/test_reconstruct_host.cpp compiles under the host compiler's sanitizers.  It is a stack flood pixel by pixel on an
// unpacked frame, on purpose unlike the kernels of canny_reconstruct.hip (whole words, rounds to a fixed point); the GPU tests
// compare both with the Python rule.
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

void unpack(const unsigned char *src, int h, int w, size_t rb, std::vector<unsigned char> &px)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) px[(size_t)y * w + x] = (src[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
}

// R_c(start, g): reached[] = the pixels of g joined to a pixel of start & g by a c-connected path inside g; the pixels of
// start & g are counted into *n_start.
void flood(const std::vector<unsigned char> &start, const std::vector<unsigned char> &g, int h, int w, int c,
           std::vector<unsigned char> &reached, std::vector<size_t> &stack, long long *n_start)
{
    static const int dy[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dx[8] = {0, 0, -1, 1, -1, 1, -1, 1};
    std::fill(reached.begin(), reached.end(), 0);
    stack.clear();
    *n_start = 0;
    for (size_t i = 0; i < start.size(); i++)
        if (start[i] && g[i]) reached[i] = 1, stack.push_back(i), ++*n_start;
    while (!stack.empty()) {
        const size_t i = stack.back();
        stack.pop_back();
        const int y = (int)(i / (size_t)w), x = (int)(i % (size_t)w);
        for (int d = 0; d < c; d++) {
            const int yy = y + dy[d], xx = x + dx[d];
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const size_t j = (size_t)yy * w + xx;
            if (g[j] && !reached[j]) reached[j] = 1, stack.push_back(j);
        }
    }
}

} // namespace

extern "C" int canny_hip_reconstruct_bits(const unsigned char *marker, const unsigned char *mask, int n_frames, int h, int w,
                                          int op, int connectivity, unsigned char *out, long long *info)
{
    if (!mask || !out || n_frames < 1 || h < 1 || w < 1 || op < CANNY_HIP_RECON_SEEDED || op > CANNY_HIP_RECON_CLEAR_BORDER ||
        (connectivity != 4 && connectivity != 8) || (op == CANNY_HIP_RECON_SEEDED) != (marker != nullptr) ||
        ((uintptr_t)info & 7))
        return CANNY_HIP_ERR_INVALID;
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t rb = ((size_t)w + 7) / 8, fbytes = rb * h, bytes = fbytes * n_frames;
    const size_t ibytes = (size_t)n_frames * CANNY_HIP_RECON_INFO * sizeof(long long);
    if (overlap(marker, bytes, out, bytes) || overlap(mask, bytes, out, bytes) || overlap(info, ibytes, out, bytes) ||
        overlap(marker, bytes, info, ibytes) || overlap(mask, bytes, info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    const size_t n = (size_t)h * w;
    std::vector<unsigned char> m(n), start(n), g(n), reached(n);
    std::vector<size_t> stack;
    for (int f = 0; f < n_frames; f++) {
        unpack(mask + (size_t)f * fbytes, h, w, rb, m);
        long long in_mask = 0;
        for (size_t i = 0; i < n; i++) in_mask += m[i];
        if (op == CANNY_HIP_RECON_SEEDED) {
            unpack(marker + (size_t)f * fbytes, h, w, rb, start);
        } else {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) start[(size_t)y * w + x] = y == 0 || y == h - 1 || x == 0 || x == w - 1;
        }
        // what conducts: the mask, or for FILL_HOLES the background, which takes the dual connectivity
        for (size_t i = 0; i < n; i++) g[i] = op == CANNY_HIP_RECON_FILL_HOLES ? !m[i] : m[i];
        long long n_start = 0;
        flood(start, g, h, w, op == CANNY_HIP_RECON_FILL_HOLES ? 12 - connectivity : connectivity, reached, stack, &n_start);
        unsigned char *dst = out + (size_t)f * fbytes;
        std::memset(dst, 0, fbytes);
        long long set = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const bool v = op == CANNY_HIP_RECON_SEEDED ? reached[i] : (op == CANNY_HIP_RECON_FILL_HOLES ? !reached[i] : m[i] && !reached[i]);
                if (v) dst[(size_t)y * rb + (x >> 3)] |= (unsigned char)(0x80u >> (x & 7)), set++;
            }
        if (info) {
            long long *r = info + (size_t)f * CANNY_HIP_RECON_INFO;
            r[0] = set, r[1] = in_mask, r[2] = n_start;
        }
    }
    return CANNY_HIP_OK;
}
