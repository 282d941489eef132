// canny_morph_host.cpp -- canny_hip_morph_bits and canny_hip_morph_element: the binary-morphology rule of include/canny_hip.h
//  in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against tests/morph_rule.py,
// and what tests/cpp/test_morph_host.cpp compiles under the host compiler's sanitizers.  It works pixel by pixel on an
// unpacked frame, on purpose unlike the kernels of canny_morph.hip (whole words, runs by doubling); the GPU tests compare
// both with the Python rule.
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

bool element_ok(const unsigned *rows, int kw, int kh)
{
    if (!rows || kw < 1 || kw > CANNY_HIP_MORPH_MAX_EXTENT || kh < 1 || kh > CANNY_HIP_MORPH_MAX_EXTENT || !(kw & 1) || !(kh & 1))
        return false;
    unsigned any = 0;
    for (int j = 0; j < kh; j++) {
        if (rows[j] >> kw) return false; // kw <= 31: the shift is defined
        any |= rows[j];
    }
    return any != 0;
}

struct Offset {
    int dx, dy;
};

// One primitive step on an unpacked frame: out(p) = AND over b of in(p + b) (erode) or OR over b of in(p - b) (dilate); a
// pixel outside the frame reads as `outside`.
void step(const std::vector<unsigned char> &in, std::vector<unsigned char> &out, int h, int w, const std::vector<Offset> &el,
          bool erode, int outside)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int v = erode ? 1 : 0;
            for (const Offset &b : el) {
                const int xx = erode ? x + b.dx : x - b.dx, yy = erode ? y + b.dy : y - b.dy;
                const int s = (xx < 0 || xx >= w || yy < 0 || yy >= h) ? outside : in[(size_t)yy * w + xx];
                if (erode ? !s : s) {
                    v = s;
                    break;
                }
            }
            out[(size_t)y * w + x] = (unsigned char)v;
        }
}

// `iterations` steps of one primitive, in place (through tmp)
void chain(std::vector<unsigned char> &a, std::vector<unsigned char> &tmp, int h, int w, const std::vector<Offset> &el,
           bool erode, int border, int iterations)
{
    const int outside = border == CANNY_HIP_MORPH_BORDER_NEUTRAL ? (erode ? 1 : 0) : border;
    for (int i = 0; i < iterations; i++) {
        step(a, tmp, h, w, el, erode, outside);
        a.swap(tmp);
    }
}

} // namespace

extern "C" int canny_hip_morph_element(int shape, int kw, int kh, unsigned *rows)
{
    if (!rows || kw < 1 || kw > CANNY_HIP_MORPH_MAX_EXTENT || kh < 1 || kh > CANNY_HIP_MORPH_MAX_EXTENT || !(kw & 1) ||
        !(kh & 1) || shape < CANNY_HIP_MORPH_RECT || shape > CANNY_HIP_MORPH_ELLIPSE)
        return CANNY_HIP_ERR_INVALID;
    const int rx = kw / 2, ry = kh / 2;
    const unsigned full = (1u << kw) - 1u;
    for (int j = 0; j < kh; j++) {
        unsigned m = 0;
        if (shape == CANNY_HIP_MORPH_RECT || (shape == CANNY_HIP_MORPH_ELLIPSE && (!rx || !ry))) {
            m = full;
        } else if (shape == CANNY_HIP_MORPH_CROSS) {
            m = j == ry ? full : 1u << rx;
        } else {
            const long long dy = j - ry;
            for (int i = 0; i < kw; i++) {
                const long long dx = i - rx;
                if (dx * dx * ry * ry + dy * dy * rx * rx <= (long long)rx * rx * ry * ry) m |= 1u << i;
            }
        }
        rows[j] = m;
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_morph_bits(const unsigned char *bits, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                                    int kh, int border, int iterations, unsigned char *out_bits, long long *counts)
{
    if (!bits || !out_bits || n_frames < 1 || h < 1 || w < 1 || op < CANNY_HIP_MORPH_ERODE || op > CANNY_HIP_MORPH_BLACKHAT ||
        border < CANNY_HIP_MORPH_BORDER_ZERO || border > CANNY_HIP_MORPH_BORDER_NEUTRAL || iterations < 1 ||
        iterations > CANNY_HIP_MORPH_MAX_ITERATIONS || !element_ok(rows, kw, kh) || ((uintptr_t)counts & 7))
        return CANNY_HIP_ERR_INVALID;
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t rb = ((size_t)w + 7) / 8, fbytes = rb * h, bytes = fbytes * n_frames, cbytes = (size_t)n_frames * sizeof(long long);
    if (overlap(bits, bytes, out_bits, bytes) || overlap(bits, bytes, counts, cbytes) || overlap(out_bits, bytes, counts, cbytes))
        return CANNY_HIP_ERR_INVALID;
    std::vector<Offset> el;
    for (int j = 0; j < kh; j++)
        for (int i = 0; i < kw; i++)
            if ((rows[j] >> i) & 1u) el.push_back(Offset{i - kw / 2, j - kh / 2});
    const size_t px = (size_t)h * w;
    std::vector<unsigned char> in(px), a(px), b(px), tmp(px);
    for (int f = 0; f < n_frames; f++) {
        const unsigned char *src = bits + (size_t)f * fbytes;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) in[(size_t)y * w + x] = (src[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1;
        a = in;
        switch (op) {
        case CANNY_HIP_MORPH_ERODE: chain(a, tmp, h, w, el, true, border, iterations); break;
        case CANNY_HIP_MORPH_DILATE: chain(a, tmp, h, w, el, false, border, iterations); break;
        case CANNY_HIP_MORPH_OPEN:
        case CANNY_HIP_MORPH_TOPHAT:
            chain(a, tmp, h, w, el, true, border, iterations);
            chain(a, tmp, h, w, el, false, border, iterations);
            if (op == CANNY_HIP_MORPH_TOPHAT)
                for (size_t i = 0; i < px; i++) a[i] = in[i] & (a[i] ^ 1);
            break;
        case CANNY_HIP_MORPH_CLOSE:
        case CANNY_HIP_MORPH_BLACKHAT:
            chain(a, tmp, h, w, el, false, border, iterations);
            chain(a, tmp, h, w, el, true, border, iterations);
            if (op == CANNY_HIP_MORPH_BLACKHAT)
                for (size_t i = 0; i < px; i++) a[i] = a[i] & (in[i] ^ 1);
            break;
        default: // GRADIENT
            b = in;
            chain(a, tmp, h, w, el, false, border, iterations);
            chain(b, tmp, h, w, el, true, border, iterations);
            for (size_t i = 0; i < px; i++) a[i] = a[i] & (b[i] ^ 1);
            break;
        }
        unsigned char *dst = out_bits + (size_t)f * fbytes;
        std::memset(dst, 0, fbytes);
        long long n = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (a[(size_t)y * w + x]) dst[(size_t)y * rb + (x >> 3)] |= (unsigned char)(0x80u >> (x & 7)), n++;
        if (counts) counts[f] = n;
    }
    return CANNY_HIP_OK;
}
