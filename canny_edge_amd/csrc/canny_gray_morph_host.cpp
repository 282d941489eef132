// canny_gray_morph_host.cpp -- canny_hip_gray_morph: the grey-level morphology and median rule of include/canny_hip.h
//  in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against
// tests/gray_morph_rule.py, and what tests/cpp/test_gray_morph_host.cpp compiles under the host compiler's sanitizers.  It
// works pixel by pixel and offset by offset, and sorts the median's window, on purpose unlike the kernels of
// canny_gray_morph.hip (words of four pixels, runs by doubling, selection networks); the GPU tests compare both with the
// Python rule.
#include "canny_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

const long long kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31;

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// the binary morphology's checks of an element
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

enum { ERODE_STEP = 0, DILATE_STEP = 1, MEDIAN_STEP = 2 };

struct Border {
    int mode, value;
};

// what the pixel (xx, yy) of `in` reads as in a step of `kind`
int read(const std::vector<unsigned char> &in, int h, int w, int xx, int yy, int kind, Border b)
{
    if (b.mode == CANNY_HIP_GRAY_BORDER_REPLICATE) {
        xx = std::min(std::max(xx, 0), w - 1), yy = std::min(std::max(yy, 0), h - 1);
    } else if (xx < 0 || xx >= w || yy < 0 || yy >= h) {
        return b.mode == CANNY_HIP_GRAY_BORDER_CONSTANT ? b.value : (kind == ERODE_STEP ? 255 : 0);
    }
    return in[(size_t)yy * w + xx];
}

void step(const std::vector<unsigned char> &in, std::vector<unsigned char> &out, int h, int w, const std::vector<Offset> &el,
          int kind, Border b)
{
    std::vector<int> win(el.size());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int v;
            if (kind == MEDIAN_STEP) {
                for (size_t i = 0; i < el.size(); i++) win[i] = read(in, h, w, x + el[i].dx, y + el[i].dy, kind, b);
                std::nth_element(win.begin(), win.begin() + (win.size() - 1) / 2, win.end());
                v = win[(win.size() - 1) / 2];
            } else if (kind == ERODE_STEP) {
                v = 255;
                for (const Offset &o : el) v = std::min(v, read(in, h, w, x + o.dx, y + o.dy, kind, b));
            } else {
                v = 0;
                for (const Offset &o : el) v = std::max(v, read(in, h, w, x - o.dx, y - o.dy, kind, b));
            }
            out[(size_t)y * w + x] = (unsigned char)v;
        }
}

// `iterations` steps of one primitive, in place (through tmp)
void chain(std::vector<unsigned char> &a, std::vector<unsigned char> &tmp, int h, int w, const std::vector<Offset> &el, int kind,
           Border b, int iterations)
{
    for (int i = 0; i < iterations; i++) {
        step(a, tmp, h, w, el, kind, b);
        a.swap(tmp);
    }
}

unsigned char sat_sub(int a, int b) { return (unsigned char)(a > b ? a - b : 0); }

} // namespace

extern "C" int canny_hip_gray_morph(const unsigned char *imgs, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                                    int kh, int border_mode, int border_value, int iterations, unsigned char *out)
{
    if (!imgs || !out || n_frames < 1 || h < 1 || w < 1 || op < CANNY_HIP_GRAY_ERODE || op > CANNY_HIP_GRAY_MEDIAN ||
        border_mode < CANNY_HIP_GRAY_BORDER_NEUTRAL || border_mode > CANNY_HIP_GRAY_BORDER_CONSTANT ||
        (border_mode == CANNY_HIP_GRAY_BORDER_CONSTANT && (border_value < 0 || border_value > 255)) || iterations < 1 ||
        iterations > CANNY_HIP_MORPH_MAX_ITERATIONS || !element_ok(rows, kw, kh))
        return CANNY_HIP_ERR_INVALID;
    if (op == CANNY_HIP_GRAY_MEDIAN) {
        if (kw != kh || (kw != 3 && kw != 5) || border_mode == CANNY_HIP_GRAY_BORDER_NEUTRAL) return CANNY_HIP_ERR_INVALID;
        for (int j = 0; j < kh; j++)
            if (rows[j] != (1u << kw) - 1u) return CANNY_HIP_ERR_INVALID;
    }
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t px = (size_t)h * w, bytes = px * n_frames;
    if (overlap(imgs, bytes, out, bytes)) return CANNY_HIP_ERR_INVALID;
    std::vector<Offset> el;
    for (int j = 0; j < kh; j++)
        for (int i = 0; i < kw; i++)
            if ((rows[j] >> i) & 1u) el.push_back(Offset{i - kw / 2, j - kh / 2});
    const Border b{border_mode, border_value};
    std::vector<unsigned char> in(px), a(px), c(px), tmp(px);
    for (int f = 0; f < n_frames; f++) {
        in.assign(imgs + (size_t)f * px, imgs + (size_t)(f + 1) * px);
        a = in;
        switch (op) {
        case CANNY_HIP_GRAY_ERODE: chain(a, tmp, h, w, el, ERODE_STEP, b, iterations); break;
        case CANNY_HIP_GRAY_DILATE: chain(a, tmp, h, w, el, DILATE_STEP, b, iterations); break;
        case CANNY_HIP_GRAY_MEDIAN: chain(a, tmp, h, w, el, MEDIAN_STEP, b, iterations); break;
        case CANNY_HIP_GRAY_OPEN:
        case CANNY_HIP_GRAY_TOPHAT:
            chain(a, tmp, h, w, el, ERODE_STEP, b, iterations);
            chain(a, tmp, h, w, el, DILATE_STEP, b, iterations);
            if (op == CANNY_HIP_GRAY_TOPHAT)
                for (size_t i = 0; i < px; i++) a[i] = sat_sub(in[i], a[i]);
            break;
        case CANNY_HIP_GRAY_CLOSE:
        case CANNY_HIP_GRAY_BLACKHAT:
            chain(a, tmp, h, w, el, DILATE_STEP, b, iterations);
            chain(a, tmp, h, w, el, ERODE_STEP, b, iterations);
            if (op == CANNY_HIP_GRAY_BLACKHAT)
                for (size_t i = 0; i < px; i++) a[i] = sat_sub(a[i], in[i]);
            break;
        default: // GRADIENT
            c = in;
            chain(a, tmp, h, w, el, DILATE_STEP, b, iterations);
            chain(c, tmp, h, w, el, ERODE_STEP, b, iterations);
            for (size_t i = 0; i < px; i++) a[i] = sat_sub(a[i], c[i]);
            break;
        }
        std::copy(a.begin(), a.end(), out + (size_t)f * px);
    }
    return CANNY_HIP_OK;
}
