// canny_binarize_host.cpp -- canny_hip_binarize and canny_hip_otsu_from_histogram: the binarization rule of include/canny_hip.h
//  in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against
// tests/binarize_rule.py, and what tests/cpp/test_binarize_host.cpp compiles under the host compiler's sanitizers.  The
// adaptive mean is computed with the rounded mean m = (2 S + A) / (2 A) and the comparison v > m - c, on purpose unlike the
// kernels of canny_binarize.hip (the division-free form); Otsu's score uses the compiler's 128-bit division where the kernel
// divides bit by bit.  The GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

const long long kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31, kMaxOtsu = 1ll << 26;

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// the smallest t with the largest floor(d^2 / (w0 w1)); N <= 2^26
int otsu(const unsigned long long *hist)
{
    unsigned long long N = 0, S = 0;
    for (int i = 0; i < 256; i++) N += hist[i], S += (unsigned long long)i * hist[i];
    unsigned long long w0 = 0, s0 = 0;
    unsigned __int128 best = 0;
    int best_t = 0;
    for (int t = 0; t < 256; t++) {
        w0 += hist[t], s0 += (unsigned long long)t * hist[t];
        const unsigned long long w1 = N - w0, s1 = S - s0;
        if (!w0 || !w1) continue; // score 0: never larger than the best
        const __int128 d = (__int128)w1 * s0 - (__int128)s1 * w0;
        const unsigned __int128 ad = (unsigned __int128)(d < 0 ? -d : d);
        const unsigned __int128 score = ad * ad / ((unsigned __int128)w0 * w1);
        if (score > best) best = score, best_t = t;
    }
    return best_t;
}

} // namespace

extern "C" {

int canny_hip_otsu_from_histogram(const unsigned long long *hist256, int *t)
{
    if (!hist256 || !t) return CANNY_HIP_ERR_INVALID;
    unsigned long long N = 0;
    for (int i = 0; i < 256; i++) {
        if (hist256[i] > (unsigned long long)kMaxOtsu) return CANNY_HIP_ERR_UNSUPPORTED;
        N += hist256[i];
    }
    if (N > (unsigned long long)kMaxOtsu) return CANNY_HIP_ERR_UNSUPPORTED;
    *t = otsu(hist256);
    return CANNY_HIP_OK;
}

int canny_hip_binarize(const unsigned char *imgs, int n_frames, int h, int w, int method, int thr_or_c, int kw, int kh,
                       int invert, unsigned char *out_bits, long long *counts, int *thresholds)
{
    if (!imgs || !out_bits || ((uintptr_t)counts & 7) || n_frames < 1 || h < 1 || w < 1 || invert < 0 || invert > 1)
        return CANNY_HIP_ERR_INVALID;
    if (method == CANNY_HIP_BIN_FIXED) {
        if (thr_or_c < -1 || thr_or_c > 255) return CANNY_HIP_ERR_INVALID;
    } else if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
        if (thr_or_c < -255 || thr_or_c > 255 || kw < 3 || kw > CANNY_HIP_BIN_MAX_EXTENT || kh < 3 ||
            kh > CANNY_HIP_BIN_MAX_EXTENT || !(kw & 1) || !(kh & 1))
            return CANNY_HIP_ERR_INVALID;
    } else if (method != CANNY_HIP_BIN_OTSU) {
        return CANNY_HIP_ERR_INVALID;
    }
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    if (method == CANNY_HIP_BIN_OTSU && (long long)h * w > kMaxOtsu) return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t rb = ((size_t)w + 7) / 8, plane = (size_t)h * w, in_bytes = plane * n_frames, out_bytes = rb * h * n_frames;
    const size_t cbytes = (size_t)n_frames * sizeof(long long), tbytes = (size_t)n_frames * sizeof(int);
    if (overlap(imgs, in_bytes, out_bits, out_bytes) || overlap(imgs, in_bytes, counts, cbytes) ||
        overlap(imgs, in_bytes, thresholds, tbytes) || overlap(out_bits, out_bytes, counts, cbytes) ||
        overlap(out_bits, out_bytes, thresholds, tbytes) || overlap(counts, cbytes, thresholds, tbytes))
        return CANNY_HIP_ERR_INVALID;

    std::vector<long long> col; // adaptive: the vertical sums of a row
    if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) col.resize((size_t)w);
    for (int f = 0; f < n_frames; f++) {
        const unsigned char *in = imgs + (size_t)f * plane;
        unsigned char *out = out_bits + (size_t)f * rb * h;
        int t = thr_or_c;
        if (method == CANNY_HIP_BIN_OTSU) {
            unsigned long long hist[256] = {0};
            for (size_t i = 0; i < plane; i++) hist[in[i]]++;
            t = otsu(hist);
        }
        long long set = 0;
        for (int y = 0; y < h; y++) {
            unsigned char *row = out + (size_t)y * rb;
            for (size_t b = 0; b < rb; b++) row[b] = 0; // pad bits are written 0
            if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
                for (int x = 0; x < w; x++) col[(size_t)x] = 0;
                for (int dy = -(kh / 2); dy <= kh / 2; dy++) {
                    const int yy = y + dy < 0 ? 0 : (y + dy >= h ? h - 1 : y + dy);
                    for (int x = 0; x < w; x++) col[(size_t)x] += in[(size_t)yy * w + x];
                }
            }
            for (int x = 0; x < w; x++) {
                const int v = in[(size_t)y * w + x];
                bool cond;
                if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
                    long long S = 0;
                    for (int dx = -(kw / 2); dx <= kw / 2; dx++) {
                        const int xx = x + dx < 0 ? 0 : (x + dx >= w ? w - 1 : x + dx);
                        S += col[(size_t)xx];
                    }
                    const long long A = (long long)kw * kh, m = (2 * S + A) / (2 * A); // the mean, halves up
                    cond = v > m - thr_or_c;
                } else {
                    cond = v > t;
                }
                if (cond != (invert != 0)) {
                    row[x >> 3] |= (unsigned char)(0x80u >> (x & 7));
                    set++;
                }
            }
        }
        if (counts) counts[f] = set;
        if (thresholds) thresholds[f] = t;
    }
    return CANNY_HIP_OK;
}

} // extern "C"
