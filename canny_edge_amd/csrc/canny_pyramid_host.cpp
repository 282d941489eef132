// canny_pyramid_host.cpp -- canny_hip_pyramid_layout, canny_hip_pyramid and canny_hip_pyr_up: the image pyramid rule of
// include/canny_hip.h in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against
// tests/pyramid_rule.py, and what tests/cpp/test_pyramid_host.cpp compiles under the host compiler's sanitizers.  It works
// pixel by pixel with all 25 (pyrDown) or up to 9 (pyrUp) taps and every index folded, on purpose unlike the kernels of
// canny_pyramid.hip (separated, packed 16-bit halves, LDS); the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>

namespace {

const long long kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31;
const int kTaps[5] = {1, 4, 6, 4, 1};

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// sizes first (INVALID), then the limits (UNSUPPORTED)
int check_planes(int n_frames, int h, int w)
{
    if (n_frames < 1 || h < 1 || w < 1) return CANNY_HIP_ERR_INVALID;
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// reflect-101: cv::BORDER_DEFAULT, scipy mode='mirror'
int fold(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// the smallest L with 2^L >= m
int ceil_log2(int m)
{
    int l = 0;
    while ((1ll << l) < m) l++;
    return l;
}

void down_plane(const unsigned char *in, int h, int w, unsigned char *out)
{
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            unsigned s = 0;
            for (int j = 0; j < 5; j++)
                for (int i = 0; i < 5; i++)
                    s += (unsigned)(kTaps[j] * kTaps[i]) * in[(size_t)fold(2 * y + j - 2, h) * w + fold(2 * x + i - 2, w)];
            out[(size_t)y * ow + x] = (unsigned char)((s + 128) >> 8);
        }
}

// the up to three source indices and weights of output index o along an axis of n source samples
struct UpTaps {
    int n, at[3], wt[3];
};
UpTaps up_taps(int o, int n)
{
    const int x = o >> 1, before = x > 0 ? x - 1 : (n > 1 ? 1 : 0), after = x + 1 < n ? x + 1 : n - 1;
    if (o & 1) return UpTaps{2, {x, after, 0}, {4, 4, 0}};
    return UpTaps{3, {before, x, after}, {1, 6, 1}};
}

} // namespace

extern "C" int canny_hip_pyramid_layout(int n_frames, int h, int w, int levels, long long *info, long long *total_bytes)
{
    if (!info || !total_bytes) return CANNY_HIP_ERR_INVALID;
    const int rc = check_planes(n_frames, h, w);
    if (rc == CANNY_HIP_ERR_INVALID) return rc;
    if (levels < 1 || levels > CANNY_HIP_PYR_MAX_LEVELS) return CANNY_HIP_ERR_INVALID;
    if (rc) return rc;
    if (levels > ceil_log2(h > w ? h : w)) return CANNY_HIP_ERR_INVALID;
    long long off = 0;
    for (int l = 0; l < levels; l++) {
        h = (h + 1) / 2, w = (w + 1) / 2;
        const long long bytes = (long long)n_frames * h * w;
        info[4 * l + 0] = h, info[4 * l + 1] = w, info[4 * l + 2] = off, info[4 * l + 3] = bytes;
        *total_bytes = off + bytes;
        off = (off + bytes + 255) & ~255ll;
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_pyramid(const unsigned char *imgs, int n_frames, int h, int w, int levels, unsigned char *out)
{
    if (!imgs || !out) return CANNY_HIP_ERR_INVALID;
    long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = 0;
    const int rc = canny_hip_pyramid_layout(n_frames, h, w, levels, info, &total);
    if (rc) return rc;
    if (overlap(imgs, (size_t)n_frames * h * w, out, (size_t)total)) return CANNY_HIP_ERR_INVALID;
    const unsigned char *src = imgs;
    for (int l = 0; l < levels; l++) {
        unsigned char *dst = out + info[4 * l + 2];
        const size_t in_px = (size_t)h * w, out_px = (size_t)info[4 * l] * (size_t)info[4 * l + 1];
        for (int f = 0; f < n_frames; f++) down_plane(src + f * in_px, h, w, dst + f * out_px);
        src = dst, h = (int)info[4 * l], w = (int)info[4 * l + 1];
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_pyr_up(const unsigned char *imgs, int n_frames, int h, int w, int oh, int ow, unsigned char *out)
{
    if (!imgs || !out) return CANNY_HIP_ERR_INVALID;
    int rc = check_planes(n_frames, h, w);
    if (rc == CANNY_HIP_ERR_INVALID) return rc;
    if ((oh != 2 * h - 1 && oh != 2 * h) || (ow != 2 * w - 1 && ow != 2 * w) || oh < 1 || ow < 1) return CANNY_HIP_ERR_INVALID;
    if (rc || (rc = check_planes(n_frames, oh, ow))) return rc;
    const size_t in_px = (size_t)h * w, out_px = (size_t)oh * ow;
    if (overlap(imgs, in_px * n_frames, out, out_px * n_frames)) return CANNY_HIP_ERR_INVALID;
    for (int f = 0; f < n_frames; f++) {
        const unsigned char *in = imgs + f * in_px;
        unsigned char *o = out + f * out_px;
        for (int y = 0; y < oh; y++) {
            const UpTaps ty = up_taps(y, h);
            for (int x = 0; x < ow; x++) {
                const UpTaps tx = up_taps(x, w);
                unsigned s = 0;
                for (int j = 0; j < ty.n; j++)
                    for (int i = 0; i < tx.n; i++) s += (unsigned)(ty.wt[j] * tx.wt[i]) * in[(size_t)ty.at[j] * w + tx.at[i]];
                o[(size_t)y * ow + x] = (unsigned char)((s + 32) >> 6);
            }
        }
    }
    return CANNY_HIP_OK;
}
