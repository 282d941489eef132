// canny_fuse_host.cpp -- canny_hip_fuse_frames and canny_hip_change_mask: the temporal-fusion rules of include/canny_hip.h
//  in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against tests/fuse_rule.py,
// and what tests/cpp/test_fuse_host.cpp compiles under the host compiler's sanitizers.  The kernels of canny_fuse.hip are
// written separately from this file on purpose (a histogram here, sorting networks and a radix select there); the GPU tests
// compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

const long long kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31;

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// 0, or the status of a stack that the calls refuse
int stack_check(int n_frames, int h, int w)
{
    if (n_frames < 1 || h < 1 || w < 1) return CANNY_HIP_ERR_INVALID;
    if (h > kMaxDim || w > kMaxDim || (long long)h * w >= kMaxPlane || n_frames > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

bool bit(const unsigned char *row_bits, int x) { return (row_bits[x >> 3] >> (7 - (x & 7))) & 1; }

} // namespace

extern "C" int canny_hip_fuse_frames(const unsigned char *frames, const unsigned char *valid_bits, int n_frames, int h, int w,
                                     int group_len, int group_step, int op, int fill, int min_count, unsigned char *fused,
                                     unsigned char *count)
{
    if (!frames || !fused || n_frames < 1 || h < 1 || w < 1 || group_len < 1 || group_len > CANNY_HIP_FUSE_MAX_GROUP ||
        group_len > n_frames || group_step < 1 || op < CANNY_HIP_FUSE_MEAN || op > CANNY_HIP_FUSE_MAX || fill < 0 || fill > 255 ||
        min_count < 1 || min_count > 255)
        return CANNY_HIP_ERR_INVALID;
    const int rc = stack_check(n_frames, h, w);
    if (rc) return rc;
    const size_t plane = (size_t)h * w, row_bytes = ((size_t)w + 7) / 8, vplane = row_bytes * h;
    const int n_groups = (n_frames - group_len) / group_step + 1;
    const size_t in_bytes = plane * n_frames, vbytes = vplane * n_frames, out_bytes = plane * n_groups;
    if (overlap(frames, in_bytes, fused, out_bytes) || overlap(frames, in_bytes, count, out_bytes) ||
        overlap(valid_bits, vbytes, fused, out_bytes) || overlap(valid_bits, vbytes, count, out_bytes) ||
        overlap(fused, out_bytes, count, out_bytes))
        return CANNY_HIP_ERR_INVALID;

    for (int g = 0; g < n_groups; g++) {
        const size_t f0 = (size_t)g * group_step;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int hist[256];
                std::memset(hist, 0, sizeof hist);
                int c = 0;
                long long s = 0;
                for (int k = 0; k < group_len; k++) {
                    const size_t f = f0 + k;
                    if (valid_bits && !bit(valid_bits + f * vplane + row_bytes * y, x)) continue;
                    const int v = frames[f * plane + (size_t)y * w + x];
                    hist[v]++, c++, s += v;
                }
                int px = fill;
                if (c >= min_count) { // min_count >= 1: c > 0
                    if (op == CANNY_HIP_FUSE_MEAN) {
                        px = (int)((2 * s + c) / (2 * c));
                    } else {
                        // the value of rank r among the sorted valid samples
                        const int r = op == CANNY_HIP_FUSE_MEDIAN ? (c - 1) >> 1 : (op == CANNY_HIP_FUSE_MIN ? 0 : c - 1);
                        int seen = 0;
                        for (px = 0; px < 256; px++) {
                            seen += hist[px];
                            if (seen > r) break;
                        }
                    }
                }
                const size_t at = (size_t)g * plane + (size_t)y * w + x;
                fused[at] = (unsigned char)px;
                if (count) count[at] = (unsigned char)c;
            }
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_change_mask(const unsigned char *frames, const unsigned char *valid_bits, int n_frames, int h, int w,
                                     const unsigned char *background, const unsigned char *bg_count,
                                     int frames_per_background, int thr, int min_count, unsigned char *mask_bits,
                                     long long *changed)
{
    if (!frames || !background || !mask_bits || n_frames < 1 || h < 1 || w < 1 || frames_per_background < 1 || thr < 0 ||
        thr > 255 || min_count < 1 || min_count > 255 || ((uintptr_t)changed & 7))
        return CANNY_HIP_ERR_INVALID;
    const int rc = stack_check(n_frames, h, w);
    if (rc) return rc;
    const size_t plane = (size_t)h * w, row_bytes = ((size_t)w + 7) / 8, vplane = row_bytes * h;
    const size_t n_bg = ((size_t)n_frames + frames_per_background - 1) / frames_per_background;
    const size_t in_bytes = plane * n_frames, vbytes = vplane * n_frames, bg_bytes = plane * n_bg;
    const size_t ch_bytes = (size_t)n_frames * sizeof(long long);
    if (overlap(frames, in_bytes, mask_bits, vbytes) || overlap(valid_bits, vbytes, mask_bits, vbytes) ||
        overlap(background, bg_bytes, mask_bits, vbytes) || overlap(bg_count, bg_bytes, mask_bits, vbytes) ||
        overlap(frames, in_bytes, changed, ch_bytes) || overlap(valid_bits, vbytes, changed, ch_bytes) ||
        overlap(background, bg_bytes, changed, ch_bytes) || overlap(bg_count, bg_bytes, changed, ch_bytes) ||
        overlap(mask_bits, vbytes, changed, ch_bytes))
        return CANNY_HIP_ERR_INVALID;

    for (int f = 0; f < n_frames; f++) {
        const size_t b = (size_t)(f / frames_per_background) * plane;
        unsigned char *m = mask_bits + vplane * f;
        std::memset(m, 0, vplane);
        long long n = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t at = (size_t)y * w + x;
                if (valid_bits && !bit(valid_bits + vplane * f + row_bytes * y, x)) continue;
                if (bg_count && bg_count[b + at] < min_count) continue;
                const int d = (int)frames[plane * f + at] - (int)background[b + at];
                if ((d < 0 ? -d : d) > thr) m[row_bytes * y + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7)), n++;
            }
        if (changed) changed[f] = n;
    }
    return CANNY_HIP_OK;
}
