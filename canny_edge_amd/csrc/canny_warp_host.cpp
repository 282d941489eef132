// canny_warp_host.cpp -- canny_hip_compose_motion and canny_hip_warp_frames: the frame-alignment rules of include/canny_hip.h
//  in plain C++ on host buffers.  No device, no HIP: what the CPU tests pin against tests/warp_rule.py,
// and what tests/cpp/test_warp_host.cpp compiles under the host compiler's sanitizers.  The kernels of canny_warp.hip are
// written separately from this file on purpose; the GPU tests compare both with the Python rule.
#include "canny_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

typedef long long i64;

const i64 kLimA = 1ll << 24, kLimT = 1ll << 36;
const i64 kMaxDim = 32768, kMaxFrames = 65535, kMaxPlane = 1ll << 31;

bool within(i64 v, i64 lim) { return v >= -lim && v <= lim; }

// c: a11, a12, tx, a21, a22, ty
bool within_limits(const i64 *c)
{
    return within(c[0], kLimA) && within(c[1], kLimA) && within(c[3], kLimA) && within(c[4], kLimA) && within(c[2], kLimT) &&
           within(c[5], kLimT);
}

// floor(v / 65536) on a signed value without shifting a negative one
i64 fl16(i64 v) { return v >= 0 ? v / 65536 : -((-v + 65535) / 65536); }
i64 fl(i64 v, int bits) { return v >= 0 ? v >> bits : -((-v + ((1ll << bits) - 1)) >> bits); }

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

} // namespace

extern "C" int canny_hip_compose_motion(const long long *motion, int n_pairs, int first_frame, long long *xforms)
{
    if (n_pairs < 0 || first_frame < 0 || !xforms || (n_pairs > 0 && !motion) || ((uintptr_t)motion & 7) ||
        ((uintptr_t)xforms & 7))
        return CANNY_HIP_ERR_INVALID;
    if (n_pairs > kMaxFrames) return CANNY_HIP_ERR_UNSUPPORTED;
    i64 p[6] = {65536, 0, 0, 0, 65536, 0};
    bool ok = true;
    for (int k = 0; k <= n_pairs; k++) {
        if (k > 0) {
            const i64 *rec = motion + (size_t)(k - 1) * CANNY_HIP_MOTION_WORDS, *m = rec + 4;
            ok = ok && (rec[0] & 3) == 3 && within_limits(m);
            if (ok) {
                // |m_ij|, |p_ij| <= 2^24: the linear sums stay under 2^50; |p_t| <= 2^36: the translation sums under 2^62
                const i64 c[6] = {fl16(m[0] * p[0] + m[1] * p[3]), fl16(m[0] * p[1] + m[1] * p[4]),
                                  fl16(m[0] * p[2] + m[1] * p[5]) + m[2],
                                  fl16(m[3] * p[0] + m[4] * p[3]), fl16(m[3] * p[1] + m[4] * p[4]),
                                  fl16(m[3] * p[2] + m[4] * p[5]) + m[5]};
                ok = within_limits(c);
                if (ok) std::memcpy(p, c, sizeof p);
            }
        }
        long long *o = xforms + (size_t)k * CANNY_HIP_XFORM_WORDS;
        o[0] = ok ? 1 : 0, o[1] = (i64)first_frame + k;
        for (int i = 0; i < 6; i++) o[2 + i] = ok ? p[i] : 0;
    }
    return CANNY_HIP_OK;
}

extern "C" int canny_hip_warp_frames(const unsigned char *src, int n_src, int src_h, int src_w, const long long *xforms,
                                     int n_out, int out_h, int out_w, int interp, int border, unsigned char *out,
                                     unsigned char *valid_bits)
{
    if (!src || !xforms || !out || n_src < 1 || n_out < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 ||
        (interp != CANNY_HIP_WARP_NEAREST && interp != CANNY_HIP_WARP_BILINEAR) || border < 0 || border > 255 ||
        ((uintptr_t)xforms & 7))
        return CANNY_HIP_ERR_INVALID;
    if (src_h > kMaxDim || src_w > kMaxDim || out_h > kMaxDim || out_w > kMaxDim || (i64)src_h * src_w >= kMaxPlane ||
        (i64)out_h * out_w >= kMaxPlane || n_src > kMaxFrames || n_out > kMaxFrames)
        return CANNY_HIP_ERR_UNSUPPORTED;
    const size_t src_plane = (size_t)src_h * src_w, out_plane = (size_t)out_h * out_w, row_bytes = ((size_t)out_w + 7) / 8;
    const size_t src_bytes = src_plane * n_src, out_bytes = out_plane * n_out, valid_bytes = row_bytes * out_h * n_out;
    if (overlap(src, src_bytes, out, out_bytes) ||
        (valid_bits && (overlap(src, src_bytes, valid_bits, valid_bytes) || overlap(out, out_bytes, valid_bits, valid_bytes))))
        return CANNY_HIP_ERR_INVALID;

    const unsigned char bd = (unsigned char)border;
    for (int o = 0; o < n_out; o++) {
        const long long *rec = xforms + (size_t)o * CANNY_HIP_XFORM_WORDS;
        unsigned char *dst = out + out_plane * o, *vb = valid_bits ? valid_bits + row_bytes * out_h * o : nullptr;
        if (vb) std::memset(vb, 0, row_bytes * out_h);
        if (!((rec[0] & 1) && within_limits(rec + 2) && rec[1] >= 0 && rec[1] < n_src)) {
            std::memset(dst, bd, out_plane);
            continue;
        }
        const unsigned char *plane = src + src_plane * (size_t)rec[1];
        const i64 a11 = rec[2], a12 = rec[3], tx = rec[4], a21 = rec[5], a22 = rec[6], ty = rec[7];
        auto tap = [&](i64 sy, i64 sx, bool &inside) -> int {
            inside = sx >= 0 && sx < src_w && sy >= 0 && sy < src_h;
            return inside ? plane[(size_t)sy * src_w + (size_t)sx] : bd;
        };
        for (int y = 0; y < out_h; y++)
            for (int x = 0; x < out_w; x++) {
                const i64 X = a11 * x + a12 * y + tx, Y = a21 * x + a22 * y + ty; // |X|, |Y| < 2^41
                int px;
                bool ok;
                if (interp == CANNY_HIP_WARP_NEAREST) {
                    px = tap(fl(Y + 32768, 16), fl(X + 32768, 16), ok);
                } else {
                    const i64 X8 = fl(X + 128, 8), Y8 = fl(Y + 128, 8);
                    const i64 ix = fl(X8, 8), iy = fl(Y8, 8);
                    const int fx = (int)(X8 - ix * 256), fy = (int)(Y8 - iy * 256);
                    bool i00, i01, i10, i11;
                    const int p00 = tap(iy, ix, i00), p01 = tap(iy, ix + 1, i01), p10 = tap(iy + 1, ix, i10),
                              p11 = tap(iy + 1, ix + 1, i11);
                    px = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11 + 32768) >> 16;
                    ok = i00 && (i01 || !fx) && (i10 || !fy) && (i11 || !fx || !fy);
                }
                dst[(size_t)y * out_w + x] = (unsigned char)px;
                if (vb && ok) vb[row_bytes * y + (x >> 3)] |= (unsigned char)(0x80 >> (x & 7));
            }
    }
    return CANNY_HIP_OK;
}
