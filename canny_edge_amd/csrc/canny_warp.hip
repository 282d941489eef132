// canny_warp.hip -- frame alignment: the motion records of consecutive pairs chained into one transform per frame, and u8
// frames warped by such transforms (inverse map, NEAREST / BILINEAR in Q8 weights, constant border, valid bits).  The rules
// are part of the interface (include/canny_hip.h); tests/warp_rule.py restates them in numpy and Python
// ints, canny_warp_host.cpp in plain C++.  All integers, no atomics, every output byte has one writer: the same bytes on
// every run.
//
//   compose : one lane walks the chain (the rounding makes it sequential); 8 words a record.
//   warp    : one workgroup of 256 lanes per 64 x 16 output tile and trip of a capped grid.  A lane produces four adjacent
//             output pixels, stepping X += a11, Y += a21 (exact: the map is linear in integers), and stores them as one
//             32-bit word; two neighbouring lanes join their valid bits into the byte of their eight pixels.
//             direct: the taps are gathered from global memory through the vector cache.
//             tiled : the tile's source footprint -- the bounding box of the images of its four corners, one more row and
//                     column under BILINEAR, clipped to the source -- is staged in LDS with coalesced row loads if it fits
//                     kLdsBytes, and the taps come from LDS; a tile whose footprint does not fit gathers directly.  The
//                     decision is made from the record on the device and is the same on every lane of the workgroup.
#include "canny_kernels.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 16; // the corners' tile
constexpr int kPx = 4;                  // adjacent output pixels of a lane: one 32-bit store
constexpr unsigned kGridCap = 4096;
constexpr int kLdsBytes = 16384;        // CANNY_HIP_WARP_LDS_BYTES
constexpr long long kLimA = 1ll << 24, kLimT = 1ll << 36;
constexpr int kXformWords = 8, kMotionWords = 16;

static_assert(kTileW / kPx * kTileH == kBlock, "one lane per run of kPx pixels of the tile");

__host__ __device__ inline long long wp_min(long long a, long long b) { return a < b ? a : b; }
__host__ __device__ inline long long wp_max(long long a, long long b) { return a > b ? a : b; }
__host__ __device__ inline bool wp_within(long long v, long long lim) { return v >= -lim && v <= lim; }

// c: a11, a12, tx, a21, a22, ty
__host__ __device__ inline bool wp_within_limits(const long long *c)
{
    return wp_within(c[0], kLimA) && wp_within(c[1], kLimA) && wp_within(c[3], kLimA) && wp_within(c[4], kLimA) &&
           wp_within(c[2], kLimT) && wp_within(c[5], kLimT);
}

__host__ __device__ inline bool wp_usable(const long long *r, int n_src)
{
    return (r[0] & 1) && wp_within_limits(r + 2) && r[1] >= 0 && r[1] < n_src;
}

// LDS row pitch of a footprint bw bytes wide: whole words, an odd number of them
__host__ __device__ inline int wp_pitch(int bw)
{
    const int words = (bw + 3) >> 2;
    return (words | 1) << 2;
}

struct WarpBox {
    int x0, y0, x1, y1; // inclusive, clipped to the source; x1 < x0 or y1 < y0: empty
};

// The footprint of the output pixels [x0, x1] x [y0, y1] under the coefficients c: the map is affine, so the bounding box of
// the four corners' images bounds every pixel's; the tap index is monotone in the position.  True: not empty and it fits LDS.
__host__ __device__ inline bool wp_footprint(const long long *c, int interp, int src_h, int src_w, int x0, int y0, int x1,
                                             int y1, WarpBox &b)
{
    long long lo[2], hi[2];
    for (int i = 0; i < 2; i++) {
        const long long a = c[3 * i], bb = c[3 * i + 1], t = c[3 * i + 2];
        const long long v00 = a * x0 + bb * y0 + t, v01 = a * x1 + bb * y0 + t, v10 = a * x0 + bb * y1 + t,
                        v11 = a * x1 + bb * y1 + t;
        const long long mn = wp_min(wp_min(v00, v01), wp_min(v10, v11)), mx = wp_max(wp_max(v00, v01), wp_max(v10, v11));
        if (interp == 0)
            lo[i] = (mn + 32768) >> 16, hi[i] = (mx + 32768) >> 16;
        else
            lo[i] = (mn + 128) >> 16, hi[i] = ((mx + 128) >> 16) + 1;
    }
    const long long bx0 = wp_max(lo[0], 0), bx1 = wp_min(hi[0], (long long)src_w - 1);
    const long long by0 = wp_max(lo[1], 0), by1 = wp_min(hi[1], (long long)src_h - 1);
    if (bx1 < bx0 || by1 < by0) {
        b = WarpBox{0, 0, -1, -1};
        return false;
    }
    b = WarpBox{(int)bx0, (int)by0, (int)bx1, (int)by1};
    return (long long)wp_pitch((int)(bx1 - bx0 + 1)) * (by1 - by0 + 1) <= kLdsBytes;
}

// The automatic route stages a tile only where the measurement shows the tiled route ahead (profiles/warp.jsonl, DESIGN.md
// section 32): under BILINEAR when an output row runs more along the source's columns than along its rows (|a21| >= |a11|,
// a turn of 45 degrees or more; measured at the quarter turn).  Everywhere else the direct gather is faster.
__host__ __device__ inline bool wp_auto_tiled(const long long *c, int interp)
{
    const long long a11 = c[0] < 0 ? -c[0] : c[0], a21 = c[3] < 0 ? -c[3] : c[3];
    return interp == 1 && a21 >= a11 && a21 > 0;
}

// grid (1), one lane: the chain of the rule
__global__ __launch_bounds__(64) void warp_compose_kernel(const long long *__restrict__ motion, int n_pairs, int first_frame,
                                                          long long *__restrict__ xforms)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long p[6] = {65536, 0, 0, 0, 65536, 0};
    bool ok = true;
    for (int k = 0; k <= n_pairs; k++) {
        if (k > 0) {
            const long long *rec = motion + (size_t)(k - 1) * kMotionWords;
            long long m[6];
            for (int i = 0; i < 6; i++) m[i] = rec[4 + i];
            ok = ok && (rec[0] & 3) == 3 && wp_within_limits(m);
            if (ok) {
                // linear sums under 2^50, translation sums under 2^62; >> on a signed value is arithmetic here: the floor
                const long long c[6] = {(m[0] * p[0] + m[1] * p[3]) >> 16, (m[0] * p[1] + m[1] * p[4]) >> 16,
                                        ((m[0] * p[2] + m[1] * p[5]) >> 16) + m[2],
                                        (m[3] * p[0] + m[4] * p[3]) >> 16, (m[3] * p[1] + m[4] * p[4]) >> 16,
                                        ((m[3] * p[2] + m[4] * p[5]) >> 16) + m[5]};
                ok = wp_within_limits(c);
                if (ok)
                    for (int i = 0; i < 6; i++) p[i] = c[i];
            }
        }
        long long *o = xforms + (size_t)k * kXformWords;
        o[0] = ok ? 1 : 0, o[1] = (long long)first_frame + k;
        for (int i = 0; i < 6; i++) o[2 + i] = ok ? p[i] : 0;
    }
}

// What a lane needs to fetch a tap: kTiled reads the staged box, otherwise the plane.
struct TapSrc {
    const uint8_t *plane; // the source frame
    int src_h, src_w;
    const uint8_t *lds;
    WarpBox b;
    int pitch;
    int border;
};

template <bool kTiled>
__device__ __forceinline__ int wp_tap(const TapSrc &s, int sy, int sx, bool &inside)
{
    if (kTiled) {
        // inside the clipped box: for a pixel of the tile the same as inside the source; lanes past the frame's edge compute
        // pixels nobody stores, and this keeps their reads inside the staged bytes
        inside = sx >= s.b.x0 && sx <= s.b.x1 && sy >= s.b.y0 && sy <= s.b.y1;
        return inside ? s.lds[(sy - s.b.y0) * s.pitch + (sx - s.b.x0)] : s.border;
    }
    inside = (unsigned)sx < (unsigned)s.src_w && (unsigned)sy < (unsigned)s.src_h;
    return inside ? s.plane[(size_t)sy * s.src_w + sx] : s.border;
}

// kPx pixels from (X, Y) on: the bytes packed little-endian, the valid bits MSB-first in a nibble
template <int kInterp, bool kTiled>
__device__ __forceinline__ void wp_run(const TapSrc &s, long long X, long long Y, long long a11, long long a21, unsigned &px,
                                       unsigned &nib)
{
    px = 0, nib = 0;
#pragma unroll
    for (int j = 0; j < kPx; j++) {
        int v;
        bool ok;
        if (kInterp == 0) {
            v = wp_tap<kTiled>(s, (int)((Y + 32768) >> 16), (int)((X + 32768) >> 16), ok); // |X| < 2^41: the index fits an int
        } else {
            const long long X8 = (X + 128) >> 8, Y8 = (Y + 128) >> 8; // under 2^33: the indices fit an int, X8 does not
            const int ix = (int)(X8 >> 8), fx = (int)(X8 & 255), iy = (int)(Y8 >> 8), fy = (int)(Y8 & 255);
            bool i00, i01, i10, i11;
            const int p00 = wp_tap<kTiled>(s, iy, ix, i00), p01 = wp_tap<kTiled>(s, iy, ix + 1, i01);
            const int p10 = wp_tap<kTiled>(s, iy + 1, ix, i10), p11 = wp_tap<kTiled>(s, iy + 1, ix + 1, i11);
            v = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11 + 32768) >> 16;
            ok = i00 && (i01 || !fx) && (i10 || !fy) && (i11 || !fx || !fy);
        }
        px |= (unsigned)v << (8 * j);
        nib |= (ok ? 1u : 0u) << (kPx - 1 - j);
        X += a11, Y += a21;
    }
}

// grid plan_warp_tiles: units = n_out * tiles_y * tiles_x.  vec_ok: out_w is a multiple of 4 and `out` is 4-byte aligned.
template <int kInterp>
__global__ __launch_bounds__(kBlock) void warp_kernel(const uint8_t *__restrict__ src, int n_src, int src_h, int src_w,
                                                      const long long *__restrict__ xforms,
                                                      unsigned long long n_units, unsigned tiles_x, unsigned tiles_y, int out_h, int out_w, int route,
                                                      int border, uint8_t *__restrict__ out, uint8_t *__restrict__ valid,
                                                      int vec_ok)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_px[kLdsBytes];
    const int tid = threadIdx.x, lx = (tid & (kTileW / kPx - 1)) * kPx, ly = tid / (kTileW / kPx);
    const size_t row_bytes = ((size_t)out_w + 7) >> 3;
    for (unsigned long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const unsigned long long t = u / tiles_x;
        const unsigned tx = (unsigned)(u % tiles_x), ty = (unsigned)(t % tiles_y), o = (unsigned)(t / tiles_y);
        long long r[kXformWords];
        for (int i = 0; i < kXformWords; i++) r[i] = xforms[(size_t)o * kXformWords + i];
        const bool usable = wp_usable(r, n_src);
        const int x0 = (int)tx * kTileW, y0 = (int)ty * kTileH;
        TapSrc s;
        s.src_h = src_h, s.src_w = src_w, s.lds = s_px, s.border = border, s.pitch = 0, s.b = WarpBox{0, 0, -1, -1};
        s.plane = src + (usable ? (size_t)r[1] * ((size_t)src_h * src_w) : 0);
        bool staged = false;
        if (usable && route != 1) {
            const bool fits = wp_footprint(r + 2, kInterp, src_h, src_w, x0, y0, (int)wp_min(x0 + kTileW, out_w) - 1,
                                           (int)wp_min(y0 + kTileH, out_h) - 1, s.b);
            staged = fits && (route == 2 || wp_auto_tiled(r + 2, kInterp));
        }
        if (staged) { // the same on every lane of the workgroup
            __syncthreads(); // an earlier trip's taps are read before this one stages
            const int bw = s.b.x1 - s.b.x0 + 1, bh = s.b.y1 - s.b.y0 + 1;
            s.pitch = wp_pitch(bw);
            // the lanes of a row: the smallest power of two that covers it, the block's lanes at most
            int lanes = kBlock, shift = 8;
            while ((lanes >> 1) >= bw) lanes >>= 1, shift--;
            const uint8_t *from = s.plane + (size_t)s.b.y0 * src_w + s.b.x0;
            for (int row = tid >> shift; row < bh; row += kBlock >> shift)
                for (int col = tid & (lanes - 1); col < bw; col += lanes)
                    s_px[row * s.pitch + col] = from[(size_t)row * src_w + col];
            __syncthreads();
        }
        const int x = x0 + lx, y = y0 + ly;
        unsigned px = 0x01010101u * (unsigned)border, nib = 0;
        if (usable) {
            const long long X = r[2] * x + r[3] * y + r[4], Y = r[5] * x + r[6] * y + r[7];
            if (staged)
                wp_run<kInterp, true>(s, X, Y, r[2], r[5], px, nib);
            else
                wp_run<kInterp, false>(s, X, Y, r[2], r[5], px, nib);
        }
        const int left = out_w - x; // pixels of this run inside the row, if positive
        if (left < kPx) nib = left > 0 ? nib & (0xfu << (kPx - left)) & 0xfu : 0; // pad bits are 0
        const bool mine = y < out_h && left > 0;
        if (mine) {
            uint8_t *dst = out + ((size_t)o * out_h + y) * out_w + x;
            if (vec_ok && left >= kPx) {
                *(unsigned *)dst = px;
            } else {
                for (int j = 0; j < kPx && j < left; j++) dst[j] = (uint8_t)(px >> (8 * j));
            }
        }
        if (valid) { // uniform: every lane takes part in the exchange
            const unsigned other = (unsigned)__shfl_xor((int)nib, 1);
            if (mine && !(tid & 1)) valid[((size_t)o * out_h + y) * row_bytes + (x >> 3)] = (uint8_t)((nib << 4) | other);
        }
    }
}

} // namespace

LaunchPlan plan_warp_tiles(int n_out, int out_h, int out_w)
{
    const unsigned long long tiles = (unsigned long long)((out_w + kTileW - 1) / kTileW) * ((out_h + kTileH - 1) / kTileH);
    return capped_plan(tiles * (unsigned long long)n_out, 1, kGridCap);
}

bool warp_tile_footprint(const long long *xform, int interp, int src_h, int src_w, int out_h, int out_w, int tile_x,
                         int tile_y, int box[4])
{
    WarpBox b{0, 0, -1, -1};
    bool fits = false;
    if ((xform[0] & 1) && wp_within_limits(xform + 2)) {
        const int x0 = tile_x * kTileW, y0 = tile_y * kTileH;
        fits = wp_footprint(xform + 2, interp, src_h, src_w, x0, y0, (int)wp_min(x0 + kTileW, out_w) - 1,
                            (int)wp_min(y0 + kTileH, out_h) - 1, b);
    }
    box[0] = b.x0, box[1] = b.y0, box[2] = b.x1, box[3] = b.y1;
    return fits;
}

hipError_t launch_warp_compose(const long long *motion, int n_pairs, int first_frame, long long *xforms, hipStream_t stream)
{
    if (n_pairs < 0 || n_pairs > 65535 || first_frame < 0 || !xforms || (n_pairs && !motion)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_compose_kernel, dim3(1), dim3(64), 0, stream, motion, n_pairs, first_frame, xforms);
    return hipGetLastError();
}

hipError_t launch_warp_frames(const uint8_t *src, int n_src, int src_h, int src_w, const long long *xforms, int n_out,
                              int out_h, int out_w, int interp, int border, int route, uint8_t *out, uint8_t *valid,
                              hipStream_t stream)
{
    if (!src || !xforms || !out || n_src < 1 || n_out < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 ||
        src_h > 32768 || src_w > 32768 || out_h > 32768 || out_w > 32768 || n_src > 65535 || n_out > 65535 || interp < 0 ||
        interp > 1 || border < 0 || border > 255 || route < 0 || route > 2)
        return hipErrorInvalidValue;
    const LaunchPlan p = plan_warp_tiles(n_out, out_h, out_w);
    const unsigned tiles_x = (unsigned)((out_w + kTileW - 1) / kTileW), tiles_y = (unsigned)((out_h + kTileH - 1) / kTileH);
    const int vec_ok = !(out_w & 3) && !((uintptr_t)out & 3);
    if (interp == 0)
        hipLaunchKernelGGL(warp_kernel<0>, dim3(p.grid), dim3(kBlock), 0, stream, src, n_src, src_h, src_w, xforms,
                           p.units, tiles_x, tiles_y, out_h, out_w, route, border, out, valid, vec_ok);
    else
        hipLaunchKernelGGL(warp_kernel<1>, dim3(p.grid), dim3(kBlock), 0, stream, src, n_src, src_h, src_w, xforms,
                           p.units, tiles_x, tiles_y, out_h, out_w, route, border, out, valid, vec_ok);
    return hipGetLastError();
}

} // namespace canny
