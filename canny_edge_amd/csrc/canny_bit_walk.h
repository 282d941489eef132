// canny_bit_walk.h -- the walking window over a bit map that the contour chains (canny_contours.hip)
// and the edge curves (canny_curves.hip, section 28) share: a thread that follows pixels one step at a time keeps 3 rows x
// 64 columns of the map in six registers (three 64-bit words), centred on the pixel at which it was loaded; the 3 x 3 ring
// around the current pixel is eight bits taken from the three words.  A vertical step shifts the rows and loads one; the
// whole window is reloaded only when the walk comes within one column of its edge, 31 columns from where it was centred.
// No table, no LDS.  The source is the strong plane or a packed bit map at any byte address (row_word<BITS>).
//
// Device code only, everything forced inline and file-local: a kernel file that includes this compiles to what it
// compiled to with the text in place.
#ifndef CANNY_BIT_WALK_H
#define CANNY_BIT_WALK_H
#include "canny_kernels.h"

namespace canny {

namespace {

// columns 64*k .. 64*k + 63 of row y of frame f, bit i = column 64*k + i; everything outside the frame reads as 0
template <bool BITS>
__device__ __forceinline__ uint64_t ct_word(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f, int y,
                                            int k)
{
    if (y < 0 || y >= g.height || k < 0 || k >= g.tiles_x) return 0ull;
    return row_word<BITS>(src, g, row_bytes, f, y, k);
}

// columns c0 .. c0 + 63 of row y, bit i = column c0 + i; c0 may be negative (>> floors)
template <bool BITS>
__device__ __forceinline__ uint64_t ct_window(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f, int y,
                                              int c0)
{
    const int k = c0 >> 6, sh = c0 & 63;
    const uint64_t lo = ct_word<BITS>(src, g, row_bytes, f, y, k);
    if (!sh) return lo;
    return (lo >> sh) | (ct_word<BITS>(src, g, row_bytes, f, y, k + 1) << (64 - sh));
}

// directions clockwise on the displayed image: 0 E, 1 SE, 2 S, 3 SW, 4 W, 5 NW, 6 N, 7 NE; two bits per direction, step + 1
__device__ __forceinline__ int ct_dx(int d) { return (int)((0x901Au >> (2 * d)) & 3u) - 1; }
__device__ __forceinline__ int ct_dy(int d) { return (int)((0x01A9u >> (2 * d)) & 3u) - 1; }

struct CtWalk {
    int y, x, c0; // the current pixel; the window's first column: 1 <= x - c0 <= 62
    uint64_t up, mid, dn;
};

template <bool BITS>
__device__ __forceinline__ void ct_load(CtWalk &w, const void *__restrict__ src, const HystGeom &g, int row_bytes, int f)
{
    w.c0 = w.x - 32;
    w.up = ct_window<BITS>(src, g, row_bytes, f, w.y - 1, w.c0);
    w.mid = ct_window<BITS>(src, g, row_bytes, f, w.y, w.c0);
    w.dn = ct_window<BITS>(src, g, row_bytes, f, w.y + 1, w.c0);
}

// bit d = the neighbour in direction d is set
__device__ __forceinline__ unsigned ct_ring(const CtWalk &w)
{
    const int sh = w.x - w.c0 - 1;
    const unsigned u = (unsigned)(w.up >> sh) & 7u, m = (unsigned)(w.mid >> sh) & 7u, d = (unsigned)(w.dn >> sh) & 7u;
    return (m >> 2) | ((d >> 2) << 1) | (((d >> 1) & 1u) << 2) | ((d & 1u) << 3) | ((m & 1u) << 4) | ((u & 1u) << 5) |
           (((u >> 1) & 1u) << 6) | ((u >> 2) << 7);
}

template <bool BITS>
__device__ __forceinline__ void ct_move(CtWalk &w, int d, const void *__restrict__ src, const HystGeom &g, int row_bytes,
                                        int f)
{
    const int dy = ct_dy(d);
    w.y += dy;
    w.x += ct_dx(d);
    const int b = w.x - w.c0;
    if (b < 1 || b > 62) {
        ct_load<BITS>(w, src, g, row_bytes, f);
    } else if (dy > 0) {
        w.up = w.mid, w.mid = w.dn;
        w.dn = ct_window<BITS>(src, g, row_bytes, f, w.y + 1, w.c0);
    } else if (dy < 0) {
        w.dn = w.mid, w.mid = w.up;
        w.up = ct_window<BITS>(src, g, row_bytes, f, w.y - 1, w.c0);
    }
}

} // namespace

} // namespace canny

// one wave per image row of the batch, grid-stride: r = f * height + y is the same in all 64 lanes
#define CT_FOR_EACH_ROW(g, r)                                                                                           \
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_rows_ = (size_t)(g).n_frames * (g).height,  \
                stride_ = ((size_t)gridDim.x * blockDim.x) >> 6;                                                        \
         r < n_rows_; r += stride_)

#endif // CANNY_BIT_WALK_H
