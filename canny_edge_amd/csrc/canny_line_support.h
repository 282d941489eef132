// canny_line_support.h -- device code that more than one file must agree on to the bit: where a Hough line's support
// lies (canny_hough_segments.hip walks it for the runs, canny_line_fits.hip for the fit) and what the edgel of a pixel is
// (canny_edgels.hip stores it, canny_line_fits.hip sums it).  One copy each, as with vote_r and sobel_pair in
// canny_kernels.h, so that the support and the edgels of the fit cannot drift from the segments' and the edgels' own.
#pragma once

#include "canny_kernels.h"

#include "canny_hip.h"

namespace canny {

// ---- the support of a line ------------------------------------------------------------------
struct SegSrc {
    const uint32_t *strong32; // the strong plane as 32-bit halves of its words
    const uint8_t *bits;      // packed rows, any byte address
    uint32_t *work;           // exclusive mode: the private copy (see launch_hough_segments_exclusive)
    size_t work_frame_words;  // ... of packed bytes: 32-bit words from one frame's start to the next
};

// Where pixel (y, x) of frame f lives in a 32-bit view: of the strong plane (or its copy), or -- BITS -- of the private
// copy of packed bytes, whose frames each start on a word of their own (frame_words apart): no word holds two frames' bits.
template <bool BITS>
__device__ __forceinline__ void bit_of(const HystGeom &g, int row_bytes, size_t frame_words, int f, int y, int x,
                                       size_t *word, unsigned *mask)
{
    if constexpr (!BITS) {
        *word = hyst_word_index(g, f, y, x >> 6) * 2 + (size_t)((x >> 5) & 1);
        *mask = 1u << (x & 31);
    } else {
        const size_t b = (size_t)y * (size_t)row_bytes + (size_t)(x >> 3); // byte within the frame; rows MSB-first
        *word = (size_t)f * frame_words + (b >> 2);
        *mask = 1u << (8 * (int)(b & 3) + 7 - (x & 7));
    }
}

// pixel (y, x) of frame f in the source itself (not a working copy): the strong plane, or -- BITS -- packed rows
template <bool BITS>
__device__ __forceinline__ bool pixel_set_src(const SegSrc &src, const HystGeom &g, int row_bytes, int f, int y, int x)
{
    if constexpr (!BITS) {
        size_t word;
        unsigned mask;
        bit_of<false>(g, row_bytes, 0, f, y, x, &word, &mask);
        return (src.strong32[word] & mask) != 0;
    } else {
        const size_t b = ((size_t)f * g.height + y) * (size_t)row_bytes + (size_t)(x >> 3);
        return ((src.bits[b] >> (7 - (x & 7))) & 1) != 0;
    }
}

struct SegLine {
    float c, s;   // the angle's table entries
    int r, half;  // the cell's column; (numrho - 1) / 2
    bool major_x;
    int L, M;     // extent of the major and of the minor axis
};

// The line of accumulator cell `base`; false: the base is not a cell of the accumulator -- no segment, no access
__device__ __forceinline__ bool seg_line(unsigned base, const float *__restrict__ tab, int numangle, int numrho,
                                         const HystGeom &g, SegLine &ln)
{
    const unsigned stride = (unsigned)numrho + 2u;
    const int n = (int)(base / stride) - 1, r = (int)(base % stride) - 1;
    if ((unsigned)n >= (unsigned)numangle || (unsigned)r >= (unsigned)numrho) return false;
    ln.c = tab[n];
    ln.s = tab[numangle + n];
    ln.r = r;
    ln.half = (numrho - 1) / 2;
    ln.major_x = fabsf(ln.s) >= fabsf(ln.c);
    ln.L = ln.major_x ? g.width : g.height;
    ln.M = ln.major_x ? g.height : g.width;
    return true;
}

// The minor coordinates [*ma, *mb] to test with the exact vote at major position t: the float solution of the line
// +- halfwin (hough_segments_halfwin), clipped to the frame.  false: none (off the frame, or no estimate at all).
__device__ __forceinline__ bool seg_window(const SegLine &ln, float halfwin, int t, int *ma, int *mb)
{
    const float c_major = ln.major_x ? ln.c : ln.s, c_minor = ln.major_x ? ln.s : ln.c; // |c_minor| >= |c_major|, never 0
    const float m0 = ((float)(ln.r - ln.half) - (float)t * c_major) / c_minor;
    const float a = fmaxf(floorf(m0 - halfwin), 0.0f);
    const float b = fminf(fminf(ceilf(m0 + halfwin), (float)(ln.M - 1)), 2147483520.0f);
    if (!(a <= b)) return false;
    *ma = (int)a;
    *mb = min((int)b, ln.M - 1);
    return true;
}

// ---- the edgel of a pixel -------------------------------------------------------------------
// floor(sqrt(256 * (gx^2 + gy^2))), exact: the double root of a value below 2^40 is within one of the integer root, and
// the two steps settle it in 64 bits.  gx, gy in [-32768, 32767]: the sum of squares is <= 2^31, formed in unsigned.
__device__ __forceinline__ unsigned edgel_mag_q4(int gx, int gy)
{
    const unsigned m = (unsigned)(gx * gx) + (unsigned)(gy * gy);
    const unsigned long long v = (unsigned long long)m << 8;
    unsigned long long r = (unsigned long long)sqrt((double)v);
    if (r * r > v) r--;
    if ((r + 1) * (r + 1) <= v) r++;
    return (unsigned)r;
}

// OpenCV's integer octant test: 0 = step (1, 0), 1 = (1, 1), 2 = (0, 1), 3 = (1, -1); (0, 0) -> 0
__device__ __forceinline__ int edgel_dir(int gx, int gy)
{
    const unsigned ax = (unsigned)(gx < 0 ? -gx : gx), ay = (unsigned)(gy < 0 ? -gy : gy);
    const unsigned t22 = ax * 13573u, y15 = ay << 15, t67 = t22 + (ax << 16);
    if (!(gx | gy) || y15 < t22) return 0;
    if (y15 > t67) return 2;
    return (gx ^ gy) >= 0 ? 1 : 3;
}

// t_q8 of three magnitudes (each < 2^20); *refined = b >= a, b >= c and 2b - a - c > 0
__device__ __forceinline__ int edgel_offset(unsigned a, unsigned b, unsigned c, bool *refined)
{
    const bool ok = b >= a && b >= c && 2u * b > a + c;
    *refined = ok;
    if (!ok) return 0;
    const unsigned dn = 2u * b - a - c, d = c >= a ? c - a : a - c;
    const int t = (int)((256u * d + dn) / (2u * dn));
    return c >= a ? t : -t;
}

template <class T>
__device__ __forceinline__ unsigned edgel_mag_at(const T *__restrict__ img, int h, int w, int y, int x)
{
    int gx, gy;
    sobel_pair(img, h, w, y, x, &gx, &gy);
    return edgel_mag_q4(gx, gy);
}

// THE record of pixel (x, y), 0 <= x < w, 0 <= y < h
template <class T>
__device__ __forceinline__ uint4 edgel_record(const T *__restrict__ img, int h, int w, int y, int x)
{
    int gx, gy;
    sobel_pair(img, h, w, y, x, &gx, &gy);
    const unsigned b = edgel_mag_q4(gx, gy);
    const int dir = edgel_dir(gx, gy);
    const int dx = dir != 2, dy = dir == 0 ? 0 : (dir == 3 ? -1 : 1);
    const int xa = x - dx, ya = y - dy, xc = x + dx, yc = y + dy;
    int t = 0;
    unsigned flag = 0;
    if ((gx | gy) && xa >= 0 && xc < w && (unsigned)ya < (unsigned)h && (unsigned)yc < (unsigned)h) {
        const unsigned a = edgel_mag_at(img, h, w, ya, xa), c = edgel_mag_at(img, h, w, yc, xc);
        bool ok;
        t = edgel_offset(a, b, c, &ok);
        if (ok) flag = CANNY_HIP_EDGEL_REFINED;
    }
    return make_uint4((unsigned)(256 * x + t * dx), (unsigned)(256 * y + t * dy),
                      ((unsigned)gx & 0xffffu) | ((unsigned)gy << 16),
                      b | (unsigned)dir << CANNY_HIP_EDGEL_DIR_SHIFT | flag);
}

} // namespace canny
