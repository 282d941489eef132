// canny_line_fits.hip -- sub-pixel line fits: for every Hough segment record the total-least-squares line through the
// sub-pixel edgels of the segment's pixels, the sub-pixel end points on it and the residuals, in one 48-byte record.  The
// rule is part of the interface (include/canny_hip.h); tests/line_fits_rule.py restates it in Python
// ints, canny_line_fits_host.cpp in plain C++.
//
// One wave per segment slot, four to a workgroup, grid (ceil(segments_max / 4), n_frames): seg_walk_kernel's shape, with
// its early exit past the frame's count, so no grid cap and no atomics.  The wave walks the segment's major positions
// [ta, tb] 64 at a time as the segment walk does (seg_window + the exact vote + the bit, canny_line_support.h); a lane
// computes the edgel record of each support pixel of its position (edgel_record, the edgel kernels' own function) and adds
// it to six 64-bit sums of its own.  One xor-shuffle reduction per segment leaves the sums in every lane; the finishing
// arithmetic (128 bits for A, B, C only, two exact roots, four divisions) is then the same in all lanes.  A second walk
// over the same positions recomputes the edgels for the residuals and the extent (sum, max, min reductions), and lanes
// 0..11 store one word each.  No LDS, no scratch, plain C++.
#include "canny_line_support.h"
#include "canny_wave.h"

namespace canny {

namespace {

constexpr int kFitBlock = 256; // four waves, four segment slots
constexpr int kFitRecord = CANNY_HIP_LINE_FIT_INTS;

typedef __int128 i128;

// floor(sqrt(v)), exact, v < 2^63.  The conversion to double is off by at most 2^-53 of v and the root by half an ulp, so
// the truncated root lies within one of the integer root for v < 2^52 and within two up to 2^63; the steps go both ways,
// twice, and (r + 1)^2 <= (2^31.5 + 3)^2 cannot overflow.
__device__ __forceinline__ unsigned long long fit_isqrt(unsigned long long v)
{
    unsigned long long r = (unsigned long long)sqrt((double)v);
    if (r * r > v) r--;
    if (r * r > v) r--;
    if ((r + 1) * (r + 1) <= v) r++;
    if ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// a / b to nearest, halves away from zero; b > 0, 2 |a| + b < 2^63
__device__ __forceinline__ long long fit_rdiv(long long a, long long b)
{
    const unsigned long long m = (unsigned long long)(a < 0 ? -a : a);
    const long long q = (long long)((2 * m + (unsigned long long)b) / (2 * (unsigned long long)b));
    return a < 0 ? -q : q;
}

__device__ __forceinline__ int fit_bitlength(i128 v) // v >= 0
{
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    return hi ? 128 - (int)__builtin_clzll(hi) : (lo ? 64 - (int)__builtin_clzll(lo) : 0);
}

struct FitSums {
    long long n, su, sv, suu, suv, svv;
};
struct FitLine {
    long long mu, mv, dx, dy; // centroid relative to the first end point (1/65536 px); unit direction (q30)
    bool degenerate;
};

// steps 4 (from the sums on) to 6 of the rule
__device__ __forceinline__ FitLine fit_finish(const FitSums &m, int ddx, int ddy)
{
    FitLine f{0, 0, 0, 0, true};
    if (m.n) {
        f.mu = fit_rdiv(256 * m.su, m.n);
        f.mv = fit_rdiv(256 * m.sv, m.n);
    }
    const i128 A = (i128)m.n * m.suu - (i128)m.su * m.su;
    const i128 B = (i128)m.n * m.suv - (i128)m.su * m.sv;
    const i128 C = (i128)m.n * m.svv - (i128)m.sv * m.sv;
    i128 top = B < 0 ? -B : B;
    if (A > top) top = A;
    if (C > top) top = C;
    const int bl = fit_bitlength(top), s = bl > 28 ? bl - 28 : 0;
    const long long a = (long long)(A >> s), b = (long long)(B >> s), c = (long long)(C >> s); // arithmetic: floor
    const long long D = a - c, E = 2 * b;
    const long long h = (long long)fit_isqrt((unsigned long long)(D * D) + (unsigned long long)(E * E));
    if (m.n < 2 || h == 0) return f;
    long long wx, wy;
    if (D >= 0) {
        wx = h + D, wy = E;
    } else {
        wx = E < 0 ? -E : E, wy = E < 0 ? -(h - D) : h - D;
    }
    if (wx * ddx + wy * ddy < 0) wx = -wx, wy = -wy;
    // the larger component to exactly 31 bits (|w| < 2^30.3, so k >= 1): len >= 2^30 and the squares stay below 2^62
    const long long ax = wx < 0 ? -wx : wx, ay = wy < 0 ? -wy : wy;
    const int k = 31 - (64 - (int)__builtin_clzll((unsigned long long)(ax > ay ? ax : ay)));
    wx *= 1ll << k, wy *= 1ll << k;
    const long long len = (long long)fit_isqrt((unsigned long long)(wx * wx) + (unsigned long long)(wy * wy));
    f.dx = fit_rdiv(wx * (1ll << 30), len);
    f.dy = fit_rdiv(wy * (1ll << 30), len);
    f.degenerate = false;
    return f;
}

__device__ __forceinline__ long long fit_along(long long p, long long q) { return (p * q + (1ll << 29)) >> 30; }

struct FitSeg {
    int x0, y0, ddx, ddy, ta, tb;
};

// Steps 2 and 3: use(u, v) for every used pixel whose major position this lane holds in some chunk of [ta, tb].
template <bool BITS, class T, class Use>
__device__ __forceinline__ void fit_walk(const SegSrc &src, const HystGeom &g, int row_bytes, int f, const SegLine &ln,
                                         float halfwin, const FitSeg &sgm, const T *__restrict__ img, int options,
                                         Use &&use)
{
    const int lane = threadIdx.x & 63;
    for (int t = sgm.ta + lane; t <= sgm.tb; t += 64) {
        int ma, mb;
        if (!seg_window(ln, halfwin, t, &ma, &mb)) continue;
        for (int m = ma; m <= mb; m++) {
            const int x = ln.major_x ? t : m, y = ln.major_x ? m : t;
            if (vote_r(x, y, ln.c, ln.s, ln.half) != ln.r) continue;
            if (!pixel_set_src<BITS>(src, g, row_bytes, f, y, x)) continue;
            const uint4 e = edgel_record(img, g.height, g.width, y, x);
            if (options & CANNY_HIP_LINE_FIT_GATE) {
                const int gx = (int)(short)(e.z & 0xffffu), gy = (int)(short)(e.z >> 16);
                const long long dot = (long long)gx * sgm.ddx + (long long)gy * sgm.ddy;
                const long long g2 = (long long)gx * gx + (long long)gy * gy;
                const long long d2 = (long long)sgm.ddx * sgm.ddx + (long long)sgm.ddy * sgm.ddy;
                if (!(gx | gy) || 4 * dot * dot > g2 * d2) continue;
            }
            if ((options & CANNY_HIP_LINE_FIT_REFINED_ONLY) && !(e.w & CANNY_HIP_EDGEL_REFINED)) continue;
            use((long long)((int)e.x - 256 * sgm.x0), (long long)((int)e.y - 256 * sgm.y0));
        }
    }
}

// grid (ceil(segments_max / 4), n_frames); one wave per segment slot
template <bool BITS, class T>
__global__ __launch_bounds__(kFitBlock) void line_fits_kernel(SegSrc src, HystGeom g, int row_bytes,
                                                              const float *__restrict__ tab, int numangle, int numrho,
                                                              float halfwin, const unsigned *__restrict__ bases,
                                                              const int *__restrict__ line_counts, int lines_max,
                                                              const int *__restrict__ segments,
                                                              const int *__restrict__ seg_counts, int segments_max,
                                                              const T *__restrict__ plane, int options,
                                                              int *__restrict__ fits)
{
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * (kFitBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= min(segments_max, seg_counts[f])) return;
    const size_t slot = (size_t)f * segments_max + j;
    const int *rec = segments + slot * kSegRecord;
    const int x0 = rec[0], y0 = rec[1], x1 = rec[2], y1 = rec[3], k = rec[4];
    int word = 0; // what this lane stores, if lane < 12; the invalid record first
    if (lane == 9) word = (int)CANNY_HIP_LINE_FIT_INVALID;
    SegLine ln;
    bool valid = (unsigned)k < (unsigned)max(min(lines_max, line_counts[f]), 0) && (unsigned)x0 < (unsigned)g.width &&
                 (unsigned)x1 < (unsigned)g.width && (unsigned)y0 < (unsigned)g.height && (unsigned)y1 < (unsigned)g.height;
    if (valid) valid = seg_line(bases[(size_t)f * lines_max + k], tab, numangle, numrho, g, ln);
    FitSeg sgm{x0, y0, x1 - x0, y1 - y0, 0, 0};
    if (valid) {
        sgm.ta = ln.major_x ? x0 : y0;
        sgm.tb = ln.major_x ? x1 : y1;
        valid = sgm.ta <= sgm.tb;
    }
    if (valid) { // wave-uniform
        const T *img = plane + (size_t)f * g.height * g.width;
        FitSums m{0, 0, 0, 0, 0, 0};
        fit_walk<BITS>(src, g, row_bytes, f, ln, halfwin, sgm, img, options, [&](long long u, long long v) {
            m.n++, m.su += u, m.sv += v, m.suu += u * u, m.suv += u * v, m.svv += v * v;
        });
        m.n = wave_sum(m.n), m.su = wave_sum(m.su), m.sv = wave_sum(m.sv);
        m.suu = wave_sum(m.suu), m.suv = wave_sum(m.suv), m.svv = wave_sum(m.svv);
        const FitLine fl = fit_finish(m, sgm.ddx, sgm.ddy);
        const long long cx = 65536ll * x0 + fl.mu, cy = 65536ll * y0 + fl.mv;
        long long w[kFitRecord] = {65536ll * x0, 65536ll * y0, 65536ll * x1, 65536ll * y1, cx, cy, 0, 0, m.n,
                                   (long long)CANNY_HIP_LINE_FIT_DEGENERATE, 0, 0};
        if (!fl.degenerate) {
            unsigned long long sdd = 0;
            long long maxd = 0, pmin = 0x7fffffffffffffffll, pmax = -0x7fffffffffffffffll - 1;
            fit_walk<BITS>(src, g, row_bytes, f, ln, halfwin, sgm, img, options, [&](long long u, long long v) {
                const long long U = 256 * u - fl.mu, V = 256 * v - fl.mv;
                const long long d = (V * fl.dx - U * fl.dy + (1ll << 37)) >> 38;
                const long long p = (U * fl.dx + V * fl.dy + (1ll << 29)) >> 30;
                sdd += (unsigned long long)(d * d);
                const long long ad = d < 0 ? -d : d;
                maxd = ad > maxd ? ad : maxd;
                pmin = p < pmin ? p : pmin;
                pmax = p > pmax ? p : pmax;
            });
            sdd = (unsigned long long)wave_sum((long long)sdd);
            maxd = wave_max(maxd), pmin = wave_min(pmin), pmax = wave_max(pmax);
            w[0] = cx + fit_along(pmin, fl.dx), w[1] = cy + fit_along(pmin, fl.dy);
            w[2] = cx + fit_along(pmax, fl.dx), w[3] = cy + fit_along(pmax, fl.dy);
            w[6] = fl.dx, w[7] = fl.dy;
            w[9] = (long long)((unsigned)maxd & CANNY_HIP_LINE_FIT_MAXD_MASK);
            w[10] = (long long)(unsigned)sdd, w[11] = (long long)(unsigned)(sdd >> 32);
        }
        word = 0;
#pragma unroll
        for (int i = 0; i < kFitRecord; i++)
            if (lane == i) word = (int)(unsigned)(unsigned long long)w[i];
    }
    if (lane < kFitRecord) fits[slot * kFitRecord + lane] = word;
}

// one lane per moment set: in = (n, Su, Sv, Suu, Suv, Svv, ddx, ddy); out = words 4..8 with (x0, y0) = (0, 0), then the
// flags of word 9 (DEGENERATE or 0)
__global__ __launch_bounds__(256) void line_fits_arith_kernel(const long long *__restrict__ in, size_t n,
                                                              int *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const long long *p = in + 8 * i;
        const FitSums m{p[0], p[1], p[2], p[3], p[4], p[5]};
        const FitLine fl = fit_finish(m, (int)p[6], (int)p[7]);
        int *o = out + 6 * i;
        o[0] = (int)fl.mu, o[1] = (int)fl.mv, o[2] = (int)fl.dx, o[3] = (int)fl.dy, o[4] = (int)m.n;
        o[5] = fl.degenerate ? (int)CANNY_HIP_LINE_FIT_DEGENERATE : 0;
    }
}

} // namespace

hipError_t launch_line_fits(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                            const float *tab, const unsigned *bases, const int *line_counts, const int *segments,
                            const int *seg_counts, const void *plane, bool plane_u8, int options, int *fits,
                            hipStream_t stream)
{
    const dim3 grid((sg.segments_max + kFitBlock / 64 - 1) / (kFitBlock / 64), g.n_frames);
    const SegSrc src{reinterpret_cast<const uint32_t *>(strong), bits, nullptr, 0};
    auto launch = [&](auto kernel, auto *img) {
        hipLaunchKernelGGL(kernel, grid, dim3(kFitBlock), 0, stream, src, g, (g.width + 7) / 8, tab, sg.numangle, sg.numrho,
                           sg.halfwin, bases, line_counts, sg.lines_max, segments, seg_counts, sg.segments_max, img, options,
                           fits);
        return hipGetLastError();
    };
    if (bits)
        return plane_u8 ? launch(line_fits_kernel<true, uint8_t>, (const uint8_t *)plane)
                        : launch(line_fits_kernel<true, int16_t>, (const int16_t *)plane);
    return plane_u8 ? launch(line_fits_kernel<false, uint8_t>, (const uint8_t *)plane)
                    : launch(line_fits_kernel<false, int16_t>, (const int16_t *)plane);
}

hipError_t launch_line_fits_arith(const long long *moments, size_t n, int *out, hipStream_t stream)
{
    if (!n) return hipSuccess;
    const size_t want = (n + 255) / 256; // no cap: one lane per set
    if (want > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(line_fits_arith_kernel, dim3((unsigned)want), dim3(256), 0, stream, moments, n, out);
    return hipGetLastError();
}

} // namespace canny
