// canny_hough_circles.hip -- Hough circle detection (cv::HoughCircles(HOUGH_GRADIENT) semantics) on a finished edge map,
// per frame of a batch: every edge pixel votes along its gradient direction for centres min_radius .. max_radius away,
// the accumulator's peaks are the candidate centres, each candidate gets the radius best supported by the map, and an
// ordered pass drops candidates too close to a stronger one.  The rule is part of the interface (include/canny_hip.h,
// DESIGN.md section 18); tests/hough_circles_rule.py restates it in numpy.
//
// Passes, all on one stream, no host round trip:
//   vote    : a workgroup takes 64 plane words (one tile of the strong plane, or 64 words of a packed map), compacts their
//             set pixels into an LDS queue (popcount, prefix, scatter), computes the Sobel pair and the step of every queued
//             pixel with all lanes active, and then votes with all lanes active: the lanes of a wave take consecutive radii
//             of one pixel's two rays (several pixels per wave when the radius range is short).  Votes are integer atomics
//             without return value into a zeroed accumulator; integer adds commute, so the bytes do not depend on the order.
//   centres : the peaks / cut-off / ties / collect / sort kernels of canny_hough.hip on the accumulator read as ah rows of
//             aw cells (launch_hough_peaks, launch_hough_select).
//   radius  : one wave per candidate scans the words of the map that cover the candidate's (2 max_radius + 3)^2 window, bins
//             every set pixel by the integer rule into an LDS histogram and reduces it with cross-multiplied comparisons.
//   accept  : one workgroup per frame walks the candidates in order; each valid one is tested against the accepted list by
//             all lanes at once.
//
// The float contract of a step rests on three operations per component, each rounded to binary32 on its own: the
// conversion of gx^2 + gy^2, the root, the quotient.  sqrtf and / are the correctly rounded expansions here (the tree is
// built without -fno-hip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn / __fdiv_rn of this toolchain are NOT (they map to
// the native instructions unless OCML_BASIC_ROUNDED_OPERATIONS is defined).  tests/test_gpu_hough_circles.py runs the
// device arithmetic on every pair of the Sobel domain.
#include "canny_kernels.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kVoteBlock = 256;                // 4 waves
constexpr int kVoteWords = 64;                 // plane words per chunk: one tile of the strong plane
constexpr int kVoteQueue = kVoteWords * 64;    // every pixel of the chunk set: 32 KiB of 8-byte entries
constexpr int kRadiusBlock = 256;              // 4 candidates, one wave each
constexpr int kAcceptBlock = 1024;

enum { kGradU8 = 0, kGradS16 = 1, kGradPlanes = 2 };

struct GradSrc {
    const void *smoothed;      // u8 or s16 plane of the batch
    const int16_t *gx, *gy;    // or the caller's planes
};

// THE step of the rule.  gx * gx + gy * gy <= 2^31 for s16 inputs: formed in unsigned.  (0, 0) -> (0, 0): no vote.
__device__ __forceinline__ void circle_step(int gx, int gy, int *sx, int *sy)
{
    const unsigned q = (unsigned)(gx * gx) + (unsigned)(gy * gy);
    if (!q) {
        *sx = *sy = 0;
        return;
    }
    const float m = sqrtf((float)q);
    *sx = (int)rintf((float)(gx * 1024) / m);
    *sy = (int)rintf((float)(gy * 1024) / m);
}

struct VoteArgs {
    int min_radius, max_radius, cell_shift, aw, ah;
    int per, shift; // samples per pixel (2 * radii); log2 of the lanes that share one pixel
};

// grid (blocks, n_frames); the accumulators have been zeroed
template <bool BITS, int GRAD>
__global__ __launch_bounds__(kVoteBlock) void circles_vote_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                                  GradSrc grad, VoteArgs a, int *__restrict__ accum)
{
    __shared__ uint64_t s_word[kVoteWords];
    __shared__ int s_y[kVoteWords], s_x0[kVoteWords];
    __shared__ unsigned s_off[kVoteWords], s_total;
    __shared__ uint2 s_queue[kVoteQueue]; // .x: word of the chunk << 6 | bit, .y: sx in the low half, sy in the high half
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = g.height, w = g.width;
    const unsigned units = BITS ? (unsigned)h * g.tiles_x : (unsigned)g.tiles_y * g.tiles_x * 64u;
    const unsigned chunks = (units + kVoteWords - 1) / kVoteWords;
    const size_t frame_px = (size_t)h * w;
    const int stride = a.aw + 2;
    int *acc = accum + (size_t)f * (a.ah + 2) * stride;
    const int nr = a.max_radius - a.min_radius + 1;
    for (unsigned c = blockIdx.x; c < chunks; c += gridDim.x) {
        // the chunk's words, the set pixels before each of them
        if (wave == 0) {
            const unsigned u = c * kVoteWords + lane;
            int y = 0, k = 0;
            if constexpr (BITS) {
                y = (int)(u / (unsigned)g.tiles_x);
                k = (int)(u - (unsigned)y * g.tiles_x);
            } else {
                const unsigned tile = u >> 6;
                const int ty = (int)(tile / (unsigned)g.tiles_x);
                y = (ty << 6) + (int)(u & 63u);
                k = (int)(tile - (unsigned)ty * g.tiles_x);
            }
            const uint64_t v = (u < units && y < h) ? row_word<BITS>(src, g, row_bytes, f, y, k) : 0ull;
            unsigned incl = (unsigned)__popcll(v);
            const unsigned mine = incl;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            s_word[lane] = v;
            s_y[lane] = y;
            s_x0[lane] = k << 6;
            s_off[lane] = incl - mine;
            if (lane == 63) s_total = incl;
        }
        __syncthreads();
        const unsigned total = s_total;
        if (total) { // (workgroup-uniform)
            // scatter: four lanes per word, 16 bits each
            {
                const int wi = tid >> 2, q = tid & 3;
                const uint64_t v = s_word[wi];
                unsigned sub = (unsigned)(v >> (16 * q)) & 0xffffu;
                unsigned at = s_off[wi] + (unsigned)__popcll(v & ((1ull << (16 * q)) - 1ull));
                while (sub) {
                    s_queue[at++].x = (unsigned)(wi << 6) | (unsigned)(16 * q + __builtin_ctz(sub));
                    sub &= sub - 1;
                }
            }
            __syncthreads();
            // gradient and step of every queued pixel
            for (unsigned i = tid; i < total; i += kVoteBlock) {
                const unsigned pos = s_queue[i].x;
                const int wi = (int)(pos >> 6), x = s_x0[wi] + (int)(pos & 63u), y = s_y[wi];
                int gx, gy;
                if constexpr (GRAD == kGradU8)
                    sobel_pair((const uint8_t *)grad.smoothed + (size_t)f * frame_px, h, w, y, x, &gx, &gy);
                else if constexpr (GRAD == kGradS16)
                    sobel_pair((const int16_t *)grad.smoothed + (size_t)f * frame_px, h, w, y, x, &gx, &gy);
                else {
                    const size_t p = (size_t)f * frame_px + (size_t)y * w + x;
                    gx = grad.gx[p];
                    gy = grad.gy[p];
                }
                int sx, sy;
                circle_step(gx, gy, &sx, &sy);
                s_queue[i].y = ((unsigned)sx & 0xffffu) | ((unsigned)sy << 16);
            }
            __syncthreads();
            // votes: 64 >> shift pixels per wave step, 1 << shift lanes per pixel
            const int group = 64 >> a.shift, lanes = 1 << a.shift;
            for (unsigned e0 = (unsigned)(wave * group); e0 < total; e0 += 4u * group) {
                const unsigned e = e0 + (unsigned)(lane >> a.shift);
                if (e >= total) continue;
                const uint2 q = s_queue[e];
                if (!q.y) continue; // zero gradient: no vote
                const int wi = (int)(q.x >> 6), x = s_x0[wi] + (int)(q.x & 63u), y = s_y[wi];
                const int sx = (int)(short)(q.y & 0xffffu), sy = (int)q.y >> 16;
                for (int j = lane & (lanes - 1); j < a.per; j += lanes) {
                    const bool neg = j >= nr;
                    const int k = a.min_radius + (neg ? j - nr : j);
                    const int dx = neg ? -k * sx : k * sx, dy = neg ? -k * sy : k * sy;
                    // X = x * 1024 + dx and x * 1024 is a multiple of 1024: X >> 10 = x + (dx >> 10), without overflow
                    const int px = x + (dx >> 10), py = y + (dy >> 10);
                    if ((unsigned)px < (unsigned)w && (unsigned)py < (unsigned)h)
                        atomicAdd(&acc[(size_t)((py >> a.cell_shift) + 1) * stride + (px >> a.cell_shift) + 1], 1);
                }
            }
        }
        __syncthreads(); // the chunk's words and queue are overwritten next
    }
}

__global__ __launch_bounds__(256) void circles_steps_kernel(const int16_t *__restrict__ gx, const int16_t *__restrict__ gy,
                                                            size_t n, int *__restrict__ sx, int *__restrict__ sy)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        circle_step(gx[i], gy[i], &sx[i], &sy[i]);
}

// floor(sqrt(d)) for 0 <= d < 2^24 (exact as a float; the correction absorbs the root's rounding)
__device__ __forceinline__ int isqrt24(int d)
{
    int s = (int)sqrtf((float)d);
    if (s * s > d) s--;
    if ((s + 1) * (s + 1) <= d) s++;
    return s;
}

// (count a, radius ra) beats (count b, radius rb): a / ra > b / rb, the smaller radius on a tie.  counts < 2^31, radii <=
// 1024: the products stay below 2^41.
__device__ __forceinline__ bool radius_beats(unsigned a, int ra, unsigned b, int rb)
{
    const unsigned long long l = (unsigned long long)a * (unsigned)rb, r = (unsigned long long)b * (unsigned)ra;
    return l > r || (l == r && ra < rb);
}

// grid (ceil(centres_max / 4), n_frames); dynamic LDS 4 * radii counters.  Candidate k of frame f: bases[f * centres_max + k].
template <bool BITS>
__global__ __launch_bounds__(kRadiusBlock) void circles_radius_kernel(const void *__restrict__ src, HystGeom g,
                                                                      int row_bytes, const unsigned *__restrict__ bases,
                                                                      const int *__restrict__ peak_counts, int centres_max,
                                                                      int min_radius, int max_radius, int cell_shift,
                                                                      int aw, int *__restrict__ radius,
                                                                      int *__restrict__ support)
{
    extern __shared__ unsigned s_hist[];
    const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nr = max_radius - min_radius + 1;
    unsigned *hist = s_hist + wave * nr;
    const int k = blockIdx.x * 4 + wave;
    const bool active = k < min(centres_max, peak_counts[f]);
    for (int i = lane; i < nr; i += 64) hist[i] = 0;
    __syncthreads();
    if (active) {
        const unsigned base = bases[(size_t)f * centres_max + k];
        const int ay = (int)(base / (unsigned)(aw + 2)) - 1, ax = (int)(base % (unsigned)(aw + 2)) - 1;
        const int c = 1 << cell_shift, x2 = (2 * ax + 1) * c, y2 = (2 * ay + 1) * c;
        // |2y - y2| <= 2 max_radius for a pixel of any bin up to max_radius; one more row / column each way for safety
        const int ylo = max(0, (y2 - 2 * max_radius - 2) >> 1), yhi = min(g.height - 1, (y2 + 2 * max_radius + 2) >> 1);
        const int xlo = max(0, (x2 - 2 * max_radius - 2) >> 1), xhi = min(g.width - 1, (x2 + 2 * max_radius + 2) >> 1);
        const int wlo = xlo >> 6, nw = (xhi >> 6) - wlo + 1;
        const int lo2 = (2 * min_radius - 1) * (2 * min_radius - 1), hi2 = (2 * max_radius + 1) * (2 * max_radius + 1);
        const int total = (yhi - ylo + 1) * nw; // <= 2052 rows * 34 words
        for (int i = lane; i < total; i += 64) {
            const int y = ylo + i / nw, kw = wlo + i % nw;
            uint64_t v = row_word<BITS>(src, g, row_bytes, f, y, kw);
            const int dy = 2 * y - y2;
            while (v) {
                const int x = (kw << 6) + (int)__builtin_ctzll(v);
                v &= v - 1;
                const int dx = 2 * x - x2;       // the word reaches up to 63 columns past the window: |dx| < 2300
                const int d = dx * dx + dy * dy; // no overflow; inside a bin of the range it is below 2^24
                if (d < lo2 || d >= hi2) continue;
                atomicAdd(&hist[((isqrt24(d) + 1) >> 1) - min_radius], 1u);
            }
        }
    }
    __syncthreads();
    if (active) {
        unsigned best = hist[0];
        int best_r = min_radius;
        for (int i = lane; i < nr; i += 64) { // ascending radii: only a strictly better quotient replaces
            const unsigned cnt = hist[i];
            if (radius_beats(cnt, min_radius + i, best, best_r)) best = cnt, best_r = min_radius + i;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned ob = __shfl_xor(best, d);
            const int orr = __shfl_xor(best_r, d);
            if (radius_beats(ob, orr, best, best_r)) best = ob, best_r = orr;
        }
        if (lane == 0) {
            radius[(size_t)f * centres_max + k] = best_r;
            support[(size_t)f * centres_max + k] = (int)best;
        }
    }
}

// one workgroup per frame; the candidates in order, each valid one against the accepted list
__global__ __launch_bounds__(kAcceptBlock) void circles_accept_kernel(const unsigned *__restrict__ bases,
                                                                      const int *__restrict__ votes,
                                                                      const int *__restrict__ radius,
                                                                      const int *__restrict__ support,
                                                                      const int *__restrict__ peak_counts, int centres_max,
                                                                      int cell_shift, int aw, int support_threshold,
                                                                      unsigned long long min_dist2_4,
                                                                      int *__restrict__ circles, int *__restrict__ counts)
{
    __shared__ int s_x2[kHoughMaxLines], s_y2[kHoughMaxLines]; // candidates first; then, in place, the accepted ones
    __shared__ unsigned short s_from[kHoughMaxLines];          // candidate index of the j-th accepted
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int K = min(centres_max, peak_counts[f]);
    const size_t at = (size_t)f * centres_max;
    const int c = 1 << cell_shift;
    for (int k = tid; k < K; k += kAcceptBlock) {
        const unsigned base = bases[at + k];
        s_x2[k] = (2 * ((int)(base % (unsigned)(aw + 2)) - 1) + 1) * c;
        s_y2[k] = (2 * ((int)(base / (unsigned)(aw + 2)) - 1) + 1) * c;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    // accepted entry j <= its candidate index, so writing it at j never overwrites a candidate still to come
    for (int k = 0; k < K; k++) {
        if (support[at + k] <= support_threshold) continue; // (workgroup-uniform)
        const int n = s_n, x2 = s_x2[k], y2 = s_y2[k];
        int near = 0;
        if (min_dist2_4)
            for (int j = tid; j < n; j += kAcceptBlock) {
                const long long dx = (long long)x2 - s_x2[j], dy = (long long)y2 - s_y2[j];
                near |= (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy) < min_dist2_4;
            }
        const int any = __syncthreads_or(near); // also: every lane has read s_n, s_x2[k], s_y2[k]
        if (!any && tid == 0) {
            s_x2[n] = x2;
            s_y2[n] = y2;
            s_from[n] = (unsigned short)k;
            s_n = n + 1;
        }
        __syncthreads();
    }
    const int n = s_n;
    if (circles)
        for (int j = tid; j < n; j += kAcceptBlock) {
            const int k = s_from[j];
            int *rec = circles + (at + j) * 6;
            rec[0] = s_x2[j];
            rec[1] = s_y2[j];
            rec[2] = radius[at + k];
            rec[3] = votes[at + k];
            rec[4] = support[at + k];
            rec[5] = (int)bases[at + k];
        }
    if (tid == 0) counts[f] = n;
}

template <bool BITS, int GRAD>
hipError_t vote(const void *src, const HystGeom &g, const GradSrc &grad, const VoteArgs &a, int *accum, hipStream_t stream)
{
    const dim3 grid(plan_circles_vote(g, BITS).grid, g.n_frames);
    hipLaunchKernelGGL((circles_vote_kernel<BITS, GRAD>), grid, dim3(kVoteBlock), 0, stream, src, g, (g.width + 7) / 8,
                       grad, a, accum);
    return hipGetLastError();
}

} // namespace

LaunchPlan plan_circles_vote(const HystGeom &g, bool from_bits)
{
    const unsigned long long words =
        from_bits ? (unsigned long long)g.height * g.tiles_x : (unsigned long long)g.tiles_y * g.tiles_x * 64;
    return capped_plan((words + kVoteWords - 1) / kVoteWords, 1, 2048);
}
LaunchPlan plan_circles_steps(size_t n) { return capped_plan(n, 256, 8192); }

hipError_t launch_circles_vote(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const void *smoothed,
                               bool smoothed_u8, const int16_t *gx, const int16_t *gy, const CircleGeom &cg, int *accum,
                               hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(accum, 0, circles_accum_bytes(cg, g.n_frames), stream);
    if (e != hipSuccess) return e;
    VoteArgs a;
    a.min_radius = cg.min_radius, a.max_radius = cg.max_radius, a.cell_shift = cg.cell_shift, a.aw = cg.aw, a.ah = cg.ah;
    a.per = 2 * (cg.max_radius - cg.min_radius + 1);
    a.shift = 0;
    while (a.shift < 6 && (1 << a.shift) < a.per) a.shift++;
    const GradSrc grad{smoothed, gx, gy};
    if (bits) return vote<true, kGradPlanes>(bits, g, grad, a, accum, stream);
    return smoothed_u8 ? vote<false, kGradU8>(strong, g, grad, a, accum, stream)
                       : vote<false, kGradS16>(strong, g, grad, a, accum, stream);
}

hipError_t launch_circles_steps(const int16_t *gx, const int16_t *gy, size_t n, int *sx, int *sy, hipStream_t stream)
{
    hipLaunchKernelGGL(circles_steps_kernel, dim3(plan_circles_steps(n).grid), dim3(256), 0, stream, gx, gy, n, sx, sy);
    return hipGetLastError();
}

hipError_t launch_circles_radius(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const CircleGeom &cg,
                                 const unsigned *bases, const int *peak_counts, int centres_max, int *radius, int *support,
                                 hipStream_t stream)
{
    const size_t lds = 4 * (size_t)(cg.max_radius - cg.min_radius + 1) * sizeof(unsigned); // <= 16 KiB
    const dim3 grid((centres_max + 3) / 4, g.n_frames);
    if (bits)
        hipLaunchKernelGGL(circles_radius_kernel<true>, grid, dim3(kRadiusBlock), lds, stream, (const void *)bits, g,
                           (g.width + 7) / 8, bases, peak_counts, centres_max, cg.min_radius, cg.max_radius, cg.cell_shift,
                           cg.aw, radius, support);
    else
        hipLaunchKernelGGL(circles_radius_kernel<false>, grid, dim3(kRadiusBlock), lds, stream, (const void *)strong, g,
                           (g.width + 7) / 8, bases, peak_counts, centres_max, cg.min_radius, cg.max_radius, cg.cell_shift,
                           cg.aw, radius, support);
    return hipGetLastError();
}

hipError_t launch_circles_accept(const HystGeom &g, const CircleGeom &cg, const unsigned *bases, const int *votes,
                                 const int *radius, const int *support, const int *peak_counts, int centres_max,
                                 int support_threshold, int min_dist, int *circles, int *counts, hipStream_t stream)
{
    if (centres_max > kHoughMaxLines) return hipErrorInvalidValue;
    const unsigned long long md = 2ull * (unsigned long long)min_dist; // < 2^32: the square fits
    hipLaunchKernelGGL(circles_accept_kernel, dim3(g.n_frames), dim3(kAcceptBlock), 0, stream, bases, votes, radius, support,
                       peak_counts, centres_max, cg.cell_shift, cg.aw, support_threshold, md * md, circles, counts);
    return hipGetLastError();
}

} // namespace canny
