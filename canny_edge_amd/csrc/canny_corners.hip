// canny_corners.hip -- corners (Harris / Shi-Tomasi) of the smoothed plane, per frame of a batch: a structure-tensor
// response at every pixel, its local maxima over a quality threshold, and an ordered, distance-suppressed list of corners.
// The rule is part of the interface (include/canny_hip.h); tests/corners_rule.py restates it in numpy
// and Python ints, canny_corners_host.cpp in plain C++.
//
// The response plane is not kept in memory (16 B/px stored and read back): every pass computes it again from the plane
// (1 B/px) with ONE tile routine, corner_tile.  Passes, all on one stream, no host round trip, the launch sequence a
// function of shapes and arguments alone:
//   max        : R of every pixel of a 64 x 16 tile; the frame's maximum by a wave reduction and one 64-bit atomicMax per
//                workgroup (a maximum does not depend on order); the response plane if the caller asks for it.
//   candidates : R again on each tile plus a one-pixel ring, the threshold, the eight-neighbour test.  key = (2^60 - 1 - R)
//                << 31 | base: 91 bits, unique, ascending in the rule's order.  The corners_max smallest keys of a frame are
//                found by a radix select: up to seven passes, each a histogram of one 13-bit digit of the keys that share
//                the prefix chosen so far (integer atomics into a zeroed histogram: counts commute) and a one-workgroup
//                choice of the digit in which the corners_max-th key lies.  A frame with no more candidates than
//                corners_max is finished after the first pass, and its later passes return at once.  The first pass also
//                lists the keys (16384 a frame at most): a frame whose keys all fit takes its later passes and the collect
//                over that list (corners_list_kernel), and only a frame with more computes the responses again in every
//                pass.  Same histograms, same slots, same bytes either way.
//   collect    : the same kernel once more stores every key <= the cut-off through an atomic slot counter -- the slots'
//                order is arbitrary, and does not reach the output:
//   accept     : one workgroup per frame sorts the collected keys (bitonic, LDS; the keys are distinct) and walks them in
//                order, each against the accepted list by all lanes at once, the pattern of the chamfer matches.
//
// corner_tile, for a tile of TX x TY pixels with a ring of RING pixels: (1) the Sobel pair (sobel_pair of canny_kernels.h,
// the one copy, with the frame's border rules) once per pixel of the tile + ring + r, its three products into LDS, zero
// outside the frame; (2) the horizontal box sums into LDS; (3) the vertical box sums in registers and the response, as 64
// bits, into LDS over the dead products.  The three sums stay in int; only the response is 64 bits wide.
#include "canny_kernels.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTileX = 64, kTileY = 16;
constexpr int kDigitBins = 8192;
constexpr int kAcceptBlock = 1024;
constexpr int kPasses = 7; // 7 x 13 = 91 bits
constexpr int kDigit = 13;
constexpr long long kOutside = (long long)0x8000000000000000ull; // a neighbour outside the frame: below every R
typedef unsigned __int128 Key;

// ceil(sqrt(v)) for v < 2^54: the double root is within one of the integer root; one correction step each way in 64 bits
__device__ __forceinline__ long long ceil_sqrt54(unsigned long long v)
{
    unsigned long long s = (unsigned long long)sqrt((double)v);
    if (s * s > v) s--;
    if ((s + 1) * (s + 1) <= v) s++;
    return (long long)(s + (s * s < v));
}

// THE response of the rule
__device__ __forceinline__ long long corner_response(int sxx, int syy, int sxy, int mode, int k_q8)
{
    const long long a = sxx, b = syy, c = sxy;
    if (mode == 0) {
        const long long d = a - b;
        return a + b - ceil_sqrt54((unsigned long long)(d * d) + 4ull * (unsigned long long)(c * c));
    }
    const long long tr = a + b;
    return 256 * (a * b - c * c) - (long long)k_q8 * tr * tr;
}

template <int BLOCK, int RING>
struct TileGeom {
    static constexpr int R = BLOCK / 2;
    static constexpr int RW = kTileX + 2 * RING, RH = kTileY + 2 * RING; // responses
    static constexpr int PW = RW + 2 * R, PH = RH + 2 * R;               // products
    static constexpr int kProdInts = 3 * PW * PH, kSumInts = 3 * RW * PH;
    static constexpr int kLdsInts = kProdInts + kSumInts;
    static_assert(RW * RH * 2 <= kProdInts, "the responses take the products' place");
};

// Responses of the tile at (y0, x0) of frame `img` with its ring, into s_resp[RH][RW] (= lds); kOutside outside the frame.
// All lanes of the workgroup; ends with a barrier, and begins with one (the previous tile's responses have been read).
template <class T, int BLOCK, int RING>
__device__ __forceinline__ void corner_tile(const T *__restrict__ img, int h, int w, int y0, int x0, int mode, int k_q8,
                                            int *lds)
{
    typedef TileGeom<BLOCK, RING> G;
    int *s_prod = lds, *s_sum = lds + G::kProdInts;
    long long *s_resp = (long long *)lds;
    const int tid = threadIdx.x;
    __syncthreads();
    for (int i = tid; i < G::PW * G::PH; i += kBlock) {
        const int py = i / G::PW, px = i - py * G::PW;
        const int y = y0 - RING - G::R + py, x = x0 - RING - G::R + px;
        int gx = 0, gy = 0;
        if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) sobel_pair(img, h, w, y, x, &gx, &gy);
        s_prod[i] = gx * gx;
        s_prod[G::PW * G::PH + i] = gy * gy;
        s_prod[2 * G::PW * G::PH + i] = gx * gy;
    }
    __syncthreads();
    for (int i = tid; i < G::RW * G::PH; i += kBlock) {
        const int py = i / G::RW, px = i - py * G::RW;
        const int *p = s_prod + py * G::PW + px;
        int a = 0, b = 0, c = 0;
#pragma unroll
        for (int k = 0; k < BLOCK; k++) {
            a += p[k];
            b += p[G::PW * G::PH + k];
            c += p[2 * G::PW * G::PH + k];
        }
        s_sum[i] = a;
        s_sum[G::RW * G::PH + i] = b;
        s_sum[2 * G::RW * G::PH + i] = c;
    }
    __syncthreads();
    for (int i = tid; i < G::RW * G::RH; i += kBlock) {
        const int ry = i / G::RW, rx = i - ry * G::RW;
        const int y = y0 - RING + ry, x = x0 - RING + rx;
        long long resp = kOutside;
        if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
            const int *p = s_sum + ry * G::RW + rx;
            int a = 0, b = 0, c = 0;
#pragma unroll
            for (int k = 0; k < BLOCK; k++) {
                a += p[k * G::RW];
                b += p[G::RW * G::PH + k * G::RW];
                c += p[2 * G::RW * G::PH + k * G::RW];
            }
            resp = corner_response(a, b, c, mode, k_q8);
        }
        s_resp[i] = resp;
    }
    __syncthreads();
}

// a maximum as an unsigned word that a zeroed cell lies below
__device__ __forceinline__ unsigned long long bias(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ long long unbias(unsigned long long v) { return (long long)(v ^ 0x8000000000000000ull); }

// grid (plan_corners_tiles, frames).  rmax: one biased word per frame, zeroed beforehand.
template <class T, int BLOCK>
__global__ __launch_bounds__(kBlock) void corners_max_kernel(const T *__restrict__ plane, int h, int w, int tiles_x,
                                                             unsigned tiles, int mode, int k_q8,
                                                             unsigned long long *__restrict__ rmax,
                                                             long long *__restrict__ response)
{
    typedef TileGeom<BLOCK, 0> G;
    __shared__ int lds[G::kLdsInts];
    __shared__ unsigned long long s_wave[kBlock / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    const size_t hw = (size_t)h * w;
    const T *img = plane + (size_t)f * hw;
    const long long *s_resp = (const long long *)lds;
    unsigned long long best = 0; // below every biased response
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty = (int)(t / (unsigned)tiles_x), tx = (int)(t - (unsigned)ty * tiles_x);
        const int y0 = ty * kTileY, x0 = tx * kTileX;
        corner_tile<T, BLOCK, 0>(img, h, w, y0, x0, mode, k_q8, lds);
        for (int i = tid; i < kTileX * kTileY; i += kBlock) {
            const int y = y0 + i / kTileX, x = x0 + (i & (kTileX - 1));
            if (y < h && x < w) {
                const long long v = s_resp[i];
                best = max(best, bias(v));
                if (response) response[(size_t)f * hw + (size_t)y * w + x] = v;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, d));
    if ((tid & 63) == 0) s_wave[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kBlock / 64; k++) best = max(best, s_wave[k]);
        atomicMax(&rmax[f], best);
    }
}

struct CornerWs {
    Key *keys, *list, *prefix, *cutoff;
    unsigned long long *rmax;
    unsigned *hist, *need, *flag, *total, *n_emit, *n_list;
};

// One candidate key in a digit pass (its digit into the histogram, if it shares the prefix) or in the collect pass (into
// a slot, if it is not beyond the cut-off).
__device__ __forceinline__ void take_key(Key key, bool collect, int pass, int shift, Key prefix, Key cutoff, int f,
                                         unsigned corners_max, const CornerWs &ws)
{
    if (collect) {
        if (key > cutoff) return;
        const unsigned slot = atomicAdd(&ws.n_emit[f], 1u);
        if (slot < corners_max) ws.keys[(size_t)f * corners_max + slot] = key;
    } else {
        if (pass > 0 && (key >> (shift + kDigit)) != prefix) return;
        atomicAdd(&ws.hist[(size_t)f * kDigitBins + ((unsigned)(key >> shift) & (kDigitBins - 1))], 1u);
    }
}

// max(thr, min_response, 1) of a frame whose maximum is rmax
__device__ __forceinline__ long long corner_cut(long long rmax, unsigned q16, long long min_response)
{
    const unsigned long long m = rmax > 0 ? (unsigned long long)rmax : 0ull;
    const long long thr = (long long)((m >> 16) * q16 + (((m & 0xffffull) * q16) >> 16));
    return max(max(thr, min_response), 1ll);
}

// grid (plan_corners_tiles, frames).  pass 0..6: the digit of every candidate that shares the prefix; pass 7: collect.
template <class T, int BLOCK>
__global__ __launch_bounds__(kBlock) void corners_cand_kernel(const T *__restrict__ plane, int h, int w, int tiles_x,
                                                              unsigned tiles, int mode, int k_q8, unsigned q16,
                                                              long long min_response, int pass, unsigned corners_max,
                                                              unsigned list_cap, CornerWs ws)
{
    typedef TileGeom<BLOCK, 1> G;
    __shared__ int lds[G::kLdsInts];
    const int f = blockIdx.y, tid = threadIdx.x;
    const bool collect = pass == kPasses;
    if (collect ? !ws.total[f] : (pass > 0 && ws.flag[f])) return; // (workgroup-uniform)
    if (pass > 0 && ws.total[f] <= list_cap) return;               // pass 0 listed every key: corners_list_kernel's frame
    const long long rmax = unbias(ws.rmax[f]);
    const long long cut = corner_cut(rmax, q16, min_response);
    if (rmax < cut) return; // no pixel reaches the threshold
    const Key prefix = (!collect && pass > 0) ? ws.prefix[f] : (Key)0;
    const Key cutoff = collect ? ws.cutoff[f] : (Key)0;
    const int shift = collect ? 0 : kDigit * (kPasses - 1 - pass);
    const T *img = plane + (size_t)f * ((size_t)h * w);
    const long long *s_resp = (const long long *)lds;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty = (int)(t / (unsigned)tiles_x), tx = (int)(t - (unsigned)ty * tiles_x);
        const int y0 = ty * kTileY, x0 = tx * kTileX;
        corner_tile<T, BLOCK, 1>(img, h, w, y0, x0, mode, k_q8, lds);
        for (int i = tid; i < kTileX * kTileY; i += kBlock) {
            const int ly = i / kTileX, lx = i & (kTileX - 1);
            const int y = y0 + ly, x = x0 + lx;
            if (y >= h || x >= w) continue;
            const long long *c = s_resp + (ly + 1) * G::RW + lx + 1;
            const long long v = c[0];
            if (v < cut) continue;
            // a neighbour outside the frame holds kOutside: both tests pass
            if (!(v > c[-G::RW - 1] && v > c[-G::RW] && v > c[-G::RW + 1] && v > c[-1])) continue;
            if (!(v >= c[1] && v >= c[G::RW - 1] && v >= c[G::RW] && v >= c[G::RW + 1])) continue;
            const unsigned base = (unsigned)y * (unsigned)w + (unsigned)x;
            const Key key = (Key)((1ull << 60) - 1ull - (unsigned long long)v) << 31 | base;
            if (pass == 0) { // the first pass also lists the keys, in arbitrary order, as far as the list goes
                const unsigned slot = atomicAdd(&ws.n_list[f], 1u);
                if (slot < list_cap) ws.list[(size_t)f * list_cap + slot] = key;
            }
            take_key(key, collect, pass, shift, prefix, cutoff, f, corners_max, ws);
        }
    }
}

// grid (ceil(list_cap / 256), frames): pass 1..6 and collect for the frames whose keys pass 0 listed in full -- the same
// histogram and the same slots as corners_cand_kernel would fill, without computing a response.
__global__ __launch_bounds__(kBlock) void corners_list_kernel(int pass, unsigned corners_max, unsigned list_cap, CornerWs ws)
{
    const int f = blockIdx.y;
    const bool collect = pass == kPasses;
    const unsigned total = ws.total[f];
    if (!total || total > list_cap || (!collect && ws.flag[f])) return;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const Key prefix = collect ? (Key)0 : ws.prefix[f];
    const Key cutoff = collect ? ws.cutoff[f] : (Key)0;
    const int shift = collect ? 0 : kDigit * (kPasses - 1 - pass);
    take_key(ws.list[(size_t)f * list_cap + i], collect, pass, shift, prefix, cutoff, f, corners_max, ws);
}

// grid (frames), one workgroup: the digit in which the need-th smallest key lies; the histogram is zeroed for the next pass.
__global__ __launch_bounds__(kAcceptBlock) void corners_choose_kernel(int pass, unsigned corners_max, CornerWs ws,
                                                                      int *__restrict__ cand_counts,
                                                                      long long *__restrict__ max_response)
{
    __shared__ unsigned s_sum[kAcceptBlock];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (pass > 0 && ws.flag[f]) return; // (workgroup-uniform)
    unsigned *hist = ws.hist + (size_t)f * kDigitBins;
    unsigned need = pass > 0 ? ws.need[f] : corners_max;
    const Key prefix = pass > 0 ? ws.prefix[f] : (Key)0;
    unsigned v[8], local = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        v[j] = hist[tid * 8 + j];
        hist[tid * 8 + j] = 0;
        local += v[j];
    }
    s_sum[tid] = local;
    __syncthreads();
    for (int d = 1; d < kAcceptBlock; d <<= 1) {
        const unsigned add = tid >= d ? s_sum[tid - d] : 0u;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    const unsigned incl = s_sum[tid], excl = incl - local, total = s_sum[kAcceptBlock - 1];
    if (pass == 0) {
        if (tid == 0) {
            ws.total[f] = total;
            if (cand_counts) cand_counts[f] = (int)total;
            if (max_response) max_response[f] = unbias(ws.rmax[f]);
        }
        if (total <= need) { // every candidate goes on (workgroup-uniform)
            if (tid == 0) {
                ws.flag[f] = 1u;
                ws.cutoff[f] = ~(Key)0;
            }
            return;
        }
    }
    if (excl < need && need <= incl) {
        unsigned run = excl;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (run + v[j] >= need) {
                const Key np = prefix << kDigit | (unsigned)(tid * 8 + j);
                ws.prefix[f] = np;
                ws.need[f] = need - run;
                if (pass == kPasses - 1) ws.cutoff[f] = np;
                break;
            }
            run += v[j];
        }
    }
}

// one workgroup per frame: sort the collected keys, then the candidates in order, each against the accepted list
__global__ __launch_bounds__(kAcceptBlock) void corners_accept_kernel(int w, unsigned corners_max,
                                                                      unsigned long long min_dist2, CornerWs ws,
                                                                      long long *__restrict__ corners,
                                                                      int *__restrict__ counts)
{
    __shared__ unsigned long long s_hi[kHoughMaxLines]; // 2^60 - 1 - R of the sorted candidates; then, in place, of the accepted
    __shared__ unsigned s_base[kHoughMaxLines];
    __shared__ unsigned short s_rank[kHoughMaxLines]; // of the accepted
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    const unsigned M = min(corners_max, ws.total[f]);
    unsigned P = 1;
    while (P < M) P <<= 1;
    for (unsigned i = tid; i < P; i += kAcceptBlock) {
        const Key k = i < M ? ws.keys[(size_t)f * corners_max + i] : ~(Key)0;
        s_hi[i] = (unsigned long long)(k >> 31);
        s_base[i] = (unsigned)k & 0x7fffffffu;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (unsigned size = 2; size <= P; size <<= 1)
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < P; i += kAcceptBlock) {
                const unsigned j = i ^ stride;
                if (j > i) {
                    const unsigned long long ah = s_hi[i], bh = s_hi[j];
                    const unsigned ab = s_base[i], bb = s_base[j];
                    const bool gt = ah > bh || (ah == bh && ab > bb);
                    if (gt == ((i & size) == 0)) s_hi[i] = bh, s_hi[j] = ah, s_base[i] = bb, s_base[j] = ab;
                }
            }
            __syncthreads();
        }
    // accepted entry j <= its candidate index, so writing it at j never overwrites a candidate still to come
    for (unsigned c = 0; c < M; c++) {
        const unsigned long long hi = s_hi[c];
        const unsigned base = s_base[c];
        const int y = (int)(base / (unsigned)w), x = (int)(base - (unsigned)y * (unsigned)w);
        const int n = s_n;
        int near = 0;
        if (min_dist2)
            for (int j = tid; j < n; j += kAcceptBlock) {
                const unsigned bj = s_base[j];
                const int yj = (int)(bj / (unsigned)w), xj = (int)(bj - (unsigned)yj * (unsigned)w);
                const long long dx = (long long)x - xj, dy = (long long)y - yj;
                near |= (unsigned long long)(dx * dx + dy * dy) < min_dist2;
            }
        const int any = __syncthreads_or(near); // also: every lane has read s_n and the candidate
        if (!any && tid == 0) {
            s_hi[n] = hi;
            s_base[n] = base;
            s_rank[n] = (unsigned short)c;
            s_n = n + 1;
        }
        __syncthreads();
    }
    const int n = s_n;
    for (int j = tid; j < n; j += kAcceptBlock) {
        const unsigned base = s_base[j];
        const unsigned y = base / (unsigned)w;
        long long *rec = corners + ((size_t)f * corners_max + j) * 4;
        rec[0] = (long long)(base - y * (unsigned)w);
        rec[1] = (long long)y;
        rec[2] = (long long)((1ull << 60) - 1ull - s_hi[j]);
        rec[3] = (long long)s_rank[j];
    }
    if (tid == 0) counts[f] = n;
}

__global__ __launch_bounds__(kBlock) void corners_arith_kernel(const int *__restrict__ sums, size_t n, int mode, int k_q8,
                                                               long long *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
        out[i] = corner_response(sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], mode, k_q8);
}

CornerWs carve(void *ws, int nf, int corners_max, unsigned list_cap)
{
    CornerWs c;
    c.keys = (Key *)ws;
    c.list = c.keys + (size_t)nf * corners_max;
    c.prefix = c.list + (size_t)nf * list_cap;
    c.cutoff = c.prefix + nf;
    c.rmax = (unsigned long long *)(c.cutoff + nf);
    c.hist = (unsigned *)(c.rmax + nf);
    c.need = c.hist + (size_t)nf * kDigitBins;
    c.flag = c.need + nf;
    c.total = c.flag + nf;
    c.n_emit = c.total + nf;
    c.n_list = c.n_emit + nf;
    return c;
}

// the bytes from rmax on: what a call zeroes
size_t zeroed_bytes(int nf) { return (size_t)nf * 8 + ((size_t)nf * kDigitBins + 5 * (size_t)nf) * sizeof(unsigned); }

// Keys of a frame that pass 0 lists: every candidate of a small frame (no two candidates are neighbours, so a frame holds
// at most ceil(h / 2) * ceil(w / 2)), 16384 otherwise -- a frame with more takes every pass over the plane.
unsigned list_cap_of(int height, int width)
{
    const unsigned long long most = (unsigned long long)((height + 1) / 2) * (unsigned long long)((width + 1) / 2);
    return (unsigned)std::min<unsigned long long>(most, 16384);
}

template <class T, int BLOCK>
void launch_max_t(const T *plane, int nf, int h, int w, int mode, int k_q8, const CornerWs &c, long long *response,
                  hipStream_t stream)
{
    const int tiles_x = (w + kTileX - 1) / kTileX;
    const LaunchPlan p = plan_corners_tiles(h, w);
    hipLaunchKernelGGL((corners_max_kernel<T, BLOCK>), dim3(p.grid, nf), dim3(kBlock), 0, stream, plane, h, w, tiles_x,
                       (unsigned)p.units, mode, k_q8, c.rmax, response);
}

template <class T, int BLOCK>
void launch_cand_t(const T *plane, int nf, int h, int w, const CornerArgs &a, int pass, const CornerWs &c,
                   hipStream_t stream)
{
    const int tiles_x = (w + kTileX - 1) / kTileX;
    const LaunchPlan p = plan_corners_tiles(h, w);
    hipLaunchKernelGGL((corners_cand_kernel<T, BLOCK>), dim3(p.grid, nf), dim3(kBlock), 0, stream, plane, h, w, tiles_x,
                       (unsigned)p.units, a.mode, a.k_q8, (unsigned)a.quality_q16, a.min_response, pass,
                       (unsigned)a.corners_max, list_cap_of(h, w), c);
}

template <class T>
void launch_cand(const T *plane, int nf, int h, int w, const CornerArgs &a, int pass, const CornerWs &c, hipStream_t stream)
{
    if (pass > 0) {
        const unsigned cap = list_cap_of(h, w);
        hipLaunchKernelGGL(corners_list_kernel, dim3((cap + kBlock - 1) / kBlock, nf), dim3(kBlock), 0, stream, pass,
                           (unsigned)a.corners_max, cap, c);
    }
    if (a.block == 3) launch_cand_t<T, 3>(plane, nf, h, w, a, pass, c, stream);
    else if (a.block == 5) launch_cand_t<T, 5>(plane, nf, h, w, a, pass, c, stream);
    else launch_cand_t<T, 7>(plane, nf, h, w, a, pass, c, stream);
}

bool bad_args(const CornerArgs &a, int nf)
{
    return (a.block != 3 && a.block != 5 && a.block != 7) || a.corners_max < 1 || a.corners_max > kHoughMaxLines || nf < 1 ||
           nf > kCornersChunk;
}

} // namespace

LaunchPlan plan_corners_tiles(int height, int width)
{
    const unsigned long long tiles =
        (unsigned long long)((width + kTileX - 1) / kTileX) * (unsigned long long)((height + kTileY - 1) / kTileY);
    return capped_plan(tiles, 1, 1024);
}
LaunchPlan plan_corners_arith(size_t n) { return capped_plan(n, kBlock, 1024); }

size_t corners_ws_bytes(int nf, int corners_max, int height, int width)
{
    return ((size_t)nf * corners_max + (size_t)nf * list_cap_of(height, width) + 2 * (size_t)nf) * sizeof(Key) +
           zeroed_bytes(nf);
}

hipError_t launch_corners_max(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a, void *ws,
                              long long *response, hipStream_t stream)
{
    if (bad_args(a, nf)) return hipErrorInvalidValue;
    const CornerWs c = carve(ws, nf, a.corners_max, list_cap_of(height, width));
    // the maxima, histogram, need, flag, total, the collect and the list counters start from zero; keys, list, prefix
    // and cutoff are written before they are read
    hipError_t e = hipMemsetAsync(c.rmax, 0, zeroed_bytes(nf), stream);
    if (e != hipSuccess) return e;
#define CORNERS_MAX_CASE(T, B) launch_max_t<T, B>((const T *)plane, nf, height, width, a.mode, a.k_q8, c, response, stream)
    if (plane_u8) {
        if (a.block == 3) CORNERS_MAX_CASE(uint8_t, 3);
        else if (a.block == 5) CORNERS_MAX_CASE(uint8_t, 5);
        else CORNERS_MAX_CASE(uint8_t, 7);
    } else {
        if (a.block == 3) CORNERS_MAX_CASE(int16_t, 3);
        else if (a.block == 5) CORNERS_MAX_CASE(int16_t, 5);
        else CORNERS_MAX_CASE(int16_t, 7);
    }
#undef CORNERS_MAX_CASE
    return hipGetLastError();
}

hipError_t launch_corners_candidates(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a,
                                     void *ws, int *cand_counts, long long *max_response, hipStream_t stream)
{
    if (bad_args(a, nf)) return hipErrorInvalidValue;
    const CornerWs c = carve(ws, nf, a.corners_max, list_cap_of(height, width));
    for (int pass = 0; pass < kPasses; pass++) {
        if (plane_u8) launch_cand((const uint8_t *)plane, nf, height, width, a, pass, c, stream);
        else launch_cand((const int16_t *)plane, nf, height, width, a, pass, c, stream);
        hipLaunchKernelGGL(corners_choose_kernel, dim3(nf), dim3(kAcceptBlock), 0, stream, pass, (unsigned)a.corners_max, c,
                           cand_counts, max_response);
    }
    return hipGetLastError();
}

hipError_t launch_corners_collect(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a,
                                  void *ws, hipStream_t stream)
{
    if (bad_args(a, nf)) return hipErrorInvalidValue;
    const CornerWs c = carve(ws, nf, a.corners_max, list_cap_of(height, width));
    if (plane_u8) launch_cand((const uint8_t *)plane, nf, height, width, a, kPasses, c, stream);
    else launch_cand((const int16_t *)plane, nf, height, width, a, kPasses, c, stream);
    return hipGetLastError();
}

hipError_t launch_corners_accept(int nf, int height, int width, const CornerArgs &a, void *ws, long long *corners,
                                 int *counts, hipStream_t stream)
{
    if (bad_args(a, nf) || height > 65535 || width > 65535) return hipErrorInvalidValue;
    const CornerWs c = carve(ws, nf, a.corners_max, list_cap_of(height, width));
    const unsigned long long md = (unsigned long long)a.min_dist;
    hipLaunchKernelGGL(corners_accept_kernel, dim3(nf), dim3(kAcceptBlock), 0, stream, width, (unsigned)a.corners_max,
                       md * md, c, corners, counts);
    return hipGetLastError();
}

hipError_t launch_corners_arith(const int *sums, size_t n, int mode, int k_q8, long long *out, hipStream_t stream)
{
    hipLaunchKernelGGL(corners_arith_kernel, dim3(plan_corners_arith(n).grid), dim3(kBlock), 0, stream, sums, n, mode, k_q8,
                       out);
    return hipGetLastError();
}

} // namespace canny
