// canny_chamfer.hip -- chamfer template matching on the distance transform, per frame of a batch: the truncated chamfer
// score of every template of a set at every anchor, its local minima under a mean-cost threshold, and an ordered,
// distance-suppressed list of matches.  The rule is part of the interface (include/canny_hip.h);
// tests/chamfer_rule.py restates it in numpy, canny_chamfer_host.cpp in plain C++.
//
// Passes, all on one stream, no host round trip, the launch sequence a function of shapes and arguments alone:
//   cost       : dist2 -> u16 cost plane, min(isqrt(d2 * 256), trunc_q4).
//   score      : tiled  -- a workgroup owns 64 x 16 anchors of one (frame, template).  The cost tile with the template's
//                halo sits in LDS, pre-filled with trunc_q4 outside the frame, so the inner loop has no bounds test.  The
//                template's points are wave-uniform (scalar loads); lanes own adjacent anchors, so a look-up is conflict
//                free; a lane keeps the sums of 4 rows.  A template whose halo does not fit is walked in bands of dy (the
//                set stores the points sorted by dy for that).
//                direct -- one lane per anchor, costs gathered from the cost plane in memory: the A/B yardstick and the
//                second implementation the tests compare.
//   candidates : key = mean_q12 << 31 | base (51 bits, unique).  The matches_max smallest keys of a frame are found by a
//                radix select: four passes, each a histogram of one 13/13/13/12-bit digit of the keys that share the prefix
//                chosen so far (integer atomics into a zeroed histogram: counts commute) and a one-workgroup choice of the
//                digit in which the matches_max-th key lies.  A collect pass then stores every key <= that cut-off key
//                through an atomic slot counter -- the slots' order is arbitrary, and does not reach the output:
//   accept     : one workgroup per frame sorts the collected keys (bitonic, LDS; the keys are distinct) and walks them in
//                order, each against the accepted list by all lanes at once, the pattern of the circles.
#include "canny_kernels.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kDigitBins = 8192;
constexpr int kAcceptBlock = 1024;
constexpr int kPasses = 4;
constexpr int kShift[kPasses] = {38, 25, 12, 0};
constexpr int kWidth[kPasses] = {13, 13, 13, 12};

// floor(sqrt(v)) for v < 2^24 (exact as a float; the correction absorbs the root's rounding)
__device__ __forceinline__ unsigned isqrt24(unsigned v)
{
    unsigned s = (unsigned)sqrtf((float)v);
    if (s * s > v) s--;
    if ((s + 1) * (s + 1) <= v) s++;
    return s;
}

// floor(sqrt(v)) for v < 2^53 (exact as a double)
__device__ __forceinline__ unsigned long long isqrt53(unsigned long long v)
{
    unsigned long long s = (unsigned long long)sqrt((double)v);
    if (s * s > v) s--;
    if ((s + 1) * (s + 1) <= v) s++;
    return s;
}

// THE cost of the rule.  trunc <= 4095: from d2 = 65536 on the root is at least 4096 and the cost is trunc; below, d2 * 256
// is below 2^24.
__device__ __forceinline__ unsigned chamfer_cost(unsigned d2, unsigned trunc)
{
    if (d2 >= 65536u) return trunc;
    return min(isqrt24(d2 << 8), trunc);
}

__global__ __launch_bounds__(kBlock) void chamfer_cost_kernel(const int *__restrict__ dist2, size_t n, unsigned trunc,
                                                              uint16_t *__restrict__ cost)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
        cost[i] = (uint16_t)chamfer_cost((unsigned)dist2[i], trunc);
}

__global__ __launch_bounds__(kBlock) void chamfer_costs_hook_kernel(const int *__restrict__ dist2, size_t n, unsigned trunc,
                                                                    unsigned *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const unsigned d2 = (unsigned)dist2[i];
        out[i] = trunc ? chamfer_cost(d2, trunc) : (unsigned)isqrt53((unsigned long long)d2 * 256ull);
    }
}

// grid (plan_chamfer_cells, frames): anchor i = t * h * w + y * w + x of the frame
__global__ __launch_bounds__(kBlock) void chamfer_score_direct_kernel(const uint16_t *__restrict__ cost, int h, int w,
                                                                      ChamferSetDev set, unsigned trunc,
                                                                      unsigned *__restrict__ scores)
{
    const unsigned hw = (unsigned)h * (unsigned)w, cells = hw * (unsigned)set.n_templates;
    const uint16_t *cf = cost + (size_t)blockIdx.y * hw;
    unsigned *sf = scores + (size_t)blockIdx.y * cells;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < cells; i += gridDim.x * kBlock) {
        const unsigned t = i / hw, r = i - t * hw;
        const int y = (int)(r / (unsigned)w), x = (int)(r - (unsigned)y * (unsigned)w);
        unsigned sum = 0;
        for (int k = set.offsets[t]; k < set.offsets[t + 1]; k++) {
            const uint32_t p = set.points[k];
            const int px = x + (int)(short)(p & 0xffffu), py = y + ((int)p >> 16);
            sum += ((unsigned)px < (unsigned)w && (unsigned)py < (unsigned)h) ? (unsigned)cf[(size_t)py * w + px] : trunc;
        }
        sf[i] = sum;
    }
}

// grid (tiles of a frame, templates, frames); dynamic LDS set.max_elems u16
__global__ __launch_bounds__(kBlock) void chamfer_score_tiled_kernel(const uint16_t *__restrict__ cost, int h, int w,
                                                                     int tiles_x, ChamferSetDev set, unsigned trunc,
                                                                     unsigned *__restrict__ scores)
{
    extern __shared__ uint16_t s_tile[];
    const int t = blockIdx.y, f = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * tiles_x);
    const int x0 = tx * kChamferTileX, y0 = ty * kChamferTileY;
    const size_t hw = (size_t)h * w;
    const uint16_t *cf = cost + (size_t)f * hw;
    const ChamferBox box = set.boxes[t];
    const int cols = kChamferTileX + box.max_x - box.min_x;
    unsigned acc[4] = {0, 0, 0, 0};
    for (int b = set.band_offsets[t]; b < set.band_offsets[t + 1]; b++) {
        const ChamferBand band = set.bands[b];
        __syncthreads(); // the previous band's tile has been read
        for (int r = wave; r < band.rows; r += 4) {
            const int gy = y0 + band.dy0 + r;
            const bool row_in = (unsigned)gy < (unsigned)h;
            for (int c = lane; c < cols; c += 64) {
                const int gx = x0 + box.min_x + c;
                s_tile[r * cols + c] =
                    (row_in && (unsigned)gx < (unsigned)w) ? cf[(size_t)gy * w + gx] : (uint16_t)trunc;
            }
        }
        __syncthreads();
        const int mine = wave * cols + lane - box.min_x - band.dy0 * cols;
#pragma unroll 4
        for (int k = band.begin; k < band.end; k++) {
            const uint32_t p = set.points[k]; // wave-uniform
            const int at = mine + ((int)p >> 16) * cols + (int)(short)(p & 0xffffu);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] += s_tile[at + 4 * j * cols];
        }
    }
    const int x = x0 + lane;
    if (x < w) {
        unsigned *sf = scores + ((size_t)f * set.n_templates + t) * hw;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int y = y0 + wave + 4 * j;
            if (y < h) sf[(size_t)y * w + x] = acc[j];
        }
    }
}

struct CandWs {
    unsigned long long *keys, *prefix, *cutoff;
    unsigned *hist, *need, *flag, *total, *n_emit;
};

// Whether anchor i of a frame's score planes is a candidate; its key if so.
__device__ __forceinline__ bool chamfer_candidate(const unsigned *__restrict__ sf, unsigned i, int h, int w, unsigned hw,
                                                  const int *__restrict__ offsets, unsigned max_mean,
                                                  unsigned long long *key)
{
    const unsigned t = i / hw, r = i - t * hw;
    const unsigned K = (unsigned)(offsets[t + 1] - offsets[t]);
    const unsigned s = sf[i];
    if (s > max_mean * K) return false; // max_mean * K < 2^28
    const int y = (int)(r / (unsigned)w), x = (int)(r - (unsigned)y * (unsigned)w);
    if (x > 0 && !(s < sf[i - 1])) return false;
    if (x < w - 1 && !(s <= sf[i + 1])) return false;
    if (y > 0 && !(s < sf[i - w])) return false;
    if (y < h - 1 && !(s <= sf[i + w])) return false;
    *key = ((unsigned long long)s * 256ull / K) << 31 | i;
    return true;
}

// grid (plan_chamfer_cells, frames).  pass 0: the first digit of every candidate; later: of those that share the prefix.
__global__ __launch_bounds__(kBlock) void chamfer_hist_kernel(const unsigned *__restrict__ scores, int h, int w,
                                                              int n_templates, const int *__restrict__ offsets,
                                                              unsigned max_mean, int pass, int shift, int prev,
                                                              int width, CandWs ws)
{
    const int f = blockIdx.y;
    if (pass > 0 && ws.flag[f]) return;
    const unsigned long long prefix = pass > 0 ? ws.prefix[f] : 0ull;
    const unsigned hw = (unsigned)h * (unsigned)w, cells = hw * (unsigned)n_templates;
    const unsigned *sf = scores + (size_t)f * cells;
    unsigned *hist = ws.hist + (size_t)f * kDigitBins;
    const unsigned mask = (1u << width) - 1u;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < cells; i += gridDim.x * kBlock) {
        unsigned long long key;
        if (!chamfer_candidate(sf, i, h, w, hw, offsets, max_mean, &key)) continue;
        if (pass > 0 && (key >> prev) != prefix) continue;
        atomicAdd(&hist[(unsigned)(key >> shift) & mask], 1u);
    }
}

// grid (frames), one workgroup: the digit in which the need-th smallest key lies; the histogram is zeroed for the next pass.
__global__ __launch_bounds__(kAcceptBlock) void chamfer_choose_kernel(int pass, int width, unsigned matches_max, CandWs ws,
                                                                      int *__restrict__ cand_counts)
{
    __shared__ unsigned s_sum[kAcceptBlock];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (pass > 0 && ws.flag[f]) return; // (workgroup-uniform)
    unsigned *hist = ws.hist + (size_t)f * kDigitBins;
    unsigned need = pass > 0 ? ws.need[f] : matches_max;
    const unsigned long long prefix = pass > 0 ? ws.prefix[f] : 0ull;
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
        }
        if (total <= need) { // every candidate goes on (workgroup-uniform)
            if (tid == 0) {
                ws.flag[f] = 1u;
                ws.cutoff[f] = ~0ull;
            }
            return;
        }
    }
    if (excl < need && need <= incl) {
        unsigned run = excl;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (run + v[j] >= need) {
                const unsigned long long np = prefix << width | (unsigned)(tid * 8 + j);
                ws.prefix[f] = np;
                ws.need[f] = need - run;
                if (pass == kPasses - 1) ws.cutoff[f] = np;
                break;
            }
            run += v[j];
        }
    }
}

// grid (plan_chamfer_cells, frames): every key up to the frame's cut-off, in arbitrary slots (the sort follows)
__global__ __launch_bounds__(kBlock) void chamfer_collect_kernel(const unsigned *__restrict__ scores, int h, int w,
                                                                 int n_templates, const int *__restrict__ offsets,
                                                                 unsigned max_mean, unsigned matches_max, CandWs ws)
{
    const int f = blockIdx.y;
    if (!ws.total[f]) return;
    const unsigned long long cutoff = ws.cutoff[f];
    const unsigned hw = (unsigned)h * (unsigned)w, cells = hw * (unsigned)n_templates;
    const unsigned *sf = scores + (size_t)f * cells;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < cells; i += gridDim.x * kBlock) {
        unsigned long long key;
        if (!chamfer_candidate(sf, i, h, w, hw, offsets, max_mean, &key) || key > cutoff) continue;
        const unsigned slot = atomicAdd(&ws.n_emit[f], 1u);
        if (slot < matches_max) ws.keys[(size_t)f * matches_max + slot] = key;
    }
}

// one workgroup per frame: sort the collected keys, then the candidates in order, each against the accepted list
__global__ __launch_bounds__(kAcceptBlock) void chamfer_accept_kernel(const unsigned *__restrict__ scores, int h, int w,
                                                                      unsigned cells, unsigned matches_max,
                                                                      unsigned long long min_dist2, CandWs ws,
                                                                      int *__restrict__ matches, int *__restrict__ counts)
{
    __shared__ unsigned long long s_key[kHoughMaxLines]; // sorted candidates; then, in place, the accepted ones
    __shared__ unsigned short s_x[kHoughMaxLines], s_y[kHoughMaxLines]; // of the accepted (height, width <= 65535)
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    const unsigned M = min(matches_max, ws.total[f]);
    unsigned P = 1;
    while (P < M) P <<= 1;
    for (unsigned i = tid; i < P; i += kAcceptBlock) s_key[i] = i < M ? ws.keys[(size_t)f * matches_max + i] : ~0ull;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (unsigned size = 2; size <= P; size <<= 1)
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < P; i += kAcceptBlock) {
                const unsigned j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = s_key[i], b = s_key[j];
                    if ((a > b) == ((i & size) == 0)) s_key[i] = b, s_key[j] = a;
                }
            }
            __syncthreads();
        }
    const unsigned hw = (unsigned)h * (unsigned)w;
    // accepted entry j <= its candidate index, so writing it at j never overwrites a candidate still to come
    for (unsigned c = 0; c < M; c++) {
        const unsigned long long key = s_key[c];
        const unsigned r = ((unsigned)key & 0x7fffffffu) % hw;
        const int y = (int)(r / (unsigned)w), x = (int)(r - (unsigned)y * (unsigned)w);
        const int n = s_n;
        int near = 0;
        if (min_dist2)
            for (int j = tid; j < n; j += kAcceptBlock) {
                const long long dx = (long long)x - s_x[j], dy = (long long)y - s_y[j];
                near |= (unsigned long long)(dx * dx + dy * dy) < min_dist2;
            }
        const int any = __syncthreads_or(near); // also: every lane has read s_n and s_key[c]
        if (!any && tid == 0) {
            s_key[n] = key;
            s_x[n] = (unsigned short)x;
            s_y[n] = (unsigned short)y;
            s_n = n + 1;
        }
        __syncthreads();
    }
    const int n = s_n;
    if (matches) {
        const unsigned *sf = scores + (size_t)f * cells;
        for (int j = tid; j < n; j += kAcceptBlock) {
            const unsigned long long key = s_key[j];
            const unsigned base = (unsigned)key & 0x7fffffffu;
            int *rec = matches + ((size_t)f * matches_max + j) * 6;
            rec[0] = s_x[j];
            rec[1] = s_y[j];
            rec[2] = (int)(base / hw);
            rec[3] = (int)sf[base];
            rec[4] = (int)(key >> 31);
            rec[5] = (int)base;
        }
    }
    if (tid == 0) counts[f] = n;
}

CandWs carve(void *ws, int nf, int matches_max)
{
    CandWs c;
    c.keys = (unsigned long long *)ws;
    c.prefix = c.keys + (size_t)nf * matches_max;
    c.cutoff = c.prefix + nf;
    c.hist = (unsigned *)(c.cutoff + nf);
    c.need = c.hist + (size_t)nf * kDigitBins;
    c.flag = c.need + nf;
    c.total = c.flag + nf;
    c.n_emit = c.total + nf;
    return c;
}

} // namespace

LaunchPlan plan_chamfer_cost(unsigned long long n_px) { return capped_plan(n_px, kBlock, 16384); }
LaunchPlan plan_chamfer_cells(unsigned long long cells) { return capped_plan(cells, kBlock, 2048); }

int chamfer_chunk_frames(int n_frames, int height, int width, int n_templates, bool with_scores, int budget_mb)
{
    // per frame: 2 B/px of costs, and 4 B per template and pixel of scores unless the caller holds them
    const unsigned long long budget = (unsigned long long)(budget_mb > 0 ? budget_mb : 256) << 20;
    const unsigned long long px = (unsigned long long)height * width;
    const unsigned long long per_frame = with_scores ? 2ull * px : 4ull * px * n_templates;
    const unsigned long long nf = std::min<unsigned long long>(4096, std::max<unsigned long long>(1, budget / per_frame));
    return (int)std::min<unsigned long long>(nf, (unsigned long long)n_frames);
}

size_t chamfer_ws_bytes(int nf, int matches_max)
{
    return (size_t)nf * matches_max * 8 + (size_t)nf * 16 + ((size_t)nf * kDigitBins + 4 * (size_t)nf) * sizeof(unsigned);
}

int chamfer_build_layout(const int *offsets, const short *points, int n_templates, ChamferLayout &out)
{
    if (!offsets || !points || n_templates < 1 || offsets[0] != 0) return 1;
    if (n_templates > 1024) return 2;
    for (int t = 0; t < n_templates; t++) {
        if (offsets[t + 1] <= offsets[t]) return 1;
        if (offsets[t + 1] - offsets[t] > 65536 || offsets[t + 1] > (1 << 20)) return 2;
    }
    const int total = offsets[n_templates];
    for (int k = 0; k < 2 * total; k++)
        if (points[k] < -255 || points[k] > 255) return 2;
    out = ChamferLayout();
    out.n_templates = n_templates;
    out.offsets.assign(offsets, offsets + n_templates + 1);
    out.points.resize((size_t)total);
    out.boxes.resize((size_t)n_templates);
    out.band_offsets.assign(1, 0);
    for (int t = 0; t < n_templates; t++) {
        const int b = offsets[t], e = offsets[t + 1];
        std::vector<std::pair<int, int>> pts; // (dy, dx)
        ChamferBox box{255, -255, 255, -255};
        for (int k = b; k < e; k++) {
            const int dx = points[2 * k], dy = points[2 * k + 1];
            pts.emplace_back(dy, dx);
            box.min_x = std::min(box.min_x, dx), box.max_x = std::max(box.max_x, dx);
            box.min_y = std::min(box.min_y, dy), box.max_y = std::max(box.max_y, dy);
        }
        std::sort(pts.begin(), pts.end());
        for (int k = b; k < e; k++)
            out.points[(size_t)k] = ((uint32_t)pts[(size_t)(k - b)].second & 0xffffu) | ((uint32_t)pts[(size_t)(k - b)].first << 16);
        out.boxes[(size_t)t] = box;
        out.max_k = std::max(out.max_k, e - b);
        // bands: as many rows of dy as keep (rows of dy + tile rows - 1) * cols within the LDS tile
        const int cols = kChamferTileX + box.max_x - box.min_x;
        const int span = kChamferLdsElems / cols - kChamferTileY + 1; // >= 42
        int k = b;
        while (k < e) {
            ChamferBand band;
            band.begin = k;
            band.dy0 = pts[(size_t)(k - b)].first;
            int last = band.dy0;
            while (k < e && pts[(size_t)(k - b)].first < band.dy0 + span) last = pts[(size_t)(k - b)].first, k++;
            band.end = k;
            band.rows = last - band.dy0 + kChamferTileY;
            out.max_elems = std::max(out.max_elems, band.rows * cols);
            out.bands.push_back(band);
        }
        out.band_offsets.push_back((int)out.bands.size());
    }
    return 0;
}

// Tiled wherever a template has enough points to pay for filling the tile.
int chamfer_auto_route(const ChamferLayout &lay) { return lay.max_k >= 8 ? 2 : 1; }

hipError_t launch_chamfer_cost(const int *dist2, size_t n_px, int trunc_q4, uint16_t *cost, hipStream_t stream)
{
    hipLaunchKernelGGL(chamfer_cost_kernel, dim3(plan_chamfer_cost(n_px).grid), dim3(kBlock), 0, stream, dist2, n_px,
                       (unsigned)trunc_q4, cost);
    return hipGetLastError();
}

hipError_t launch_chamfer_costs_hook(const int *dist2, size_t n, int trunc_q4, unsigned *out, hipStream_t stream)
{
    hipLaunchKernelGGL(chamfer_costs_hook_kernel, dim3(plan_chamfer_cost(n).grid), dim3(kBlock), 0, stream, dist2, n,
                       (unsigned)trunc_q4, out);
    return hipGetLastError();
}

hipError_t launch_chamfer_score(const uint16_t *cost, int nf, int height, int width, const ChamferSetDev &set, int trunc_q4,
                                bool tiled, unsigned *scores, hipStream_t stream)
{
    if (tiled) {
        if (set.max_elems > kChamferLdsElems) return hipErrorInvalidValue;
        const int tiles_x = (width + kChamferTileX - 1) / kChamferTileX, tiles_y = (height + kChamferTileY - 1) / kChamferTileY;
        const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, set.n_templates, nf);
        hipLaunchKernelGGL(chamfer_score_tiled_kernel, grid, dim3(kBlock), (size_t)set.max_elems * sizeof(uint16_t), stream,
                           cost, height, width, tiles_x, set, (unsigned)trunc_q4, scores);
    } else {
        const dim3 grid(plan_chamfer_cells((unsigned long long)height * width * set.n_templates).grid, nf);
        hipLaunchKernelGGL(chamfer_score_direct_kernel, grid, dim3(kBlock), 0, stream, cost, height, width, set,
                           (unsigned)trunc_q4, scores);
    }
    return hipGetLastError();
}

hipError_t launch_chamfer_candidates(const unsigned *scores, int nf, int height, int width, const ChamferSetDev &set,
                                     int max_mean_q4, int matches_max, void *ws, int *cand_counts, hipStream_t stream)
{
    const CandWs c = carve(ws, nf, matches_max);
    // histogram, need, flag, total and the collect counters start from zero; keys, prefix and cutoff are written before
    // they are read
    hipError_t e = hipMemsetAsync(c.hist, 0, ((size_t)nf * kDigitBins + 4 * (size_t)nf) * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(plan_chamfer_cells((unsigned long long)height * width * set.n_templates).grid, nf);
    for (int pass = 0; pass < kPasses; pass++) {
        hipLaunchKernelGGL(chamfer_hist_kernel, grid, dim3(kBlock), 0, stream, scores, height, width, set.n_templates,
                           set.offsets, (unsigned)max_mean_q4, pass, kShift[pass], pass ? kShift[pass - 1] : 63,
                           kWidth[pass], c);
        hipLaunchKernelGGL(chamfer_choose_kernel, dim3(nf), dim3(kAcceptBlock), 0, stream, pass, kWidth[pass],
                           (unsigned)matches_max, c, cand_counts);
    }
    hipLaunchKernelGGL(chamfer_collect_kernel, grid, dim3(kBlock), 0, stream, scores, height, width, set.n_templates,
                       set.offsets, (unsigned)max_mean_q4, (unsigned)matches_max, c);
    return hipGetLastError();
}

hipError_t launch_chamfer_accept(const unsigned *scores, int nf, int height, int width, int n_templates, int matches_max,
                                 int min_dist, void *ws, int *matches, int *counts, hipStream_t stream)
{
    if (matches_max > kHoughMaxLines || height > 65535 || width > 65535) return hipErrorInvalidValue;
    const CandWs c = carve(ws, nf, matches_max);
    const unsigned long long md = (unsigned long long)min_dist;
    hipLaunchKernelGGL(chamfer_accept_kernel, dim3(nf), dim3(kAcceptBlock), 0, stream, scores, height, width,
                       (unsigned)height * (unsigned)width * (unsigned)n_templates, (unsigned)matches_max, md * md, c,
                       matches, counts);
    return hipGetLastError();
}

} // namespace canny
