// canny_hough.hip -- the standard Hough line transform (cv::HoughLines semantics) of a finished edge map, per frame of a
// batch: accumulator, five-way local-maximum peaks, the lines_max strongest lines first.  The rule is part of the
// interface (include/canny_hip.h); a few lines of numpy restate it (tests/hough_rule.py).
//
// Passes, all on one stream, no host round trip:
//   vote    : LDS rows (default) -- a workgroup owns one frame and A consecutive angles, keeps those accumulator rows in
//             LDS, walks the frame's set pixels, votes with LDS integer atomics and writes its rows (and their zero
//             border) once with plain coalesced stores: no global atomics, nothing to zero in HBM beforehand.
//             Global atomics (fallback for rows that do not fit in LDS, and the A/B form) -- one lane per pixel, every
//             angle, atomicAdd into a zeroed accumulator.  Integer adds commute: both forms give the same bytes.
//   peaks   : every cell against its four neighbours and the threshold; per frame the true count and a histogram of
//             the peaks' vote values
//   select  : cut-off vote from the histogram (one workgroup per frame) -> ties at the cut-off counted per accumulator
//             row -> the base of the last tie that still fits (one workgroup per frame: prefix over the rows, then an
//             ordered scan of ONE row) -> everything above the cut and the ties up to that base collected (any order)
//             -> at most lines_max 64-bit keys sorted in LDS by one workgroup per frame (votes descending, base
//             ascending: a total order, so the output bytes do not depend on the collection order).
//
// The float contract of a vote rests on three operations, each rounded to binary32 on its own (the tree is built with
// -ffp-contract=off; __fmul_rn / __fadd_rn say so again at the place it matters): x*cos, y*sin, their sum; then
// round-half-even to int (v_rndne_f32).  No transcendental function runs on the device: the tables come from the host.
#include "canny_kernels.h"
#include "canny_wave.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kVoteBlock = 1024;  // LDS-row vote: 16 waves share the rows
constexpr int kCellBlock = 256;   // passes over the accumulator's cells
constexpr int kSortBlock = 1024;
constexpr int kSortMax = 4096;    // = CANNY_HIP_HOUGH_MAX_LINES: 32 KB of 64-bit keys

enum { kCutK = 0, kCutVote = 1, kCutNeed = 2, kCutBase = 3, kCutTaken = 4, kCutWords = 8 };

struct VoteSrc {
    const uint64_t *strong;
    const uint8_t *bits;
    const uint32_t *points;
    const unsigned long long *offsets;
};

// word u of frame f: 64 consecutive pixels of one row, bit i = column x0 + i, columns >= width cleared.
// Strong plane: u runs over the plane's words in memory order (a wave's load is one coalesced 512 bytes = 64 rows of
// one tile); rows past the height hold nothing.  Packed bits: u = y * tiles_x + k, rows MSB-first, padding bits masked.
template <int SRC>
__device__ __forceinline__ uint64_t src_word(const VoteSrc &src, const HystGeom &g, int row_bytes, int f, unsigned u,
                                             int *y, int *x0)
{
    if constexpr (SRC == kSrcStrong) {
        const unsigned tile = u >> 6;
        const int ty = (int)(tile / (unsigned)g.tiles_x), tx = (int)(tile - (unsigned)ty * g.tiles_x);
        *y = (ty << 6) + (int)(u & 63u);
        *x0 = tx << 6;
        if (*y >= g.height) return 0ull;
        const int left = g.width - *x0;
        const uint64_t mask = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        return src.strong[(size_t)f * g.tiles_y * g.tiles_x * 64 + u] & mask;
    } else {
        const int yy = (int)(u / (unsigned)g.tiles_x), k = (int)(u - (unsigned)yy * g.tiles_x);
        *y = yy;
        *x0 = k << 6;
        const int left = g.width - *x0;
        const uint64_t mask = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        const uint8_t *row = src.bits + ((size_t)f * g.height + yy) * (size_t)row_bytes + (size_t)k * 8;
        const int nb = min(8, row_bytes - k * 8);
        uint64_t w = 0;
        for (int j = 0; j < nb; j++) w |= (uint64_t)(__brev((unsigned)row[j]) >> 24) << (8 * j);
        return w & mask;
    }
}

template <int SRC>
__device__ __forceinline__ unsigned src_units(const HystGeom &g)
{
    return SRC == kSrcStrong ? (unsigned)g.tiles_y * g.tiles_x * 64u : (unsigned)g.height * g.tiles_x;
}

// vote(x, y) for every set pixel of frame f that falls to this thread (tid of nthreads)
template <int SRC, class Vote>
__device__ __forceinline__ void for_each_point(const VoteSrc &src, const HystGeom &g, int row_bytes, int f, unsigned tid,
                                               unsigned nthreads, Vote &&vote)
{
    if constexpr (SRC == kSrcPoints) {
        const unsigned long long b = src.offsets[f], e = src.offsets[f + 1];
        const unsigned n_px = (unsigned)g.height * (unsigned)g.width;
        for (unsigned long long p = b + tid; p < e; p += nthreads) {
            const unsigned idx = src.points[p];
            if (idx >= n_px) continue; // not a pixel of the frame: no vote, no access
            const int y = (int)(idx / (unsigned)g.width);
            vote((int)(idx - (unsigned)y * g.width), y);
        }
    } else {
        const unsigned n = src_units<SRC>(g);
        for (unsigned u0 = tid; u0 < n; u0 += 4u * nthreads) { // four words in flight per lane
            uint64_t w[4];
            int y[4], x0[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned u = u0 + (unsigned)j * nthreads;
                w[j] = u < n ? src_word<SRC>(src, g, row_bytes, f, u, &y[j], &x0[j]) : 0ull;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint64_t v = w[j];
                while (v) {
                    vote(x0[j] + (int)__builtin_ctzll(v), y[j]);
                    v &= v - 1;
                }
            }
        }
    }
}

// grid (ceil(numangle / rows), n_frames); dynamic LDS rows * numrho ints
template <int SRC>
__global__ __launch_bounds__(kVoteBlock) void hough_vote_lds_kernel(VoteSrc src, HystGeom g, int row_bytes,
                                                                    const float *__restrict__ tab, int numangle,
                                                                    int numrho, int rows, int *__restrict__ accum)
{
    extern __shared__ int s_rows[];
    const int f = blockIdx.y, n0 = blockIdx.x * rows, na = min(rows, numangle - n0);
    for (int i = threadIdx.x; i < na * numrho; i += kVoteBlock) s_rows[i] = 0;
    __syncthreads();
    const int half = (numrho - 1) / 2;
    const float *tc = tab + n0, *ts = tab + numangle + n0; // wave-uniform reads
    for_each_point<SRC>(src, g, row_bytes, f, threadIdx.x, kVoteBlock, [&](int x, int y) {
        for (int a = 0; a < na; a++) {
            const int r = vote_r(x, y, tc[a], ts[a], half);
            if ((unsigned)r < (unsigned)numrho) atomicAdd(&s_rows[a * numrho + r], 1); // always true for a pixel
        }
    });
    __syncthreads();
    const int stride = numrho + 2;
    int *acc = accum + (size_t)f * (numangle + 2) * stride;
    for (int a = 0; a < na; a++) {
        int *row = acc + (size_t)(n0 + a + 1) * stride;
        for (int i = threadIdx.x; i < stride; i += kVoteBlock)
            row[i] = (i == 0 || i == stride - 1) ? 0 : s_rows[a * numrho + i - 1];
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < stride; i += kVoteBlock) acc[i] = 0;
    if (blockIdx.x == gridDim.x - 1)
        for (int i = threadIdx.x; i < stride; i += kVoteBlock) acc[(size_t)(numangle + 1) * stride + i] = 0;
}

// grid (blocks, n_frames); the accumulator has been zeroed
template <int SRC>
__global__ __launch_bounds__(256) void hough_vote_global_kernel(VoteSrc src, HystGeom g, int row_bytes,
                                                                const float *__restrict__ tab, int numangle, int numrho,
                                                                int *__restrict__ accum)
{
    const int f = blockIdx.y;
    const int half = (numrho - 1) / 2, stride = numrho + 2;
    int *acc = accum + (size_t)f * (numangle + 2) * stride;
    for_each_point<SRC>(src, g, row_bytes, f, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x,
                        [&](int x, int y) {
                            for (int n = 0; n < numangle; n++) {
                                const int r = vote_r(x, y, tab[n], tab[numangle + n], half);
                                if ((unsigned)r < (unsigned)numrho) atomicAdd(&acc[(size_t)(n + 1) * stride + r + 1], 1);
                            }
                        });
}

// cell (n, r) of a frame's accumulator: its votes if it is a peak, else 0 (a peak has at least one vote)
__device__ __forceinline__ int peak_votes(const int *__restrict__ acc, int stride, int n, int r, int threshold)
{
    const int *p = acc + (size_t)(n + 1) * stride + r + 1;
    const int v = p[0];
    if (v <= 0 || v <= threshold) return 0;
    return (v > p[-1] && v >= p[1] && v > p[-stride] && v >= p[stride]) ? v : 0;
}

// grid (blocks, n_frames): counts[f] = peaks of frame f; hist[f][v] = peaks with v votes (v clamped to nb - 1, which the
// host's bound on a cell's votes never reaches)
__global__ __launch_bounds__(kCellBlock) void hough_peaks_kernel(const int *__restrict__ accum, int numangle, int numrho,
                                                                 int threshold, int *__restrict__ counts,
                                                                 unsigned *__restrict__ hist, int nb)
{
    const int f = blockIdx.y, stride = numrho + 2;
    const int *acc = accum + (size_t)f * (numangle + 2) * stride;
    const unsigned cells = (unsigned)numangle * (unsigned)numrho;
    unsigned mine = 0;
    for (unsigned c = blockIdx.x * kCellBlock + threadIdx.x; c < cells; c += gridDim.x * kCellBlock) {
        const int n = (int)(c / (unsigned)numrho), r = (int)(c - (unsigned)n * numrho);
        const int v = peak_votes(acc, stride, n, r, threshold);
        if (v) {
            mine++;
            atomicAdd(&hist[(size_t)f * nb + min(v, nb - 1)], 1u);
        }
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&counts[f], (int)mine);
}

// one workgroup per frame: K = min(lines_max, counts[f]); the cut-off vote is the largest v with at least K peaks of v or
// more votes; need = K - (peaks above v) ties at v are taken
__global__ __launch_bounds__(kCellBlock) void hough_cut_kernel(const int *__restrict__ counts,
                                                               const unsigned *__restrict__ hist, int nb, int lines_max,
                                                               unsigned *__restrict__ cut)
{
    __shared__ unsigned s_wave[4];
    const int f = blockIdx.x;
    const unsigned K = (unsigned)min(lines_max, counts[f]);
    unsigned *c = cut + (size_t)f * kCutWords;
    if (threadIdx.x == 0) {
        c[kCutK] = K;
        c[kCutTaken] = 0;
        c[kCutBase] = 0xffffffffu;
        if (!K) c[kCutVote] = 0x7fffffffu, c[kCutNeed] = 0;
    }
    if (!K) return;
    const unsigned *h = hist + (size_t)f * nb;
    unsigned above = 0; // peaks with more votes than this chunk's highest bin
    for (int top = nb - 1; top >= 0 && above < K; top -= kCellBlock) {
        const int v = top - (int)threadIdx.x;
        const unsigned here = v >= 0 ? h[v] : 0u;
        unsigned chunk;
        const unsigned ex = block_exclusive_scan(here, s_wave, &chunk);
        if (here && above + ex < K && above + ex + here >= K) {
            c[kCutVote] = (unsigned)v;
            c[kCutNeed] = K - (above + ex);
        }
        above += chunk;
    }
}

// grid (blocks, n_frames): ties[f][n] = peaks of accumulator row n with exactly the cut-off vote
__global__ __launch_bounds__(kCellBlock) void hough_ties_kernel(const int *__restrict__ accum, int numangle, int numrho,
                                                                int threshold, const unsigned *__restrict__ cut,
                                                                unsigned *__restrict__ ties)
{
    const int f = blockIdx.y, stride = numrho + 2;
    if (!cut[(size_t)f * kCutWords + kCutK]) return;
    const int vc = (int)cut[(size_t)f * kCutWords + kCutVote];
    const int *acc = accum + (size_t)f * (numangle + 2) * stride;
    const unsigned cells = (unsigned)numangle * (unsigned)numrho;
    for (unsigned c = blockIdx.x * kCellBlock + threadIdx.x; c < cells; c += gridDim.x * kCellBlock) {
        const int n = (int)(c / (unsigned)numrho), r = (int)(c - (unsigned)n * numrho);
        if (acc[(size_t)(n + 1) * stride + r + 1] != vc) continue;
        if (peak_votes(acc, stride, n, r, threshold)) atomicAdd(&ties[(size_t)f * numangle + n], 1u);
    }
}

// one workgroup per frame: the base of the need-th tie in base order.  Rows partition the bases, so a prefix over the
// rows' tie counts finds its row, and an ordered scan of that one row finds the cell.
__global__ __launch_bounds__(kCellBlock) void hough_tie_base_kernel(const int *__restrict__ accum, int numangle,
                                                                    int numrho, int threshold,
                                                                    const unsigned *__restrict__ ties,
                                                                    unsigned *__restrict__ cut)
{
    __shared__ unsigned s_wave[4];
    __shared__ unsigned s_row, s_rank;
    const int f = blockIdx.x, stride = numrho + 2;
    unsigned *c = cut + (size_t)f * kCutWords;
    if (!c[kCutK]) return;
    const unsigned need = c[kCutNeed];
    const int vc = (int)c[kCutVote];
    const unsigned *t = ties + (size_t)f * numangle;
    if (threadIdx.x == 0) s_row = 0, s_rank = 0;
    __syncthreads();
    unsigned before = 0;
    for (int n0 = 0; n0 < numangle && before < need; n0 += kCellBlock) {
        const int n = n0 + (int)threadIdx.x;
        const unsigned here = n < numangle ? t[n] : 0u;
        unsigned chunk;
        const unsigned ex = block_exclusive_scan(here, s_wave, &chunk);
        if (here && before + ex < need && before + ex + here >= need) {
            s_row = (unsigned)n;
            s_rank = need - (before + ex); // 1-based rank of the tie within its row
        }
        before += chunk;
    }
    __syncthreads();
    const int n = (int)s_row;
    const unsigned rank = s_rank;
    const int *acc = accum + (size_t)f * (numangle + 2) * stride;
    before = 0;
    for (int r0 = 0; r0 < numrho && before < rank; r0 += kCellBlock) {
        const int r = r0 + (int)threadIdx.x;
        const unsigned here =
            (r < numrho && acc[(size_t)(n + 1) * stride + r + 1] == vc && peak_votes(acc, stride, n, r, threshold)) ? 1u : 0u;
        unsigned chunk;
        const unsigned ex = block_exclusive_scan(here, s_wave, &chunk);
        if (here && before + ex + 1 == rank) c[kCutBase] = (unsigned)((n + 1) * stride + r + 1);
        before += chunk;
    }
}

// grid (blocks, n_frames): the K survivors of a frame as keys, in whatever order the slots are handed out
__global__ __launch_bounds__(kCellBlock) void hough_collect_kernel(const int *__restrict__ accum, int numangle, int numrho,
                                                                   int threshold, int lines_max,
                                                                   unsigned *__restrict__ cut,
                                                                   unsigned long long *__restrict__ cand)
{
    const int f = blockIdx.y, stride = numrho + 2;
    unsigned *cf = cut + (size_t)f * kCutWords;
    const unsigned K = cf[kCutK];
    if (!K) return;
    const int vc = (int)cf[kCutVote];
    const unsigned last = cf[kCutBase];
    const int *acc = accum + (size_t)f * (numangle + 2) * stride;
    const unsigned cells = (unsigned)numangle * (unsigned)numrho;
    for (unsigned c = blockIdx.x * kCellBlock + threadIdx.x; c < cells; c += gridDim.x * kCellBlock) {
        const int n = (int)(c / (unsigned)numrho), r = (int)(c - (unsigned)n * numrho);
        const unsigned base = (unsigned)((n + 1) * stride + r + 1);
        if (acc[base] < vc) continue;
        const int v = peak_votes(acc, stride, n, r, threshold);
        if (!v || (v == vc && base > last)) continue;
        const unsigned slot = atomicAdd(&cf[kCutTaken], 1u);
        if (slot < K) cand[(size_t)f * lines_max + slot] = ((unsigned long long)(0x7fffffffu - (unsigned)v) << 32) | base;
    }
}

// one workgroup per frame: bitonic sort of the K keys (padded with all-ones to a power of two) in LDS, then the outputs
__global__ __launch_bounds__(kSortBlock) void hough_sort_kernel(const unsigned *__restrict__ cut,
                                                                const unsigned long long *__restrict__ cand,
                                                                int lines_max, int numrho, float rho, float theta,
                                                                float min_theta, float *__restrict__ lines,
                                                                int *__restrict__ votes, unsigned *__restrict__ bases)
{
    __shared__ unsigned long long s_key[kSortMax];
    const int f = blockIdx.x;
    const int K = (int)cut[(size_t)f * kCutWords + kCutK];
    if (!K) return;
    int N = 2;
    while (N < K) N <<= 1;
    for (int i = threadIdx.x; i < N; i += kSortBlock) s_key[i] = i < K ? cand[(size_t)f * lines_max + i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += kSortBlock) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = s_key[i], b = s_key[p];
                    if ((a > b) == ((i & k) == 0)) s_key[i] = b, s_key[p] = a;
                }
            }
            __syncthreads();
        }
    }
    const int stride = numrho + 2;
    const float centre = (float)(numrho - 1) * 0.5f;
    for (int i = threadIdx.x; i < K; i += kSortBlock) {
        const unsigned long long key = s_key[i];
        const unsigned base = (unsigned)key;
        const size_t slot = (size_t)f * lines_max + i;
        if (bases) bases[slot] = base;
        if (votes) votes[slot] = (int)(0x7fffffffu - (unsigned)(key >> 32));
        if (lines) {
            const int n = (int)(base / (unsigned)stride) - 1, r = (int)(base % (unsigned)stride) - 1;
            lines[2 * slot] = __fmul_rn(__fsub_rn((float)r, centre), rho);
            lines[2 * slot + 1] = __fadd_rn(min_theta, __fmul_rn((float)n, theta));
        }
    }
}

unsigned cell_grid(const HoughGeom &hg) { return plan_hough_cells((unsigned long long)hg.numangle * hg.numrho).grid; }

template <int SRC>
hipError_t vote_lds(const VoteSrc &src, const HystGeom &g, const HoughGeom &hg, const float *tab, int *accum, int rows,
                    hipStream_t stream)
{
    const size_t lds = (size_t)rows * hg.numrho * sizeof(int);
    auto kernel = hough_vote_lds_kernel<SRC>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((hg.numangle + rows - 1) / rows, g.n_frames), dim3(kVoteBlock), lds, stream, src, g,
                       (g.width + 7) / 8, tab, hg.numangle, hg.numrho, rows, accum);
    return hipGetLastError();
}

template <int SRC>
hipError_t vote_global(const VoteSrc &src, const HystGeom &g, const HoughGeom &hg, const float *tab, int *accum,
                       hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(accum, 0, hough_accum_bytes(hg, g.n_frames), stream);
    if (e != hipSuccess) return e;
    const unsigned blocks = plan_hough_vote_global(g, (VoteSource)SRC).grid;
    hipLaunchKernelGGL(hough_vote_global_kernel<SRC>, dim3(blocks, g.n_frames), dim3(256), 0, stream, src, g,
                       (g.width + 7) / 8, tab, hg.numangle, hg.numrho, accum);
    return hipGetLastError();
}

} // namespace

// enough lanes that each takes a few pixels' worth of words; every lane then walks all angles.  The grid is sized by the
// strong plane's words for both plane sources.
LaunchPlan plan_hough_vote_global(const HystGeom &g, VoteSource src, unsigned long long n_points)
{
    const unsigned long long words = (unsigned long long)g.tiles_y * g.tiles_x * 64;
    if (src == kSrcPoints) return sized_plan(n_points, 256, (unsigned long long)g.height * g.width / 16, 256, 2048);
    return sized_plan(src == kSrcBits ? (unsigned long long)g.height * g.tiles_x : words, 256, words, 256, 2048);
}
// a workgroup takes kCellBlock cells per trip; uncapped, the grid is sized for four trips
LaunchPlan plan_hough_cells(unsigned long long cells)
{
    return sized_plan(cells, kCellBlock, cells, kCellBlock * 4, 4096);
}

int hough_lds_rows(const HoughGeom &hg, int budget_bytes)
{
    const size_t row = (size_t)hg.numrho * sizeof(int);
    if (row > (size_t)kHoughLdsMax) return 0;
    const size_t budget = std::max<size_t>(row, std::min<size_t>((size_t)std::max(budget_bytes, 1), kHoughLdsMax));
    return (int)std::min<size_t>(std::min<size_t>(budget / row, 16), (size_t)hg.numangle);
}

hipError_t launch_hough_vote(const uint64_t *strong, const uint8_t *bits, const uint32_t *points,
                             const unsigned long long *offsets, const HystGeom &g, const HoughGeom &hg, const float *tab,
                             int *accum, int lds_rows, hipStream_t stream)
{
    const VoteSrc src{strong, bits, points, offsets};
    if (lds_rows > 0) {
        if (points) return vote_lds<kSrcPoints>(src, g, hg, tab, accum, lds_rows, stream);
        if (bits) return vote_lds<kSrcBits>(src, g, hg, tab, accum, lds_rows, stream);
        return vote_lds<kSrcStrong>(src, g, hg, tab, accum, lds_rows, stream);
    }
    if (points) return vote_global<kSrcPoints>(src, g, hg, tab, accum, stream);
    if (bits) return vote_global<kSrcBits>(src, g, hg, tab, accum, stream);
    return vote_global<kSrcStrong>(src, g, hg, tab, accum, stream);
}

hipError_t launch_hough_peaks(const int *accum, int n_frames, const HoughGeom &hg, int threshold, int *counts,
                              unsigned *hist, int hist_bins, hipStream_t stream)
{
    hipLaunchKernelGGL(hough_peaks_kernel, dim3(cell_grid(hg), n_frames), dim3(kCellBlock), 0, stream, accum, hg.numangle,
                       hg.numrho, threshold, counts, hist, hist_bins);
    return hipGetLastError();
}

hipError_t launch_hough_select(const int *accum, int n_frames, const HoughGeom &hg, int threshold, int lines_max,
                               const int *counts, const unsigned *hist, int hist_bins, unsigned *ties, unsigned *cut,
                               unsigned long long *cand, float *lines, int *votes, unsigned *bases, hipStream_t stream)
{
    if (lines_max > kSortMax) return hipErrorInvalidValue;
    hipError_t e;
    hipLaunchKernelGGL(hough_cut_kernel, dim3(n_frames), dim3(kCellBlock), 0, stream, counts, hist, hist_bins, lines_max,
                       cut);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(hough_ties_kernel, dim3(cell_grid(hg), n_frames), dim3(kCellBlock), 0, stream, accum, hg.numangle,
                       hg.numrho, threshold, cut, ties);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(hough_tie_base_kernel, dim3(n_frames), dim3(kCellBlock), 0, stream, accum, hg.numangle, hg.numrho,
                       threshold, ties, cut);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(hough_collect_kernel, dim3(cell_grid(hg), n_frames), dim3(kCellBlock), 0, stream, accum,
                       hg.numangle, hg.numrho, threshold, lines_max, cut, cand);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(hough_sort_kernel, dim3(n_frames), dim3(kSortBlock), 0, stream, cut, cand, lines_max, hg.numrho,
                       hg.rho, hg.theta, hg.min_theta, lines, votes, bases);
    return hipGetLastError();
}

} // namespace canny
