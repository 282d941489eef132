// canny_points.hip -- edge point lists: the pixels of an edge map as ascending indices r*width + c per frame
// (np.flatnonzero / cv::findNonZero; the reference's own index convention, src/utils.cpp:360-427), the lists of a
// batch concatenated in frame order with a CSR offset array.  DESIGN.md section 12.
//
// Three passes on one stream, no host round trip, no atomics:
//   count   : one wave per image row; lanes take the row's 64-pixel words, popcount, wave sum -> one u32 per row
//   scan    : exclusive prefix of the row counts within each frame (one workgroup per frame, in place), then of the
//             frame totals across the batch (one workgroup) -> offsets[0..n_frames]
//   scatter : one wave per image row again; a shuffle ladder turns the per-word popcounts into each lane's position in
//             the row's run, and each lane expands its word (ctz / clear lowest bit) into points[]
// The unit that owns a contiguous run of the output is an image ROW: the strong plane is tiled (64 rows of tile tx,
// then 64 rows of tile tx + 1), raster order is not tile order.  A row's words lie 512 bytes apart in the strong plane,
// so a wave's load touches tiles_x cache lines and uses 8 bytes of each; the 16 rows that share those lines are the 16
// waves of one workgroup.
//
// Two sources, one row-word fetch:
//   strong plane : hysteresis' converged bit-plane (HystGeom; bit i of a word = column 64*tx + i)
//   packed bits  : a caller's bit map, rows MSB-first and padded to bytes (canny_hip_dev_canny_bits), any byte address;
//                  its padding bits are masked off, never trusted
// Nothing is stored at or beyond points + capacity; the counts and offsets are always the true ones.
#include "canny_kernels.h"
#include "canny_wave.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kPtsBlock = 1024; // 16 waves = 16 consecutive rows per workgroup step

template <bool BITS>
__global__ __launch_bounds__(kPtsBlock) void points_count_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                                 uint32_t *__restrict__ row_counts)
{
    const int lane = threadIdx.x & 63;
    const size_t n_rows = (size_t)g.n_frames * g.height;
    const size_t wave_stride = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rows; r += wave_stride) {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        unsigned c = 0;
        for (int k = lane; k < g.tiles_x; k += 64) c += (unsigned)__popcll(row_word<BITS>(src, g, row_bytes, f, y, k));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) row_counts[r] = c;
    }
}

// rows[f][y]: count of row y -> number of edge pixels of frame f before row y; totals[f] = the frame's count
__global__ __launch_bounds__(256) void points_scan_rows_kernel(uint32_t *__restrict__ rows,
                                                               unsigned long long *__restrict__ totals, int height)
{
    __shared__ unsigned long long s_wave[4];
    uint32_t *r = rows + (size_t)blockIdx.x * height;
    unsigned long long carry = 0;
    for (int base = 0; base < height; base += 256) {
        const int i = base + (int)threadIdx.x;
        unsigned long long chunk;
        const unsigned long long ex = block_exclusive_scan<unsigned long long>(i < height ? r[i] : 0u, s_wave, &chunk);
        if (i < height) r[i] = (uint32_t)(carry + ex); // < height * width < 2^31
        carry += chunk;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// offsets[0] = 0, offsets[f + 1] = offsets[f] + totals[f]
__global__ __launch_bounds__(256) void points_scan_frames_kernel(const unsigned long long *__restrict__ totals,
                                                                 unsigned long long *__restrict__ offsets, int n_frames)
{
    __shared__ unsigned long long s_wave[4];
    unsigned long long carry = 0;
    for (int base = 0; base < n_frames; base += 256) {
        const int i = base + (int)threadIdx.x;
        unsigned long long chunk;
        const unsigned long long ex = block_exclusive_scan(i < n_frames ? totals[i] : 0ull, s_wave, &chunk);
        if (i < n_frames) offsets[i] = carry + ex;
        carry += chunk;
    }
    if (threadIdx.x == 0) offsets[n_frames] = carry;
}

template <bool BITS>
__global__ __launch_bounds__(kPtsBlock) void points_scatter_kernel(const void *__restrict__ src, HystGeom g,
                                                                   int row_bytes, const uint32_t *__restrict__ row_offsets,
                                                                   const unsigned long long *__restrict__ offsets,
                                                                   uint32_t *__restrict__ points,
                                                                   unsigned long long capacity)
{
    const int lane = threadIdx.x & 63;
    const size_t n_rows = (size_t)g.n_frames * g.height;
    const size_t wave_stride = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rows; r += wave_stride) {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        unsigned long long run = offsets[f] + row_offsets[r]; // where this row's run starts (wave-uniform)
        if (run >= capacity) continue;
        for (int k0 = 0; k0 < g.tiles_x; k0 += 64) { // rows wider than 4096 pixels take several rounds
            const int k = k0 + lane;
            uint64_t w = k < g.tiles_x ? row_word<BITS>(src, g, row_bytes, f, y, k) : 0ull;
            const unsigned c = (unsigned)__popcll(w);
            unsigned incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            unsigned long long pos = run + (incl - c);
            run += __shfl(incl, 63);
            const uint32_t px = (uint32_t)y * (uint32_t)g.width + ((uint32_t)k << 6);
            while (w) {
                if (pos < capacity) points[pos] = px + (uint32_t)__builtin_ctzll(w);
                pos++;
                w &= w - 1;
            }
        }
    }
}

} // namespace

LaunchPlan plan_points_rows(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.n_frames * g.height, kPtsBlock / 64, 1u << 16);
}
LaunchPlan plan_scan_frames(int n_frames) { return capped_plan((unsigned long long)n_frames, 256, 1); }

hipError_t launch_points_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, uint32_t *row_counts,
                               hipStream_t stream)
{
    const int row_bytes = (g.width + 7) / 8;
    const unsigned grid = plan_points_rows(g).grid;
    if (bits)
        hipLaunchKernelGGL(points_count_kernel<true>, dim3(grid), dim3(kPtsBlock), 0, stream, (const void *)bits, g,
                           row_bytes, row_counts);
    else
        hipLaunchKernelGGL(points_count_kernel<false>, dim3(grid), dim3(kPtsBlock), 0, stream, (const void *)strong, g,
                           row_bytes, row_counts);
    return hipGetLastError();
}

hipError_t launch_points_scan(uint32_t *rows, unsigned long long *frame_totals, unsigned long long *offsets, int height,
                              int n_frames, hipStream_t stream)
{
    hipLaunchKernelGGL(points_scan_rows_kernel, dim3(n_frames), dim3(256), 0, stream, rows, frame_totals, height);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(points_scan_frames_kernel, dim3(plan_scan_frames(n_frames).grid), dim3(256), 0, stream,
                       frame_totals, offsets, n_frames);
    return hipGetLastError();
}

hipError_t launch_points_scatter(const uint64_t *strong, const uint8_t *bits, const HystGeom &g,
                                 const uint32_t *row_offsets, const unsigned long long *offsets, uint32_t *points,
                                 unsigned long long capacity, hipStream_t stream)
{
    if (capacity == 0) return hipSuccess;
    const int row_bytes = (g.width + 7) / 8;
    const unsigned grid = plan_points_rows(g).grid;
    if (bits)
        hipLaunchKernelGGL(points_scatter_kernel<true>, dim3(grid), dim3(kPtsBlock), 0, stream, (const void *)bits, g,
                           row_bytes, row_offsets, offsets, points, capacity);
    else
        hipLaunchKernelGGL(points_scatter_kernel<false>, dim3(grid), dim3(kPtsBlock), 0, stream, (const void *)strong, g,
                           row_bytes, row_offsets, offsets, points, capacity);
    return hipGetLastError();
}

} // namespace canny
