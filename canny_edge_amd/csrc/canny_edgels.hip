// canny_edgels.hip -- sub-pixel edgels: one 16-byte record per edge pixel (position along the gradient to 1/256 pixel,
// gradient pair, magnitude to 1/16 grey level, direction, flags).  The rule is part of the interface (include/canny_hip.h,
// DESIGN.md section 23); tests/edgels_rule.py restates it in numpy / Python ints, canny_edgels_host.cpp in plain C++.
//
// Two kernels, both without atomics and without a host round trip:
//   rows : behind the point lists' count + scan (canny_points.hip).  One wave per image row, as there: a row owns a
//          contiguous run of the output.  The wave loads the row's words (64 per round), the shuffle ladder of
//          points_scatter_kernel gives each word its offset, and the lanes write the columns of their set bits into a
//          per-wave LDS queue.  Then ALL 64 lanes take queue entries i = lane, lane + 64, ...: the refinement (three Sobel
//          pairs, three exact roots, one division) runs on full waves however the bits are spread over the words, and
//          consecutive lanes store consecutive records.  Only the cheap expansion into the queue runs on the few lanes
//          whose words hold bits (DESIGN.md section 13 measured a vote kernel of that shape as bound by nearly empty
//          wave instructions).
//          The queue of a round is 4096 two-byte entries = 8 KiB per wave; four waves per workgroup = 32 KiB, so five
//          workgroups = 20 waves share a CU's 160 KiB (5 waves per SIMD).  The queue is private to its wave: LDS
//          instructions of one wave execute in order, so a wavefront fence (for the compiler) is all the ordering needed,
//          and the waves of a workgroup never wait for one another.
//   at   : one lane per entry of a caller's index list, grid (blocks, n_frames), grid-stride over the frame's range; the
//          index is tested against height * width before any address is formed.
#include "canny_line_support.h"

namespace canny {

namespace {

constexpr int kEdgelBlock = 256;                 // 4 waves, one image row each
constexpr int kEdgelWaves = kEdgelBlock / 64;
constexpr int kEdgelQueue = 64 * 64;             // every pixel of a round's 64 words set
constexpr int kAtBlock = 256;

// edgel_mag_q4, edgel_dir, edgel_offset and edgel_record live in canny_line_support.h: the line fits sum the same records.

// one wave per image row; grid-stride over the rows of the batch
template <class T>
__global__ __launch_bounds__(kEdgelBlock) void edgels_rows_kernel(const uint64_t *__restrict__ strong, HystGeom g,
                                                                  const T *__restrict__ plane,
                                                                  const uint32_t *__restrict__ row_offsets,
                                                                  const unsigned long long *__restrict__ offsets,
                                                                  uint4 *__restrict__ edgels, uint32_t *__restrict__ points,
                                                                  unsigned long long capacity)
{
    __shared__ uint16_t s_queue[kEdgelWaves][kEdgelQueue];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t *queue = s_queue[wave];
    const int h = g.height, w = g.width;
    const size_t n_rows = (size_t)g.n_frames * h;
    const size_t wave_stride = (size_t)gridDim.x * kEdgelWaves;
    for (size_t r = (size_t)blockIdx.x * kEdgelWaves + wave; r < n_rows; r += wave_stride) {
        const int f = (int)(r / (size_t)h), y = (int)(r - (size_t)f * h);
        unsigned long long run = offsets[f] + row_offsets[r]; // where this row's run starts (wave-uniform)
        const T *img = plane + (size_t)f * h * w;
        for (int k0 = 0; k0 < g.tiles_x && run < capacity; k0 += 64) { // rows wider than 4096 pixels take several rounds
            const int k = k0 + lane;
            uint64_t bits = k < g.tiles_x ? row_word<false>(strong, g, 0, f, y, k) : 0ull;
            const unsigned c = (unsigned)__popcll(bits);
            unsigned incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            const unsigned total = __shfl(incl, 63); // <= 4096
            unsigned at = incl - c;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the last round's queue reads come first
            while (bits) {
                queue[at++] = (uint16_t)((lane << 6) | __builtin_ctzll(bits));
                bits &= bits - 1;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the queue is written before any lane reads it
            for (unsigned i = lane; i < total; i += 64) {
                const unsigned long long pos = run + i;
                if (pos >= capacity) break;
                const int x = (k0 << 6) + (int)queue[i];
                edgels[pos] = edgel_record(img, h, w, y, x);
                if (points) points[pos] = (uint32_t)y * (uint32_t)w + (uint32_t)x;
            }
            run += total;
        }
    }
}

// grid (blocks, n_frames): one lane per point of the frame's range
template <class T>
__global__ __launch_bounds__(kAtBlock) void edgels_at_kernel(const T *__restrict__ plane, int h, int w,
                                                             const uint32_t *__restrict__ points,
                                                             const unsigned long long *__restrict__ offsets,
                                                             uint4 *__restrict__ edgels, unsigned long long capacity)
{
    const int f = blockIdx.y;
    const unsigned long long lo = offsets[f], end = offsets[f + 1];
    const unsigned long long hi = end < capacity ? end : capacity;
    const uint32_t frame_px = (uint32_t)h * (uint32_t)w; // < 2^31
    const T *img = plane + (size_t)f * frame_px;
    for (unsigned long long q = lo + (unsigned long long)blockIdx.x * kAtBlock + threadIdx.x; q < hi;
         q += (unsigned long long)gridDim.x * kAtBlock) {
        const uint32_t p = points[q];
        uint4 rec = make_uint4(0u, 0u, 0u, CANNY_HIP_EDGEL_INVALID);
        if (p < frame_px) { // the only place an index becomes an address
            const int y = (int)(p / (uint32_t)w);
            rec = edgel_record(img, h, w, y, (int)(p - (uint32_t)y * (uint32_t)w));
        }
        edgels[q] = rec;
    }
}

__global__ __launch_bounds__(256) void edgels_arith_pairs_kernel(const int16_t *__restrict__ gx,
                                                                 const int16_t *__restrict__ gy, size_t n,
                                                                 uint32_t *__restrict__ mag, int *__restrict__ dir)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        mag[i] = edgel_mag_q4(gx[i], gy[i]);
        dir[i] = edgel_dir(gx[i], gy[i]);
    }
}

__global__ __launch_bounds__(256) void edgels_arith_triples_kernel(const uint32_t *__restrict__ abc, size_t n,
                                                                   int *__restrict__ t, int *__restrict__ refined)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        bool ok;
        t[i] = edgel_offset(abc[3 * i], abc[3 * i + 1], abc[3 * i + 2], &ok);
        refined[i] = ok;
    }
}

} // namespace

LaunchPlan plan_edgels_at(int height, int width, unsigned long long n_points)
{
    return sized_plan(n_points, kAtBlock, (unsigned long long)height * width, 1024, 1024);
}
LaunchPlan plan_edgels_arith(size_t n) { return capped_plan(n, 256, 8192); }

hipError_t launch_edgels_rows(const uint64_t *strong, const HystGeom &g, const void *plane, bool plane_u8,
                              const uint32_t *row_offsets, const unsigned long long *offsets, int *edgels,
                              uint32_t *points, unsigned long long capacity, hipStream_t stream)
{
    if (capacity == 0) return hipSuccess;
    // the rows of plan_points_rows, four to a workgroup here: the same rows per trip, so the plan's trips hold
    const LaunchPlan p = plan_points_rows(g);
    const unsigned grid = p.grid * (p.per_group / kEdgelWaves);
    if (plane_u8)
        hipLaunchKernelGGL(edgels_rows_kernel<uint8_t>, dim3(grid), dim3(kEdgelBlock), 0, stream, strong, g,
                           (const uint8_t *)plane, row_offsets, offsets, (uint4 *)edgels, points, capacity);
    else
        hipLaunchKernelGGL(edgels_rows_kernel<int16_t>, dim3(grid), dim3(kEdgelBlock), 0, stream, strong, g,
                           (const int16_t *)plane, row_offsets, offsets, (uint4 *)edgels, points, capacity);
    return hipGetLastError();
}

hipError_t launch_edgels_at(const void *plane, bool plane_u8, int height, int width, int n_frames, const uint32_t *points,
                            const unsigned long long *offsets, int *edgels, unsigned long long capacity,
                            hipStream_t stream)
{
    if (capacity == 0) return hipSuccess;
    const dim3 grid(plan_edgels_at(height, width, 1).grid, n_frames);
    if (plane_u8)
        hipLaunchKernelGGL(edgels_at_kernel<uint8_t>, grid, dim3(kAtBlock), 0, stream, (const uint8_t *)plane, height,
                           width, points, offsets, (uint4 *)edgels, capacity);
    else
        hipLaunchKernelGGL(edgels_at_kernel<int16_t>, grid, dim3(kAtBlock), 0, stream, (const int16_t *)plane, height,
                           width, points, offsets, (uint4 *)edgels, capacity);
    return hipGetLastError();
}

hipError_t launch_edgels_arith(const int16_t *gx, const int16_t *gy, size_t n_pairs, uint32_t *mag, int *dir,
                               const uint32_t *abc, size_t n_triples, int *t, int *refined, hipStream_t stream)
{
    if (n_pairs) {
        hipLaunchKernelGGL(edgels_arith_pairs_kernel, dim3(plan_edgels_arith(n_pairs).grid), dim3(256), 0, stream, gx, gy,
                           n_pairs, mag, dir);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n_triples)
        hipLaunchKernelGGL(edgels_arith_triples_kernel, dim3(plan_edgels_arith(n_triples).grid), dim3(256), 0, stream, abc,
                           n_triples, t, refined);
    return hipGetLastError();
}

} // namespace canny
